"""CPU-side checks of adaptive sampling (fw_render_adaptive): the export at ABI 8, the argument and no-device errors (checked before the
scene is looked at), the CLI's flag conflicts, and the numpy twin of the convergence rule and the round schedule that
tests/test_gpu_adaptive.py replays the device against."""
import ctypes as C

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes

F = np.float32


def converged(S, Q, n, tol):
    """The rule of include/firework_hip.h in float32, IEEE, one rounding per operation.  S, Q: (..., 3) sums and sums of squares of n
    samples.  -> bool (...)"""
    S = np.asarray(S, F)
    Q = np.asarray(Q, F)
    nf = F(n)
    with np.errstate(all="ignore"):
        m = S / nf
        v = (Q - S * m) / (nf - F(1))
        L = ((m[..., 0] + m[..., 1]) + m[..., 2]) / F(3)
        t = F(tol) * np.where(L > F(1 / 256), L, F(1 / 256)).astype(F)
        lim = (t * t) * nf
        finite = np.isfinite(S).all(-1) & np.isfinite(Q).all(-1)
        return finite & (v <= lim[..., None]).all(-1)


def schedule(min_samples, cap):
    """The sample counts after each round: min, 2 min, 4 min, ..., cap"""
    out = [min_samples]
    while out[-1] < cap:
        out.append(min(2 * out[-1], cap))
    return out


def replay(colors, tol, min_samples, cap):
    """colors: (P, cap, 3) float32 per-sample colours in sample order.  Replays the sums, squares and round decisions as the device
    makes them.  -> (S, Q, counts, round_pixels)"""
    P = colors.shape[0]
    S = np.zeros((P, 3), F)
    Q = np.zeros((P, 3), F)
    counts = np.zeros(P, np.uint32)
    active = np.arange(P)
    rounds = []
    done = 0
    for target in schedule(min_samples, cap):
        if active.size == 0:
            break
        rounds.append(int(active.size))
        for s in range(done, target):
            v = colors[active, s]
            S[active] += v
            Q[active] += v * v
        done = target
        counts[active] = target
        keep = ~converged(S[active], Q[active], target, tol) if target < cap else np.zeros(active.size, bool)
        active = active[keep]
    return S, Q, counts, rounds + [0] * (32 - len(rounds))


def test_adaptive_export_at_abi_8():
    lib = _lib.load()
    assert hasattr(lib, "fw_render_adaptive")
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION


def _call(scene, p, tol=0.05, min_samples=4):
    lib = _lib.load()
    return lib.fw_render_adaptive(scene, None if p is None else C.byref(p), tol, min_samples, None, None, None, None, None, None, None)


def test_adaptive_argument_checks():
    """Every argument error is FW_ERR_BAD_ARG before the scene is dereferenced: a pointer to 64 bytes that are not a scene stands in."""
    not_a_scene = C.addressof(C.create_string_buffer(64))
    _s, r = scenes.cornell_box()

    def params(samples=64, **kw):
        p = r.width(8).height(8).samples(samples).to_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    ids = np.arange(4, dtype=np.uint32)
    with_ids = params()
    with_ids.pixel_ids = ids.ctypes.data_as(C.POINTER(C.c_uint32))
    with_ids.n_pixels = 4
    assert _call(None, params()) == A.FW_ERR_BAD_ARG                                  # null scene
    assert _call(not_a_scene, None) == A.FW_ERR_BAD_ARG                               # null params
    assert _call(not_a_scene, with_ids) == A.FW_ERR_BAD_ARG                           # pixel subsets
    assert _call(not_a_scene, params(), min_samples=1) == A.FW_ERR_BAD_ARG            # min_samples < 2
    assert _call(not_a_scene, params(), min_samples=0) == A.FW_ERR_BAD_ARG
    assert _call(not_a_scene, params(samples=8), min_samples=16) == A.FW_ERR_BAD_ARG  # cap < min
    assert _call(not_a_scene, params(samples=(1 << 24) + 1)) == A.FW_ERR_BAD_ARG      # cap > 2^24
    for tol in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(not_a_scene, params(), tol=tol) == A.FW_ERR_BAD_ARG, tol
    assert _call(not_a_scene, params(rng_mode=A.FW_RNG_LCG)) == A.FW_ERR_UNSUPPORTED


def test_render_adaptive_without_a_device_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene, r = scenes.cornell_box()
    with pytest.raises(_lib.FireworkError) as e:
        r.width(8).height(8).samples(16).render_adaptive(scene, 0.05, min_samples=4)
    assert e.value.status == A.FW_ERR_NO_DEVICE


def test_cli_rejects_adaptive_with_progressive_or_checkpoint(tmp_path, capsys):
    from firework_amd.__main__ import main
    for extra in (["--progressive", "2"], ["--checkpoint", str(tmp_path / "ck.npz")]):
        with pytest.raises(SystemExit) as e:
            main(["--scene-file", "s.yml", "-s", "64", "--adaptive", "0.05", "-o", str(tmp_path / "o.png")] + extra)
        assert e.value.code == 2
        assert "--adaptive" in capsys.readouterr().err


def test_rule_non_finite_sums_never_converge():
    ok = np.array([[0.5, 0.5, 0.5]], F)
    for bad in (np.nan, np.inf, -np.inf):
        for which in range(6):
            S, Q = ok.copy(), (ok * ok * 16).copy()
            (S if which < 3 else Q)[0, which % 3] = bad
            assert not converged(S * 16, Q, 16, 1e30)[0], (bad, which)
    assert converged(ok * 16, ok * ok * 16, 16, 1e-3)[0]           # the finite twin, all samples equal: v = 0


def test_rule_zero_variance_converges_at_any_tolerance():
    c = np.array([0.3, 0.7, 0.1], F)
    for n in (2, 4, 16, 1024):
        S = np.zeros(3, F)
        Q = np.zeros(3, F)
        for _ in range(n):
            S += c
            Q += c * c
        v = (Q - S * (S / F(n))) / F(n - 1)
        if (v <= 0).all():                                           # exactly constant samples (v may round to <= 0)
            assert converged(S[None], Q[None], n, 1e-30)[0]
    # black: S = Q = 0 converges (v = 0 <= anything, the floor keeps t > 0)
    assert converged(np.zeros((1, 3), F), np.zeros((1, 3), F), 4, 1e-30)[0]


def test_rule_brightness_floor():
    """Dark pixels are judged against 1/256, not against their own tiny mean."""
    n = 4
    m = F(1e-4)                                                      # L = 1e-4 << 1/256
    # v such that the standard error sqrt(v / n) sits between tol * L and tol * (1/256)
    tol = F(0.1)
    v = F(((tol * F(1 / 256)) ** 2) * n * 0.5)
    S = np.full(3, m * n, F)
    Q = (v * F(n - 1) + S * (S / F(n))).astype(F)
    assert converged(S[None], Q[None], n, tol)[0]
    vv = (Q - S * (S / F(n))) / F(n - 1)
    assert (vv > (tol * m) ** 2 * F(n)).all()                        # against its own mean alone it would go on
    # four times that variance is over the floor's limit too
    Q4 = (F(4) * v * F(n - 1) + S * (S / F(n))).astype(F)
    assert not converged(S[None], Q4[None], n, tol)[0]


def test_rule_negative_rounding_residue():
    """Q - S*m can round below zero for equal samples; v < 0 is <= any limit: converged."""
    x = F(0.1)
    n = 3
    S = F(0)
    Q = F(0)
    for _ in range(n):
        S = F(S + x)
        Q = F(Q + x * x)
    v = (Q - S * (S / F(n))) / F(n - 1)
    S3 = np.full((1, 3), S, F)
    Q3 = np.full((1, 3), Q, F)
    if v < 0:
        assert converged(S3, Q3, n, 1e-30)[0]
    # hand-made negative residue
    S3 = np.full((1, 3), F(1.0), F)
    Q3 = np.full((1, 3), F(0.25), F)                                  # Q < S^2 / n: v < 0
    assert ((Q3 - S3 * (S3 / F(2))) / F(1) < 0).all()
    assert converged(S3, Q3, 2, 1e-30)[0]


def test_schedule_and_replay():
    assert schedule(4, 64) == [4, 8, 16, 32, 64]
    assert schedule(16, 1024) == [16, 32, 64, 128, 256, 512, 1024]
    assert schedule(16, 100) == [16, 32, 64, 100]
    assert schedule(8, 8) == [8]
    assert len(schedule(2, 1 << 24)) == 1 + 23 <= 32
    rng = np.random.default_rng(1)
    P, cap = 50, 64
    colors = np.zeros((P, cap, 3), F)
    colors[:10] = F(0.5)                                              # constant: stop at min
    colors[10:20] = rng.random((10, cap, 3), dtype=F)                 # noisy: go further
    colors[20:30] = (rng.random((10, cap, 3)) < 0.02).astype(F) * F(50)   # rare fireflies
    colors[30:40, 2] = F(np.inf)                                      # non-finite from sample 2 on: to the cap
    colors[40:] = rng.random((10, cap, 3), dtype=F) * F(1e-4)         # dark noise: the floor decides
    S, Q, counts, rounds = replay(colors, 0.05, 4, cap)
    assert (counts[:10] == 4).all()
    assert (counts[30:40] == cap).all()
    assert set(np.unique(counts)) <= set(schedule(4, cap))
    assert rounds[0] == P and rounds[len(schedule(4, cap)):] == [0] * (32 - len(schedule(4, cap)))
    assert all(a >= b for a, b in zip(rounds, rounds[1:]))
    # the sums are the first counts[p] samples in order
    for p in range(P):
        s = np.zeros(3, F)
        for k in range(int(counts[p])):
            s += colors[p, k]
        assert np.array_equal(s, S[p]) or not np.isfinite(s).all()
