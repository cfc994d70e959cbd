"""CPU-side checks of the irradiance-probe baker (fw_probe_rays, fw_probe_project, fw_bake_probes): the exports and
fw_probe_set's layout at ABI 8, every argument error in the header's order (before the scene is looked at or HIP is called), the
no-device error with the caller's buffers left as they were, the numpy statements (ProbeSet.rays, sh_basis, sh_project, sh_irradiance)
against closed forms within the lattice's derived C / D bound (tests/probes_ref.py), ProbeSet.grid and the CLI's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import ProbeSet

import probes_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    for name, args in (("fw_probe_rays", r"const fw_probe_set \*set, int device, uint32_t round, uint32_t first_probe, uint32_t n, float \*rays, "
                                         r"int on_device, void \*stream"),
                       ("fw_probe_project", r"int device, uint32_t n_probes, uint32_t directions, uint32_t samples, const float \*rays, "
                                            r"const float \*accum, float \*sums, int on_device, void \*stream"),
                       ("fw_bake_probes", r"fw_scene \*scene, const fw_probe_set \*set, const fw_render_rays_params \*rp, uint32_t first_round, "
                                          r"uint32_t rounds, float \*sums, float \*sh, fw_stats \*stats")):
        assert hasattr(lib, name), name
        assert re.search(rf"\bint {name}\s*\({args}\);", text), name


def test_probe_set_layout(tmp_path):
    """ctypes' fw_probe_set equals the C compiler's, size and every field offset"""
    names = [f for f, _ in A.fw_probe_set._fields_]
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu' + " %zu" * len(names) +
           '\\n",sizeof(fw_probe_set)' + "".join(f",offsetof(fw_probe_set,{f})" for f in names) + ');return 0;}')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out[0] == C.sizeof(A.fw_probe_set)
    assert out[1:] == [getattr(A.fw_probe_set, f).offset for f in names]
    assert names == ["n_probes", "positions", "directions", "jitter", "seed", "chunk_probes"]


POS = np.array([[3e3, -2e3, 5e3], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [-1.0, 0.5, 2.0]], np.float32)


def _set(pos=POS, **kw):
    """a valid set of 4 probes x 8 directions, then fields overwritten; returns (struct, the array it points into)"""
    s, keep = ProbeSet(pos, 8).seed(3).to_abi()
    for k, v in kw.items():
        setattr(s, k, v)
    return s, keep


def _bad_sets():
    """(what, set) for every set error of the header, in its order"""
    out = [("null positions", _set(positions=None)), ("n_probes", _set(n_probes=0)), ("directions", _set(directions=0)),
           ("directions", _set(directions=(1 << 20) + 1))]
    for idx, v in ((0, NAN), (5, INF), (11, -INF)):
        pos = POS.copy()
        pos.reshape(-1)[idx] = v
        out.append((f"position {idx // 3}", _set(pos)))
    return out


BIG = dict(n_probes=1 << 11, directions=1 << 20)      # n_probes x D = 2^31 (the positions are never read that far: the count comes first)


def _big():
    return _set(np.zeros((1 << 11, 3), np.float32), **BIG)


def _rp(**kw):
    p = A.fw_render_rays_params()
    p.samples, p.use_bvh = 2, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_probe_rays_argument_checks():
    lib = _lib.load()
    rays = np.full((4 * 8, 6), 7.0, np.float32)

    def call(s, rnd=0, first=0, n=4, r=rays, on_device=0, ptr=None):
        return lib.fw_probe_rays(None if s is None else C.byref(s[0]), 0, rnd, first, n, ptr if ptr is not None else (None if r is None else r.ctypes.data),
                                 on_device, None)

    assert call(None) == A.FW_ERR_BAD_ARG
    assert call(_set(), r=None) == A.FW_ERR_BAD_ARG
    for what, s in _bad_sets():
        assert call(s) == A.FW_ERR_BAD_ARG, what
        if what.startswith("position"):
            assert f"probe {what.split()[1]} " in lib.fw_last_error().decode(), what          # the index is in the detail string
    assert call(_set(), n=0) == A.FW_ERR_BAD_ARG
    assert call(_set(), first=2, n=3) == A.FW_ERR_BAD_ARG                                    # past the last probe
    assert call(_set(), first=0xFFFFFFFF, n=2) == A.FW_ERR_BAD_ARG                           # (no 32-bit wrap)
    assert call(_set(), on_device=1, ptr=C.c_void_p(rays.ctypes.data + 2)) == A.FW_ERR_BAD_ARG
    # the order: bad arguments before the size limit, the size limit before the device
    assert call(_big(), n=0) == A.FW_ERR_BAD_ARG
    assert call(_big()) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call(_set()) == A.FW_ERR_NO_DEVICE
        assert call(_set(), rnd=0xFFFFFFFF, first=3, n=1) == A.FW_ERR_NO_DEVICE
        assert call(_set(directions=1 << 20, n_probes=1), n=1) == A.FW_ERR_NO_DEVICE
        assert np.all(rays == 7.0)                                                           # the caller's buffer is as it was


def test_probe_project_argument_checks():
    lib = _lib.load()
    rays = np.full((32, 6), 7.0, np.float32)
    acc = np.full((32, 4), 7.0, np.float32)
    sums = np.full((4, 9, 3), 7.0, np.float32)

    def call(n=4, d=8, s=2, r=rays, a=acc, o=sums, on_device=0, ptrs=None):
        pr, pa, po = ptrs if ptrs else (None if r is None else r.ctypes.data, None if a is None else a.ctypes.data, None if o is None else o.ctypes.data)
        return lib.fw_probe_project(0, n, d, s, pr, pa, po, on_device, None)

    assert call(r=None) == A.FW_ERR_BAD_ARG and call(a=None) == A.FW_ERR_BAD_ARG and call(o=None) == A.FW_ERR_BAD_ARG
    assert call(n=0) == A.FW_ERR_BAD_ARG
    assert call(d=0) == A.FW_ERR_BAD_ARG and call(d=(1 << 20) + 1) == A.FW_ERR_BAD_ARG
    assert call(s=0) == A.FW_ERR_BAD_ARG and call(s=(1 << 24) + 1) == A.FW_ERR_BAD_ARG
    good = (rays.ctypes.data, acc.ctypes.data, sums.ctypes.data)
    assert acc.ctypes.data % 16 == 0
    for k, off in ((0, 2), (1, 4), (2, 1)):
        ptrs = [C.c_void_p(x + (off if i == k else 0)) for i, x in enumerate(good)]
        assert call(on_device=1, ptrs=ptrs) == A.FW_ERR_BAD_ARG, k
    assert call(n=1 << 11, d=1 << 20, s=0) == A.FW_ERR_BAD_ARG
    assert call(n=1 << 11, d=1 << 20) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE
        assert np.all(sums == 7.0) and np.all(acc == 7.0)


def test_bake_probes_argument_checks():
    """a 64-byte buffer that is no scene stands in for one: nothing dereferences it before the arguments are valid and a device is found"""
    lib = _lib.load()
    not_a_scene = C.create_string_buffer(64)
    sums = np.full((4, 9, 3), 7.0, np.float32)
    sh = np.full((4, 9, 3), 7.0, np.float32)

    def call(scene, s, p, first=0, rounds=1, o=sums, h=sh, ptrs=None):
        po, ph = ptrs if ptrs else (None if o is None else o.ctypes.data, None if h is None else h.ctypes.data)
        return lib.fw_bake_probes(scene, None if s is None else C.byref(s[0]), None if p is None else C.byref(p), first, rounds, po, ph, None)

    assert call(None, _set(), _rp()) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, None, _rp()) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _set(), None) == A.FW_ERR_BAD_ARG
    for what, s in _bad_sets():
        assert call(not_a_scene, s, _rp()) == A.FW_ERR_BAD_ARG, what
    assert call(not_a_scene, _set(), _rp(), rounds=0) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _set(), _rp(), first=0xFFFFFFFF, rounds=1) == A.FW_ERR_BAD_ARG      # first_round + rounds = 2^32
    assert call(not_a_scene, _set(), _rp(samples=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _set(), _rp(samples=(1 << 24) + 1)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _set(), _rp(), first=3, o=None) == A.FW_ERR_BAD_ARG
    for ptrs in ((C.c_void_p(sums.ctypes.data + 2), C.c_void_p(sh.ctypes.data)), (C.c_void_p(sums.ctypes.data), C.c_void_p(sh.ctypes.data + 1))):
        assert call(not_a_scene, _set(), _rp(on_device=1), ptrs=ptrs) == A.FW_ERR_BAD_ARG
    # the order
    assert call(not_a_scene, _big(), _rp(), rounds=0) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _big(), _rp(samples=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _big(), _rp()) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call(not_a_scene, _set(), _rp()) == A.FW_ERR_NO_DEVICE
        # the ignored fields change nothing: n_rays, first_sample, per_sample_rays, key_base and gamma
        odd = _rp(n_rays=5, first_sample=0xFFFFFFFF, per_sample_rays=1, key_base=9, gamma=0.0)
        assert call(not_a_scene, _set(), odd, first=0xFFFFFFFE, rounds=1) == A.FW_ERR_NO_DEVICE      # the last valid round
        assert call(not_a_scene, _set(chunk_probes=3), _rp(), o=None, h=None) == A.FW_ERR_NO_DEVICE
        assert np.all(sums == 7.0) and np.all(sh == 7.0)


def test_python_entry_points_without_a_device_fail_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene, r = scenes.cornell_box()
    probes = ProbeSet(POS, 8)
    rays = probes.rays(0)
    for call in (lambda: _lib.probe_rays(probes, 0), lambda: _lib.probe_project(rays, np.zeros((32, 4), np.float32), 1, 8),
                 lambda: r.samples(2).bake_probes(scene, probes, 2)):
        with pytest.raises(_lib.FireworkError) as e:
            call()
        assert e.value.status == A.FW_ERR_NO_DEVICE


@pytest.mark.parametrize("D", [1, 63, 64, 65, 200])
def test_probe_set_rays(D):
    probes = ProbeSet(POS, D).seed(7)
    n = POS.shape[0]
    rays = probes.rays(5)
    assert rays.shape == (n * D, 6) and rays.dtype == np.float32
    assert np.array_equal(rays[:, :3].view(np.uint32), np.repeat(POS, D, axis=0).view(np.uint32))       # origins bit for bit
    d = rays[:, 3:].astype(np.float64).reshape(n, D, 3)
    assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() <= 1e-7
    if D > 1:
        assert np.all(np.diff(d[:, :, 1], axis=1) < 0.0)                                    # c strictly decreasing in j
    # rounds and seeds give different shifts, each probe its own
    s5, s6, other = probes.shifts(5), probes.shifts(6), ProbeSet(POS, D).seed(8).shifts(5)
    assert s5.shape == (n, 2) and np.all((0.0 <= s5) & (s5 < 1.0))
    assert not np.any(s5 == s6) and not np.any(s5 == other) and len({tuple(x) for x in s5}) == n
    assert np.array_equal(s5, api.pixel_jitter(7, 5, n))
    assert not np.array_equal(rays, probes.rays(6)) and not np.array_equal(rays, ProbeSet(POS, D).seed(8).rays(5))
    # jitter off: the shift (1/2, 1/2) in every round
    fixed = ProbeSet(POS, D).seed(7).jitter(False)
    assert np.all(fixed.shifts(3) == 0.5) and np.array_equal(fixed.rays(0), fixed.rays(9))
    c = fixed.rays(0)[:D, 4].astype(np.float64)
    assert np.abs(c - (1.0 - 2.0 * (np.arange(D) + 0.5) / D)).max() <= 2.0 ** -24
    m = fixed.to_abi()[0]
    assert (m.n_probes, m.directions, m.jitter, m.seed, m.chunk_probes) == (n, D, 0, 7, 0)


def _lattice(D, n=4, rounds=4, seed=3):
    """the float32 rays of n probes over some rounds, as (rounds * n, D, 3) float64 directions"""
    probes = ProbeSet(np.zeros((n, 3), np.float32), D).seed(seed)
    return np.concatenate([probes.rays(r)[:, 3:].astype(np.float64).reshape(n, D, 3) for r in range(rounds)])


def _pair(k, l):
    return lambda d: api.sh_basis(d)[..., k] * api.sh_basis(d)[..., l]


@pytest.mark.parametrize("D", [64, 256, 4096])
def test_basis_is_orthonormal_on_the_lattice(D):
    """(4 pi / D) sum_j Y_k Y_l = delta_kl within C_kl / D, C derived per product (tests/probes_ref.py); the largest C is printed beside
    the largest error x D"""
    bound = np.zeros((9, 9))
    for k in range(9):
        for l in range(k, 9):
            bound[k, l] = bound[l, k] = P.quadrature_bound(_pair(k, l), D)
    Y = api.sh_basis(_lattice(D))
    gram = (4.0 * np.pi / D) * np.einsum("pjk,pjl->pkl", Y, Y)
    err = np.abs(gram - np.eye(9)).max(axis=0)
    print(f"D {D}: largest error x D {float((err * D).max()):.3f}, largest bound x D {float((bound * D).max()):.2f}")
    assert np.all(err <= bound), (D, float((err / bound).max()))


@pytest.mark.parametrize("D", [64, 256, 4096])
def test_closed_forms_through_sh_project(D):
    n, rounds = 4, 3
    probes = ProbeSet(POS, D).seed(11)
    Lc = np.array([0.25, 1.5, 3.0])                                                        # a constant radiance
    hor, zen = np.array([1.0, 1.0, 1.0]), np.array([0.5, 0.7, 1.0])                        # the default sky
    sky = lambda d: hor + 0.5 * (d[..., 1:2] + 1.0) * (zen - hor)                          # noqa: E731
    basis_bound = [P.quadrature_bound(lambda x, k=k: api.sh_basis(x)[..., k], D) for k in range(9)]
    sky_bound = [[P.quadrature_bound(lambda x, k=k, c=c: api.sh_basis(x)[..., k] * sky(x)[..., c], D) for c in range(3)] for k in range(9)]
    normals = np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.6, 0.0, -0.8], [1.0, 2.0, -2.0] / np.float64(3.0)])
    for rnd in range(rounds):
        rays = probes.rays(rnd)
        d = rays[:, 3:].astype(np.float64)
        for S in (1, 7):
            # constant: c0 = 2 sqrt(pi) L, the rest 0
            acc = np.zeros((n * D, 4))
            acc[:, :3] = Lc * S
            got = api.sh_project(rays, acc, S, D)
            want = np.zeros((9, 3))
            want[0] = 2.0 * np.sqrt(np.pi) * Lc
            for k in range(9):
                bound = Lc.max() * basis_bound[k]
                assert np.all(np.abs(got[:, k] - want[k]) <= bound), (D, rnd, k)
            # sh_irradiance of the constant: pi L for every normal (exact up to the projection's own error, band by band)
            E = api.sh_irradiance(want, normals)
            assert np.allclose(E, np.pi * Lc, rtol=0, atol=1e-12)
            # the sky: c0 = sqrt(pi) (h + z), c1 = sqrt(pi / 3) (z - h), the rest 0
            acc[:, :3] = sky(d) * S
            got = api.sh_project(rays, acc, S, D)
            want = np.zeros((9, 3))
            want[0] = np.sqrt(np.pi) * (hor + zen)
            want[1] = np.sqrt(np.pi / 3.0) * (zen - hor)
            for k in range(9):
                for c in range(3):
                    assert np.all(np.abs(got[:, k, c] - want[k, c]) <= sky_bound[k][c]), (D, rnd, k, c)
            E = api.sh_irradiance(want, normals)
            closed = np.pi * (hor + zen) / 2.0 + (np.pi / 3.0) * (zen - hor) * normals[:, 1:2]
            assert np.allclose(E, closed, rtol=0, atol=1e-12)
    # sh_radiance reconstructs what l <= 2 can hold: the sky is linear in y
    dirs = _lattice(64, 1, 1)[0]
    assert np.allclose(api.sh_radiance(want, dirs), sky(dirs), rtol=0, atol=1e-12)


def test_probe_grid_positions():
    g = ProbeSet.grid((0.0, -1.0, 10.0), (3.0, 1.0, 10.5), (4, 3, 2), directions=32)
    assert g.n_probes == 24 and g.directions == 32 and g.positions.dtype == np.float32
    want = np.array([[x, y, z] for z in (10.0, 10.5) for y in (-1.0, 0.0, 1.0) for x in (0.0, 1.0, 2.0, 3.0)], np.float32)
    assert np.array_equal(g.positions, want)                                              # x fastest, then y, then z; corners included
    one = ProbeSet.grid((0.0, 2.0, 4.0), (1.0, 4.0, 8.0), (1, 2, 1))
    assert np.array_equal(one.positions, np.array([[0.5, 2.0, 6.0], [0.5, 4.0, 6.0]], np.float32))
    assert one.directions == 256
    with pytest.raises(ValueError):
        ProbeSet.grid((0, 0, 0), (1, 1, 1), (2, 0, 2))


def test_cli_bake_probes_checks(capsys):
    from firework_amd.__main__ import main
    base = ["--scene-file", "s.yml", "-s", "4", "--bake-probes", "2,2,2", "--probe-min", "0,0,0", "--probe-max", "1,1,1", "-o", "p.npz"]
    for extra in (["--camera", "panorama"], ["--denoise"], ["--orbit", "3"], ["--adaptive", "0.05"], ["--progressive", "2"],
                  ["--checkpoint", "c.npz"], ["--temporal"], ["--orbit", "3", "--temporal"]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
        assert "--bake-probes cannot be combined" in capsys.readouterr().err, extra
    for bad, word in ((["--bake-probes", "2,2"], "NX,NY,NZ"), (["--bake-probes", "2,0,2"], "NX,NY,NZ"), (["--bake-probes", "a,b,c"], "NX,NY,NZ"),
                      (["--probe-min", "0,0"], "--probe-min"), (["--probe-max", "0,nan,1"], "--probe-max"), (["--probe-dirs", "0"], "--probe-dirs"),
                      (["--probe-dirs", str((1 << 20) + 1)], "--probe-dirs"), (["--probe-rounds", "0"], "--probe-rounds")):
        with pytest.raises(SystemExit) as e:
            main(base + bad)                                                              # (a repeated option: the last one counts)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad
    with pytest.raises(SystemExit) as e:
        main(base[:-2])
    assert e.value.code == 2 and "-o" in capsys.readouterr().err
    for alone in (["--probe-min", "0,0,0"], ["--probe-dirs", "64"], ["--probe-rounds", "2"]):
        with pytest.raises(SystemExit) as e:
            main(["--scene-file", "s.yml", "-s", "4", "-o", "x.png"] + alone)
        assert e.value.code == 2 and "need --bake-probes" in capsys.readouterr().err
