"""CPU-side checks of the reflection gather (fw_reflect_rays, fw_reflect_reduce, fw_bake_reflect): the exports and
fw_reflect's layout at ABI 8; every argument error of the three calls in the header's order (they come before the scene is looked at or
HIP is called) and the no-device error with the caller's buffers untouched; ReflectionGather.check; the Python entry points and the
CLI's refusals; the numpy statements — api.reflect_rays against an independent restatement built on ggx_ref, with the property the GPU
test relies on (no ray of its cases lies on the horizon), api.reflect_reduce against hand-computed cases and a plain loop written from
the statement, api.reflect_resolve — and the estimator's known answer: with L = 1 on every alive ray it estimates GgxMat's directional
albedo F0 A + B."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import ReflectionGather

import reflect_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
PI = 3.141592653589793
DIRECTIONS = [1, 3, 65, 64, 200]                                          # the gather tests' own

# The largest |estimate - (F0 A + B)| of the numpy statement over the cases of test_estimator_known_answer at D = 256, R = 4, measured on
# the CPU with this file's seed: at mu = 0.2, rho = 0.1, F0 = 1.  The tests assert twice that: the margin covers a
# change of seed; the lattice is deterministic.
ESTIMATOR_MEASURED = 1.7145e-3
ESTIMATOR_BOUND = 2.0 * ESTIMATOR_MEASURED


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.REFLECT_PROTOTYPES) == ["fw_bake_reflect", "fw_reflect_rays", "fw_reflect_reduce"]
    for name in A.REFLECT_PROTOTYPES:
        assert hasattr(lib, name), name
        assert len(re.findall(rf"\bint {name}\s*\(", text)) == 1, name


def test_struct_layout(tmp_path):
    """ctypes' fw_reflect equals the C compiler's, size and every field offset, and has fw_gather's shape"""
    names = ["directions", "jitter", "bias", "direct_bias", "flags", "chunk_points", "seed"]
    assert [f for f, _ in A.fw_reflect._fields_] == names == [f for f, _ in A.fw_gather._fields_]
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("' + "%zu " * (len(names) + 2) + '\\n",sizeof(fw_reflect)' +
           "".join(f",offsetof(fw_reflect,{f})" for f in names) + ",(size_t)FW_REFLECT_DIRECT);return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_reflect)] + [getattr(A.fw_reflect, f).offset for f in names] + [A.FW_REFLECT_DIRECT]
    g = ReflectionGather(33).bias(0.25).direct_bias(0.5).seed(7).jitter(False).to_abi()
    assert (g.directions, g.jitter, g.bias, g.direct_bias, g.flags, g.chunk_points, g.seed) == (33, 0, 0.25, 0.5, A.FW_REFLECT_DIRECT, 0, 7)
    assert ReflectionGather(33).direct_bias(0.5).direct_bias(None).to_abi().flags == 0


def test_reflection_gather_check():
    for bad, word in ((ReflectionGather(0), "directions"), (ReflectionGather((1 << 20) + 1), "directions"), (ReflectionGather(4).bias(-1.0), "bias"),
                      (ReflectionGather(4).bias(NAN), "bias"), (ReflectionGather(4).direct_bias(-1.0), "direct_bias"),
                      (ReflectionGather(4).direct_bias(INF), "direct_bias")):
        with pytest.raises(ValueError, match=word):
            bad.check()
    g = ReflectionGather(1 << 20).bias(0.0).check()
    assert g.directions == 1 << 20 and g.to_abi().flags == 0 and ReflectionGather().directions == 16


# ---- api.reflect_rays ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D, stride, with_ids, rnd, jitter", R.ray_cases())
def test_reflect_rays_equal_the_restatement_and_stay_off_the_horizon(D, stride, with_ids, rnd, jitter):
    """api.reflect_rays against ggx_ref's sampler, frame and Lambda: the same rays dead, origins, directions and weights within one
    float32 ulp (the restatement orders its operations differently; both round once).  And what the GPU test relies on: with
    reflect_ref.SEED no ray of these cases has |wi.z| or |wo.z| below 1e-9, so no ray can be dead on one side and alive on the other."""
    reflect, pos, nrm, view, spec, ids = R.case_inputs(D, stride, with_ids, jitter)
    rays, w, t = api.reflect_rays(reflect, pos, nrm, view, spec, ids, rnd, terms=True)
    ref = R.rays_ref(reflect, pos, nrm, view, spec, ids, rnd)
    n = ref["alive"].shape[0]
    assert rays.shape == (n * D, 6) and w.shape == (n * D, 2) and rays.dtype == w.dtype == np.float32 and n == (31 if with_ids else 37)
    usable = t["usable"]
    assert np.array_equal(usable, ref["usable"]) and usable.sum() == n - sum(1 for i in R.UNUSABLE if ids is None or i in ids)
    assert np.nanmin(np.abs(t["wi_z"])) >= 1e-9 and np.nanmin(np.abs(t["wo_z"])) >= 1e-9
    alive = (w[:, 0] > 0).reshape(n, D)
    assert np.array_equal(alive, ref["alive"]) and 0 < alive.sum() < usable.sum() * D          # some rays are dead, and not all
    dead = ~alive.reshape(-1)
    assert not rays[dead].any() and not w[dead].any() and not np.signbit(rays[dead]).any()
    o, d = rays[:, 0:3].reshape(n, D, 3), rays[:, 3:6].reshape(n, D, 3)
    assert np.all(np.abs(o - ref["origin"]) <= R.vector_ulp(ref["origin"]))
    assert np.all(np.abs(d - ref["direction"])[alive] <= R.vector_ulp(ref["direction"])[alive])
    assert np.all(np.abs(w[:, 0].reshape(n, D) - ref["g"])[alive] <= R.ulp32(ref["g"])[alive])
    assert np.all(np.abs(w[:, 1].reshape(n, D) - ref["s"])[alive] <= R.ulp32(ref["s"])[alive])
    assert np.all(np.abs(np.sqrt(np.sum(d.astype(np.float64) ** 2, -1))[alive] - 1.0) < 3e-7)
    # another round or seed: other rays; without ids the points are taken in order
    other, _ = api.reflect_rays(reflect, pos, nrm, view, spec, ids, rnd + 1)
    assert jitter == (not np.array_equal(other, rays))
    if ids is not None:
        everyone, _ = api.reflect_rays(reflect, pos, nrm, view, spec, None, rnd)
        assert np.array_equal(R.u32(everyone.reshape(37, D, 6)[ids]), R.u32(rays.reshape(n, D, 6)))


def test_reflect_rays_mirror_a_smooth_surface():
    """a nearly smooth floor seen at 45 degrees reflects about its normal; seen from below the stored normal the frame turns over"""
    reflect = ReflectionGather(8).bias(0.5).seed(3)
    for normal in ((0.0, 2.0, 0.0), (0.0, -2.0, 0.0)):
        rays, w = api.reflect_rays(reflect, [[1.0, 0.0, 2.0]], [normal], [[3.0, -3.0, 0.0]], [[1.0, 1.0, 1.0, 0.03]])
        assert np.all(w[:, 0] > 0.99) and np.all(w[:, 0] <= 1.0) and np.all(w[:, 1] < 0.01)
        assert np.allclose(rays[:, 0:3], [1.0, 0.5, 2.0]) and np.allclose(rays[:, 3:6], np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0), atol=5e-3)


# ---- api.reflect_reduce, api.reflect_resolve -------------------------------------------------------------------------------------------
def _record(kind, albedo=(0, 0, 0), emitted=(0, 0, 0)):
    r = np.full(16, NAN, np.float32)
    r[0:3], r[3], r[12:15] = albedo, kind, emitted
    return r


def test_reflect_reduce_by_hand():
    g, s = np.float32(0.75), np.float32(0.25)
    wa, wb = float(g) * (1.0 - float(s)), float(g) * float(s)
    # D = 1: one diffuse ray: L = (a max(E, 0)) (1 / pi), P = (g (1 - s)) L, Q = (g s) L, alive 1, sky 0
    rec = _record(0, (0.5, 0.25, 1.0))[None]
    out = api.reflect_reduce(rec, [[2.0, 4.0, -3.0]], [[g, s]], 1)
    assert out.shape == (1, 8) and out.dtype == np.float64
    L = [(0.5 * 2.0) * (1.0 / PI), (0.25 * 4.0) * (1.0 / PI), 0.0]
    assert np.array_equal(out[0], [wa * L[0], wa * L[1], wa * L[2], 1.0, wb * L[0], wb * L[1], wb * L[2], 0.0])
    # ... with direct: T = max(E, 0) + Ed, Ed added after the clamp
    ed = np.array([[1.0, 0.5, 2.0, NAN, NAN, NAN, NAN, NAN]], np.float32)
    out = api.reflect_reduce(rec, [[2.0, 4.0, -3.0]], [[g, s]], 1, direct=ed)
    L = [(0.5 * 3.0) * (1.0 / PI), (0.25 * 4.5) * (1.0 / PI), (1.0 * 2.0) * (1.0 / PI)]
    assert np.array_equal(out[0], [wa * L[0], wa * L[1], wa * L[2], 1.0, wb * L[0], wb * L[1], wb * L[2], 0.0])
    # D = 2: the environment (sky) and a dead ray: G = 2, the butterfly adds lane 0 and lane 1
    rec = np.stack([_record(-1, (9, 9, 9), (1.0, 2.0, 3.0)), _record(-2, (9, 9, 9), (7.0, 7.0, 7.0))])
    out = api.reflect_reduce(rec, np.full((2, 3), NAN, np.float32), [[g, s], [0.0, 0.0]], 2)
    assert np.array_equal(out[0], [0.5 * (wa * 1.0), 0.5 * (wa * 2.0), 0.5 * (wa * 3.0), 0.5, 0.5 * (wb * 1.0), 0.5 * (wb * 2.0), 0.5 * (wb * 3.0), 0.5])
    # D = 3: an emitter (not clamped, its albedo and E ignored), a diffuse hit, and a ray whose record names no material (kind -2) but
    # that did leave the surface (g > 0): it counts as alive and brings nothing.  G = 4: (l0 + l2) + (l1 + l3)
    rec = np.stack([_record(3, (9, 9, 9), (15.0, 0.0, 2.0)), _record(5, (1.0, 1.0, 0.0)), _record(-2)])
    E = np.array([[NAN, NAN, NAN], [PI, 2 * PI, 5.0], [NAN, NAN, NAN]], np.float32)
    e = E.astype(np.float64)
    w = np.array([[1.0, 0.0], [g, s], [0.5, 0.5]], np.float32)
    out = api.reflect_reduce(rec, E, w, 3)
    third = 1.0 / 3
    want = [third * ((15.0 + 0.0) + (wa * ((1.0 * e[1, 0]) * (1.0 / PI)) + 0.0)), third * ((0.0 + 0.0) + (wa * ((1.0 * e[1, 1]) * (1.0 / PI)) + 0.0)),
            third * ((2.0 + 0.0) + (0.0 + 0.0)), third * ((1.0 + 1.0) + (1.0 + 0.0)),
            third * ((0.0 + 0.0) + (wb * ((1.0 * e[1, 0]) * (1.0 / PI)) + 0.0)), third * ((0.0 + 0.0) + (wb * ((1.0 * e[1, 1]) * (1.0 / PI)) + 0.0)), 0.0, 0.0]
    assert np.array_equal(out[0], want)
    # two points: each is its own
    both = api.reflect_reduce(np.concatenate([rec, rec[::-1]]), np.concatenate([E, E[::-1]]), np.concatenate([w, w[::-1]]), 3)
    assert np.array_equal(both[0], out[0]) and both[1, 3] == 1.0


@pytest.mark.parametrize("D", DIRECTIONS)
def test_reflect_reduce_keeps_the_statements_order(D):
    """bit for bit a plain loop over Python floats: G partial sums in ascending j, then the xor butterfly"""
    rng = np.random.default_rng(D)
    s, E, Ed = R.synthetic_records(6, D, rng, unusable=1)
    w, s = R.synthetic_weights(6, D, rng, s)
    w.reshape(6, D, 2)[-1] = 0.0
    for direct in (None, Ed):
        got, want = api.reflect_reduce(s, E, w, D, direct), R.reduce_loop(s, E, w, D, direct)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (D, direct is None)
        assert np.all(got[-1] == 0.0) and np.all(np.isfinite(got))


def test_reflect_resolve():
    sums = np.array([[3.0, 1.0, 0.5, 2.0, 0.25, 0.5, 1.0, 1.0], [0.0] * 8], np.float32)
    spec = np.array([[0.5, 1.0, 0.04, 0.3], [0.9, 0.9, 0.9, 0.0]], np.float32)
    out = api.reflect_resolve(sums, spec, 3)
    f0 = spec[0, 0:3].astype(np.float64)
    assert out.dtype == np.float32 and out.shape == (2, 4) and np.all(out[1] == 0.0)
    assert np.array_equal(out[0], np.concatenate([(f0 * [3.0, 1.0, 0.5] + [0.25, 0.5, 1.0]) / 3.0, [2.0 / 3.0]]).astype(np.float32))
    assert np.array_equal(api.reflect_resolve(sums.reshape(1, 2, 8), spec.reshape(1, 2, 4), 3), out.reshape(1, 2, 4))


# ---- the estimator's known answer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", [0.2, 0.7, 1.0])
@pytest.mark.parametrize("rho", [0.1, 0.3, 1.0])
def test_estimator_known_answer(mu, rho):
    """L = 1 on every alive ray: (f0 P + Q) over 4 rounds of 256 rays estimates F0 A + B of api.ggx_terms"""
    A_, B_ = api.ggx_terms([mu], [rho])[0].astype(np.float64)
    for f0 in (0.04, 1.0):
        got = R.estimate(mu, rho, f0, 256, 4)
        print(f"mu {mu} rho {rho} F0 {f0}: estimate {got:.7f}, F0 A + B {f0 * A_ + B_:.7f}, error {abs(got - (f0 * A_ + B_)):.3e}")
        assert abs(got - (f0 * A_ + B_)) <= ESTIMATOR_BOUND, (mu, rho, f0)


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def _said(lib, st, word):
    """the status and that the detail string names `word`: which check fired"""
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def _reflect(directions=5, bias=1e-3, direct_bias=1e-3, flags=0):
    g = A.fw_reflect()
    g.directions, g.jitter, g.bias, g.direct_bias, g.flags = directions, 1, bias, direct_bias, flags
    return g


BAD_DESCRIPTIONS = (("directions", dict(directions=0)), ("directions", dict(directions=(1 << 20) + 1)), ("bias", dict(bias=-0.5)), ("bias", dict(bias=NAN)),
                    ("direct_bias", dict(direct_bias=-1.0)), ("direct_bias", dict(direct_bias=INF)))


def test_reflect_rays_argument_checks():
    lib = _lib.load()
    buf = dict(pos=np.full((4, 3), 7.0, np.float32), nrm=np.full((4, 3), 7.0, np.float32), view=np.full((4, 3), 7.0, np.float32),
               spec=np.full((4, 4), 7.0, np.float32), rays=np.full((4 * 5, 6), 7.0, np.float32), weights=np.full((4 * 5, 2), 7.0, np.float32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}

    def call(g=None, n=4, stride=3, view_stride=3, device=0, on_device=0, ids_p=None, null_g=False, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_reflect_rays(None if null_g else C.byref(g if g is not None else _reflect()), device, 0, n, a["pos"], a["nrm"], stride, ids_p,
                                   a["view"], view_stride, a["spec"], a["rays"], a["weights"], on_device, None)

    assert _said(lib, call(null_g=True, n=0), "null") == A.FW_ERR_BAD_ARG
    for name in good:
        assert _said(lib, call(_reflect(directions=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name    # NULL before the description
    for word, kw in BAD_DESCRIPTIONS:
        assert _said(lib, call(_reflect(**kw), n=0), word) == A.FW_ERR_BAD_ARG, word                          # the description before n
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, view_stride=2), "stride_floats") == A.FW_ERR_BAD_ARG and "view" not in lib.fw_last_error().decode()
    assert _said(lib, call(view_stride=2, on_device=1, spec=C.c_void_p(good["spec"] + 4)), "view_stride") == A.FW_ERR_BAD_ARG
    for name, off in (("spec", 4), ("spec", 8), ("weights", 4), ("pos", 2), ("nrm", 2), ("view", 2), ("rays", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    big = _reflect(directions=1 << 20)
    assert _said(lib, call(big, n=1 << 11, on_device=1, spec=C.c_void_p(good["spec"] + 4)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(big, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(big, n=1 << 11, device=-1), "directions must be below") == A.FW_ERR_UNSUPPORTED   # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_reflect_reduce_argument_checks():
    lib = _lib.load()
    buf = dict(surface=np.full((4 * 5, 16), 7.0, np.float32), irr=np.full((4 * 5, 3), 7.0, np.float32), direct=np.full((4 * 5, 8), 7.0, np.float32),
               weights=np.full((4 * 5, 2), 7.0, np.float32), sums=np.full((4, 8), 7.0, np.float32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}

    def call(D=5, n=4, device=0, on_device=0, ids_p=None, **ptrs):
        a = dict(good, **ptrs)
        return lib.fw_reflect_reduce(device, D, n, ids_p, a["surface"], a["irr"], a["direct"], a["weights"], a["sums"], on_device, None)

    for name in ("surface", "irr", "weights", "sums"):
        assert _said(lib, call(D=0, **{name: None}), "null") == A.FW_ERR_BAD_ARG, name           # NULL before the directions
    for D in (0, (1 << 20) + 1):
        assert _said(lib, call(D=D, n=0), "directions") == A.FW_ERR_BAD_ARG                      # the directions before n
    assert _said(lib, call(n=0, device=-1), "n must") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("surface", 4), ("surface", 8), ("weights", 4), ("irr", 2), ("direct", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(D=1 << 20, n=1 << 11, on_device=1, sums=C.c_void_p(good["sums"] + 4)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(D=1 << 20, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(D=1 << 20, n=1 << 11, device=-1), "directions must be below") == A.FW_ERR_UNSUPPORTED    # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data, direct=None) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def _grid(counts=(2, 2, 2), lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), flags=A.FW_PROBE_WRAP):
    g = A.fw_probe_grid()
    for k in range(3):
        g.lo[k], g.hi[k], g.counts[k] = lo[k], hi[k], counts[k]
    g.flags = flags
    return g


def _depth(resolution=8):
    d = A.fw_probe_depth()
    d.resolution, d.sharpness_log2, d.max_distance = resolution, 0, 10.0
    return d


def test_bake_reflect_argument_checks():
    """fw_bake_gather's order with view and spec among the NULL and alignment checks and view_stride_floats after stride_floats"""
    lib = _lib.load()
    buf = dict(pos=np.full((4, 3), 7.0, np.float32), nrm=np.full((4, 3), 7.0, np.float32), view=np.full((4, 3), 7.0, np.float32),
               spec=np.full((4, 4), 7.0, np.float32), sums=np.full((4, 8), 7.0, np.float32), out=np.full((4, 4), 7.0, np.float32),
               sh=np.full((8, 9, 3), 7.0, np.float32), moments=np.full((8, 8, 8, 2), 7.0, np.float32), placement=np.full((8, 4), 7.0, np.float32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}
    scene = C.c_void_p(0x1000)                                                           # never dereferenced by a refused call

    def call(g=None, n=4, stride=3, view_stride=3, first=0, rounds=1, on_device=0, null=None, ids_p=None, grid=None, pd=None, normal_bias=0.0,
             with_moments=False, with_placement=False, **ptrs):
        a = dict(good, **ptrs)
        tp = A.fw_trace_params()
        tp.use_bvh, tp.on_device = 1, on_device
        args = dict(scene=scene, g=C.byref(g if g is not None else _reflect()), tp=C.byref(tp), grid=C.byref(grid if grid is not None else _grid()))
        if null:
            args[null] = None
        return lib.fw_bake_reflect(args["scene"], args["g"], args["tp"], args["grid"], a["sh"], None if pd is None else C.byref(pd),
                                   a["moments"] if with_moments else None, normal_bias, a["placement"] if with_placement else None, n, a["pos"],
                                   a["nrm"], stride, ids_p, a["view"], view_stride, a["spec"], first, rounds, a["sums"], a["out"], None)

    for null in ("scene", "g", "tp"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("pos", "nrm", "view", "spec"):
        assert _said(lib, call(_reflect(directions=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for word, kw in BAD_DESCRIPTIONS:
        assert _said(lib, call(_reflect(**kw), n=0), word) == A.FW_ERR_BAD_ARG, word             # the description before n
    assert _said(lib, call(_reflect(directions=0, bias=-1.0, direct_bias=-1.0)), "directions") == A.FW_ERR_BAD_ARG
    assert "direct_bias" not in lib.fw_last_error().decode()
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, view_stride=2), "stride_floats") == A.FW_ERR_BAD_ARG and "view" not in lib.fw_last_error().decode()
    assert _said(lib, call(view_stride=2, rounds=0), "view_stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(rounds=0, first=0xFFFFFFFF), "rounds must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=0xFFFFFFFF, rounds=1, sums=None), "overflows") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=2, sums=None, on_device=1, out=C.c_void_p(good["out"] + 4)), "first_round > 0") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("out", 4), ("out", 8), ("spec", 4), ("spec", 8), ("pos", 2), ("nrm", 2), ("view", 2)):
        assert _said(lib, call(on_device=1, null="grid", **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2), null="grid"), "aligned") == A.FW_ERR_BAD_ARG
    # the probes, after the points: NULL grid or sh, one of pd / moments without the other, the depth description, normal_bias, the grid
    flagged = _reflect(flags=2)
    assert _said(lib, call(flagged, null="grid"), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, sh=None), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, pd=_depth()), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, with_moments=True), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, pd=_depth(5), with_moments=True), "resolution") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, pd=_depth(), with_moments=True, normal_bias=-1.0), "normal_bias") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flagged, grid=_grid(counts=(0, 2, 2))), "count") == A.FW_ERR_BAD_ARG
    for name in ("sh", "moments", "placement"):
        st = call(flagged, on_device=1, pd=_depth(), with_moments=True, with_placement=True, **{name: C.c_void_p(good[name] + 2)})
        assert _said(lib, st, "aligned") == A.FW_ERR_BAD_ARG, name
    # unknown flag bits, after the probes and before the sizes
    big = _reflect(directions=1 << 20, flags=2)
    assert _said(lib, call(big, n=1 << 11), "reflect flags") == A.FW_ERR_BAD_ARG
    big.flags = A.FW_REFLECT_DIRECT
    assert _said(lib, call(big, n=1 << 11, rounds=0), "rounds must") == A.FW_ERR_BAD_ARG          # bad arguments before the size
    assert _said(lib, call(big, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(grid=_grid(counts=(1 << 11, 1 << 10, 1 << 10))), "below 2^31") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(sums=None, out=None) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert call(_reflect(flags=A.FW_REFLECT_DIRECT), pd=_depth(), with_moments=True, with_placement=True) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())


def test_python_entry_points_check_and_fail_loudly():
    rng = np.random.default_rng(0)
    s, E, Ed = R.synthetic_records(2, 4, rng, unusable=0)
    w, s = R.synthetic_weights(2, 4, rng, s)
    with pytest.raises(ValueError, match="surface"):
        _lib.reflect_reduce(s[:7], E[:7], w[:7], 4, np.zeros((2, 8), np.float32))
    with pytest.raises(ValueError, match="sums"):
        _lib.reflect_reduce(s, E, w, 4, np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match="weights"):
        _lib.reflect_reduce(s, E, w[:7], 4, np.zeros((2, 8), np.float32))
    with pytest.raises(ValueError, match="id"):
        _lib.reflect_reduce(s, E, w, 4, np.zeros((2, 8), np.float32), ids=np.array([0, 2], np.uint32))
    pos, nrm, view, spec = np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32), np.ones((3, 3), np.float32), np.ones((3, 4), np.float32)
    with pytest.raises(ValueError, match="view and spec"):
        _lib.reflect_rays(ReflectionGather(4), pos, nrm, None, spec)
    with pytest.raises(ValueError, match="view and spec"):
        _lib.reflect_rays(ReflectionGather(4), pos, nrm, view, None)
    with pytest.raises(ValueError, match="spec"):
        _lib.reflect_rays(ReflectionGather(4), pos, nrm, view, spec[:2])
    with pytest.raises(ValueError, match="weights"):
        _lib.reflect_rays(ReflectionGather(4), pos, nrm, view, spec, weights=np.zeros((12, 3), np.float32))
    with pytest.raises(ValueError, match="directions"):
        api.Renderer.default().render_reflect(None, ReflectionGather(0), None, None)
    r = api.Renderer.default()
    grid = api.ProbeGrid((0, 0, 0), (1, 1, 1), (1, 1, 1))
    for kw in (dict(ao=api.AmbientOcclusion(1.0)), dict(radiance=api.ProbeRadiance(4, 2, [0.5]), maps=np.zeros((1, 1, 4), np.float32))):
        with pytest.raises(ValueError, match="reflect cannot be combined"):
            r.render_probe_lit(None, grid, np.zeros((1, 9, 3), np.float32), reflect=ReflectionGather(4), **kw)
    with pytest.raises(ValueError, match="directions"):
        r.render_probe_lit(None, grid, np.zeros((1, 9, 3), np.float32), reflect=ReflectionGather(0))
    if _lib.device_count() == 0:
        with pytest.raises(_lib.FireworkError) as e:
            _lib.reflect_reduce(s, E, w, 4, np.zeros((2, 8), np.float32), direct=Ed)
        assert e.value.status == A.FW_ERR_NO_DEVICE
        with pytest.raises(_lib.FireworkError) as e:
            _lib.reflect_rays(ReflectionGather(4), pos, nrm, view, spec)
        assert e.value.status == A.FW_ERR_NO_DEVICE


# ---- the CLI's refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, word", [
    (["--probe-reflect", "16", "-o", "x.png"], "needs --probe-lit"), (["--reflect-bias", "0.1", "--probe-lit", "p.npz", "-o", "x.png"], "needs --probe-reflect"),
    (["--probe-lit", "p.npz", "--probe-reflect", "16", "--ao", "2", "-o", "x.png"], "cannot be combined with --ao"),
    (["--probe-lit", "p.npz", "--probe-reflect", "16", "--probe-split-sum", "-o", "x.png"], "cannot be combined with --probe-split-sum"),
    (["--probe-lit", "p.npz", "--probe-reflect", "0", "-o", "x.png"], "D[,ROUNDS]"), (["--probe-lit", "p.npz", "--probe-reflect", "x", "-o", "x.png"], "D[,ROUNDS]"),
    (["--probe-lit", "p.npz", "--probe-reflect", str((1 << 20) + 1), "-o", "x.png"], "D[,ROUNDS]"),
    (["--probe-lit", "p.npz", "--probe-reflect", "16,0", "-o", "x.png"], "D[,ROUNDS]"), (["--probe-lit", "p.npz", "--probe-reflect", "16,2,1", "-o", "x.png"], "D[,ROUNDS]"),
    (["--probe-lit", "p.npz", "--probe-reflect", "16", "--reflect-bias", "-1", "-o", "x.png"], "--reflect-bias"),
    (["--probe-lit", "p.npz", "--probe-reflect", "16", "--reflect-bias", "inf", "-o", "x.png"], "--reflect-bias"),
    (["--probe-lit", "p.npz", "--probe-reflect", "16", "--probe-gather", "8", "--ao", "2", "-o", "x.png"], "cannot be combined with --ao"),
    (["--probe-lit", "p.npz", "--probe-reflect", "16"], "-o FILE.png")])
def test_cli_refusals_come_before_the_device(args, word, capsys):
    """argparse's exit 2 with a message naming the flag; the scene file does not exist, so nothing was loaded, let alone a device asked"""
    from firework_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "none.yml", "-s", "1"] + args)
    assert e.value.code == 2 and word in capsys.readouterr().err, args


def test_cli_refuses_a_files_radiance_maps_in_use(tmp_path, capsys):
    """the probes file is looked at before the device is: radiance maps in use and --probe-reflect are a message and exit status 2"""
    from firework_amd.__main__ import main
    from firework_amd.api import ProbeRadiance
    pr = ProbeRadiance(4, 2, [0.5])
    npz = str(tmp_path / "p.npz")
    np.savez(npz, sh=np.zeros((1, 9, 3), np.float32), grid_lo=np.zeros(3), grid_hi=np.ones(3), grid_counts=np.ones(3, np.int64),
             radiance=np.zeros((1, pr.texels, 4), np.float32), radiance_res=np.int64(4), radiance_sharpness=np.int64(2),
             radiance_roughness=np.array([0.5], np.float32))
    assert main(["--scene-file", "none.yml", "-s", "1", "--probe-lit", npz, "--probe-reflect", "8", "-o", str(tmp_path / "x.png")]) == 2
    assert "--probe-reflect" in capsys.readouterr().err
