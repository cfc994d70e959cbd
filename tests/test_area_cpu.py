"""CPU-side checks of the area lights at surface points (fw_scene_area_lights, fw_area_rays, fw_area_reduce, fw_area_mask, fw_bake_area and
FW_GATHER_NO_LIGHTS): the exports and fw_area's layout at ABI 8; every argument error of the five calls in the header's
order (they come before the scene is looked at or HIP is called) and the new flag bit beside the refused ones; AreaLight.check and
to_abi; the numpy statements — api.area_rays against closed forms with every sample visible (Lambert's polygon formula on and off
axis, a sphere wholly above the horizon, and the visible half of a half-occluded lamp), its dead cases, api.area_reduce against a plain
loop written from the statement, api.area_resolve and api.area_mask; the CLI's refusals.  fw_scene_area_lights needs a resident scene,
which only a device gives: its equality with fw_selftest_lights is tests/test_gpu_area.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import AreaLight, FinalGather

import area_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F32 = np.float32


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.AREA_PROTOTYPES) == ["fw_area_mask", "fw_area_rays", "fw_area_reduce", "fw_bake_area", "fw_scene_area_lights"]
    for name in A.AREA_PROTOTYPES:
        assert hasattr(lib, name), name
        assert len(re.findall(rf"\bint {name}\s*\(", text)) == 1, name


def test_struct_layout_and_round_trip(tmp_path):
    """ctypes' fw_area equals the C compiler's, size and every field offset; the new gather flag is bit 4 in both; to_abi round-trips"""
    names = ["samples", "jitter", "bias", "chunk_points", "seed"]
    assert [f for f, _ in A.fw_area._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("' + "%zu " * (len(names) + 3) + '\\n",sizeof(fw_area)' +
           "".join(f",offsetof(fw_area,{f})" for f in names) + ",(size_t)FW_GATHER_NO_LIGHTS,(size_t)FW_LIGHT_RECORD_FLOATS);return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_area)] + [getattr(A.fw_area, f).offset for f in names] + [A.FW_GATHER_NO_LIGHTS, A.FW_LIGHT_RECORD_FLOATS]
    assert A.FW_GATHER_NO_LIGHTS == 4
    area = AreaLight(33, 0.25).seed((7 << 32) | 5).jitter(False)
    area.chunk_points = 9
    a = area.to_abi()
    assert (a.samples, a.jitter, a.bias, a.chunk_points, a.seed) == (33, 0, 0.25, 9, (7 << 32) | 5)
    assert AreaLight().to_abi().jitter == 1 and AreaLight(bias=0.1).bias == float(F32(0.1))
    assert FinalGather(8, no_lights=True).to_abi().flags == A.FW_GATHER_NO_LIGHTS
    assert FinalGather(8, direct=True, no_lights=True).to_abi().flags == A.FW_GATHER_DIRECT | A.FW_GATHER_NO_LIGHTS
    assert FinalGather(8).to_abi().flags == 0


def test_area_light_check():
    for bad, word in ((AreaLight(0), "samples"), (AreaLight((1 << 20) + 1), "samples"), (AreaLight(4, -1.0), "bias"), (AreaLight(4, NAN), "bias"),
                      (AreaLight(4, INF), "bias")):
        with pytest.raises(ValueError, match=word):
            bad.check()
    assert AreaLight(1 << 20, 0.0).check().samples == 1 << 20


# ---- the numpy statements against closed forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.cases()))
def test_known_answers(name):
    """every sample visible (or, half-occluded, blocked as the geometry says) and the emission constant: the estimate at the tests' S and
    rounds against the closed form, within MARGIN x the error recorded in area_ref.MEASURED — this test is where that error is measured"""
    point, normal, E, vis = R.cases()[name]
    rec = _lib.light_records(R.case_scene(name).to_desc())
    assert rec.shape == (1, 16) and rec[0, 0] == 0
    got, v = R.statement_estimate(rec, point, normal, R.L_LAMP, blocked=R.blocked_by_case_occluder if name == "half-occluded" else None)
    err = float(np.max(np.abs(got.astype(np.float64) - E) / E))
    print(f"{name}: closed form {E}, estimate {got}, relative error {err:.4e} (recorded {R.MEASURED[name]:.4e}), vis {v}")
    assert err <= R.MARGIN * R.MEASURED[name]
    assert abs(float(v) - vis) <= (R.VIS_TOLERANCE if name == "half-occluded" else 0.0)


def test_known_answers_converge():
    """the closed forms are the estimator's limit: at 256 times the samples every case is far inside its tolerance"""
    for name, (point, normal, E, _vis) in R.cases().items():
        rec = _lib.light_records(R.case_scene(name).to_desc())
        got, _v = R.statement_estimate(rec, point, normal, R.L_LAMP, samples=16384, rounds=1,
                                       blocked=R.blocked_by_case_occluder if name == "half-occluded" else None)
        assert float(np.max(np.abs(got.astype(np.float64) - E) / E)) <= 2e-5, name


def test_rays_point_at_their_light():
    """a live ray ends on its light at t = 1: on the rectangle's plane inside its edges, on the sphere's near side"""
    rng = np.random.default_rng(5)
    rec = R.mixed_records(4, rng)
    P = rng.uniform(-1.0, 1.0, (9, 3)).astype(F32)
    N = np.tile(np.array([[0.0, 1.0, 0.0]], F32), (9, 1))
    rays, w = api.area_rays(AreaLight(5, 1e-3).seed(3), rec, P, N)
    assert rays.shape == (9 * 4 * 5, 6) and rays.dtype == F32 and w.shape == (9 * 4 * 5,) and w.dtype == F32
    live = w > 0
    assert live.sum() > 60 and np.all(rays[~live] == 0) and np.all(np.any(rays[live, 3:] != 0, axis=1))
    end = (rays[:, 0:3].astype(np.float64) + rays[:, 3:6]).reshape(9, 4, 5, 3)
    for i in range(4):
        on = live.reshape(9, 4, 5)[:, i]
        e = end[:, i][on]
        if rec[i, 1] == 0:
            c, rad = rec[i, 2:5].astype(np.float64), float(rec[i, 5])
            assert np.allclose(np.linalg.norm(e - c, axis=1), rad, rtol=0, atol=1e-5)
            o = rays[:, 0:3].reshape(9, 4, 5, 3)[:, i][on].astype(np.float64)
            assert np.all(np.einsum("ij,ij->i", e - c, o - c) > 0)                                  # the near side
        else:
            c0 = rec[i, 2:5].astype(np.float64)
            e1, e2 = rec[i, 5:8] - c0, rec[i, 11:14] - c0
            a, b = (e - c0) @ e1 / (e1 @ e1), (e - c0) @ e2 / (e2 @ e2)
            assert np.all((a > -1e-5) & (a < 1 + 1e-5) & (b > -1e-5) & (b < 1 + 1e-5))
            assert np.allclose((e - c0) @ np.cross(e1, e2), 0.0, atol=1e-5)
    # the jitter is per (id, light): ids permute the points, not the draws
    ids = np.array([4, 0, 7], np.uint32)
    r2, w2 = api.area_rays(AreaLight(5, 1e-3).seed(3), rec, P, N, ids=ids)
    assert np.array_equal(r2.reshape(3, 20, 6), rays.reshape(9, 20, 6)[ids]) and np.array_equal(w2.reshape(3, 20), w.reshape(9, 20)[ids])
    # without jitter the shift is (1/2, 1/2) whatever the seed and round
    a = api.area_rays(AreaLight(5, 0.0).seed(1).jitter(False), rec, P, N, round=0)
    b = api.area_rays(AreaLight(5, 0.0).seed(2).jitter(False), rec, P, N, round=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_dead_cases():
    """each gives six zeros and the weight 0: the point inside the sphere, in the rectangle's plane, a back-facing normal, a NaN point,
    a zero normal, a zero-area rectangle — and beside each a live twin, so that the case itself is what kills the entry"""
    sphere = R.sphere_record(0, (0.0, 2.0, 0.0), 0.5)
    rect = R.rect_record(1, (-1.0, 2.0, -1.0), (1.0, 2.0, -1.0), (1.0, 2.0, 1.0), (-1.0, 2.0, 1.0))
    flat = R.rect_record(2, (-1.0, 2.0, -1.0), (1.0, 2.0, -1.0), (1.0, 2.0, -1.0), (-1.0, 2.0, -1.0))      # c3 = c0: no area
    area = AreaLight(3, 0.0).seed(1)
    up, down = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)

    def weights(rec, p, n):
        rays, w = api.area_rays(area, np.array([rec], F32), np.array([p], F32), np.array([n], F32))
        assert np.all(rays[w == 0] == 0) and np.all(np.isfinite(rays)) and np.all(np.isfinite(w))
        return w

    assert np.all(weights(sphere, (0, 0, 0), up) > 0) and np.all(weights(rect, (0, 0, 0), up) > 0)        # the live twins
    assert np.all(weights(sphere, (0.1, 2.0, 0.2), up) == 0)                                                # inside the sphere
    assert np.all(weights(sphere, (0.0, 1.5, 0.0), up) == 0)                                                # on it: d2 > r2 fails
    assert np.all(weights(rect, (0.3, 2.0, 0.2), up) == 0) and np.all(weights(rect, (5.0, 2.0, 0.0), (-1, 0, 0)) == 0)   # in the plane
    assert np.all(weights(sphere, (0, 0, 0), down) == 0) and np.all(weights(rect, (0, 0, 0), down) == 0)   # back-facing
    assert np.all(weights(rect, (NAN, 0, 0), up) == 0) and np.all(weights(sphere, (0, INF, 0), up) == 0)
    assert np.all(weights(rect, (0, 0, 0), (0, NAN, 0)) == 0)
    assert np.all(weights(sphere, (0, 0, 0), (0, 0, 0)) == 0) and np.all(weights(rect, (0, 0, 0), (0, 0, 0)) == 0)
    assert np.all(weights(flat, (0, 0, 0), up) == 0)
    # a rectangle lights both of its sides: from above the lamp, looking down at it
    assert np.all(weights(rect, (0, 4.0, 0), down) > 0)


@pytest.mark.parametrize("Ln, S", [(1, 1), (1, 5), (3, 5), (1, 64), (2, 32), (3, 64), (40, 5)])
def test_area_reduce_keeps_the_statements_order(Ln, S):
    """bit for bit a plain loop over Python floats: G partial sums in ascending m, then the xor butterfly, at M = 1, 5, 15, 64, 192, 200"""
    rng = np.random.default_rng(Ln * 100 + S)
    w, hits, surface, objects = R.synthetic_entries(5, Ln, S, rng)
    hobj = hits.view(np.uint32)[:, 10]
    got, want = api.area_reduce(w, hobj, surface, objects, S), R.reduce_loop(w, hobj, surface, objects, S)
    assert got.shape == (5, 4) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all(got[:, 3] > 0) or Ln * S < 4                                   # (the cases really count something)


def test_area_reduce_by_hand_and_resolve():
    objects = np.array([7, 9], np.uint32)
    surface = np.zeros((4, 16), F32)
    surface[:, 3] = [3, 3, 0, 3]
    surface[:, 12:15] = [[2, 4, 8], [1, 1, 1], [5, 5, 5], [3, 0, 1]]
    w = np.array([0.5, 0.25, 1.0, 2.0], F32)
    hobj = np.array([7, 9, 9, 9], np.uint32)                                     # entry 1 hit light 1 while aimed at light 0; entry 2 is not an emitter
    out = api.area_reduce(w, hobj, surface, objects, 2)
    assert np.array_equal(out[0], [(1.0 / 2) * (2 * 0.5 + 3 * 2.0), (1.0 / 2) * (4 * 0.5 + 0.0), (1.0 / 2) * (8 * 0.5 + 1 * 2.0), 2 / 4])
    sums = np.array([[3.0, 1.0, 0.5, 2.0]], F32)
    assert np.array_equal(api.area_resolve(sums, 3), (sums.astype(np.float64) / 3.0).astype(F32))


def test_area_mask_statement():
    rng = np.random.default_rng(2)
    surface = rng.normal(size=(6, 16)).astype(F32)
    surface[:, 3] = [3, 3, 3, 0, -1, 3]
    hobj = np.array([4, 5, 9, 4, 4, A.FW_NO_HIT], np.uint32)
    out = api.area_mask(hobj, surface, [4, 9])
    want = surface.copy()
    want[[0, 2]] = 0
    want[[0, 2], 3] = -2
    assert out is not surface and np.array_equal(R.u32(out), R.u32(want))


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def _said(lib, st, word):
    """the status and that the detail string names `word`: which check fired"""
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def _area(samples=5, bias=1e-3):
    a = A.fw_area()
    a.samples, a.jitter, a.bias = samples, 1, bias
    return a


def test_scene_area_lights_argument_checks():
    lib = _lib.load()
    n = C.c_uint32(77)
    out = np.full((2, 16), 7.0, F32)
    assert _said(lib, lib.fw_scene_area_lights(None, out.ctypes.data, 2, C.byref(n)), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, lib.fw_scene_area_lights(C.c_void_p(0x1000), out.ctypes.data, 2, None), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, lib.fw_scene_area_lights(C.c_void_p(0x1000), None, 2, C.byref(n)), "null") == A.FW_ERR_BAD_ARG
    assert n.value == 77 and np.all(out == 7.0)


def test_area_rays_argument_checks():
    lib = _lib.load()
    rec = np.array([R.sphere_record(0, (0, 2, 0), 0.5), R.rect_record(3, (-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1))], F32)
    buf = dict(pos=np.full((4, 3), 7.0, F32), nrm=np.full((4, 3), 7.0, F32), rays=np.full((4 * 2 * 5, 6), 7.0, F32), w=np.full(4 * 2 * 5, 7.0, F32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = dict({k: v.ctypes.data for k, v in buf.items()}, lights=rec.ctypes.data)

    def call(a=None, ln=2, n=4, stride=3, device=0, on_device=0, ids_p=None, null=None, **ptrs):
        p = dict(good, **ptrs)
        return lib.fw_area_rays(None if null == "area" else C.byref(a if a is not None else _area()), p["lights"], ln, device, 0, n, p["pos"], p["nrm"],
                                stride, ids_p, p["rays"], p["w"], on_device, None)

    assert _said(lib, call(_area(samples=0), null="area"), "null") == A.FW_ERR_BAD_ARG
    for name in ("lights", "pos", "nrm", "rays", "w"):
        assert _said(lib, call(_area(samples=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name    # NULL before the description
    for word, a in (("samples", _area(samples=0)), ("samples", _area(samples=(1 << 20) + 1)), ("bias", _area(bias=-0.5)), ("bias", _area(bias=NAN)),
                    ("bias", _area(bias=INF))):
        assert _said(lib, call(a, ln=0), word) == A.FW_ERR_BAD_ARG, word                               # the description before the lights
    for ln in (0, A.FW_MAX_LIGHTS + 1):
        assert _said(lib, call(ln=ln, n=0), "n_lights") == A.FW_ERR_BAD_ARG                            # the lights before n
    odd = rec.copy()
    odd[1, 1] = 4.0
    assert _said(lib, call(lights=odd.ctypes.data, n=0), "kind") == A.FW_ERR_BAD_ARG and "lights[1]" in lib.fw_last_error().decode()
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, device=-1), "stride") == A.FW_ERR_BAD_ARG
    for name in ("pos", "nrm", "rays", "w"):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + 2)}), "aligned") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_area(samples=1 << 20), n=1 << 10, on_device=1, w=C.c_void_p(good["w"] + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_area(samples=1 << 20), n=1 << 10), "samples must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(_area(samples=1 << 20), n=1 << 10, device=-1), "samples must be below") == A.FW_ERR_UNSUPPORTED   # the size before the device
    far = np.array([(1 << 30) + 5], np.uint32)
    assert _said(lib, call(n=1, ids_p=far.ctypes.data), "id x n_lights") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_area_reduce_argument_checks():
    lib = _lib.load()
    objects = np.array([0, 3], np.uint32)
    buf = dict(w=np.full(4 * 2 * 5, 7.0, F32), hits=np.full((4 * 2 * 5, 12), 7.0, F32), surface=np.full((4 * 2 * 5, 16), 7.0, F32), sums=np.full((4, 4), 7.0, F32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = dict({k: v.ctypes.data for k, v in buf.items()}, objects=objects.ctypes.data)

    def call(S=5, ln=2, n=4, device=0, on_device=0, ids_p=None, **ptrs):
        p = dict(good, **ptrs)
        return lib.fw_area_reduce(device, S, p["objects"], ln, n, ids_p, p["w"], p["hits"], p["surface"], p["sums"], on_device, None)

    for name in ("objects", "w", "hits", "surface", "sums"):
        assert _said(lib, call(S=0, **{name: None}), "null") == A.FW_ERR_BAD_ARG, name               # NULL before the samples
    for S in (0, (1 << 20) + 1):
        assert _said(lib, call(S=S, ln=0), "samples") == A.FW_ERR_BAD_ARG                             # the samples before the objects
    for ln in (0, A.FW_MAX_LIGHTS + 1):
        assert _said(lib, call(ln=ln, n=0), "n_objects") == A.FW_ERR_BAD_ARG                          # the objects before n
    assert _said(lib, call(n=0, device=-1), "n must") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("hits", 4), ("hits", 8), ("surface", 4), ("surface", 8), ("w", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(S=1 << 20, n=1 << 10), "samples must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(S=1 << 20, n=1 << 10, device=-1), "samples must be below") == A.FW_ERR_UNSUPPORTED     # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_area_mask_argument_checks():
    lib = _lib.load()
    objects = np.array([0, 3, 9], np.uint32)
    buf = dict(hits=np.full((6, 12), 7.0, F32), surface=np.full((6, 16), 7.0, F32))
    good = dict({k: v.ctypes.data for k, v in buf.items()}, objects=objects.ctypes.data)

    def call(ln=3, n=6, device=0, on_device=0, **ptrs):
        p = dict(good, **ptrs)
        return lib.fw_area_mask(device, p["objects"], ln, n, p["hits"], p["surface"], on_device, None)

    for name in ("objects", "hits", "surface"):
        assert _said(lib, call(ln=0, **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for ln in (0, A.FW_MAX_LIGHTS + 1):
        assert _said(lib, call(ln=ln, n=0), "n_objects") == A.FW_ERR_BAD_ARG
    for bad in ([3, 0, 9], [0, 3, 3]):
        o = np.array(bad, np.uint32)
        assert _said(lib, call(objects=o.ctypes.data, n=0), "ascend") == A.FW_ERR_BAD_ARG                # the list before n
    assert _said(lib, call(n=0, device=-1), "n must") == A.FW_ERR_BAD_ARG
    for name, off in (("hits", 4), ("hits", 8), ("surface", 4), ("surface", 8)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(n=1 << 31, device=-1), "below 2^31") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7.0) for v in buf.values())
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_bake_area_argument_checks():
    """fw_bake_gather's pattern and order, all before the scene is looked at: a handle that is never dereferenced will do"""
    lib = _lib.load()
    buf = dict(pos=np.full((4, 3), 7.0, F32), nrm=np.full((4, 3), 7.0, F32), sums=np.full((4, 4), 7.0, F32), out=np.full((4, 4), 7.0, F32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}
    scene = C.c_void_p(0x1000)

    def call(a=None, n=4, stride=3, first=0, rounds=1, on_device=0, null=None, ids_p=None, **ptrs):
        p = dict(good, **ptrs)
        tp = A.fw_trace_params()
        tp.use_bvh, tp.on_device = 1, on_device
        args = dict(scene=scene, area=C.byref(a if a is not None else _area()), tp=C.byref(tp))
        if null:
            args[null] = None
        return lib.fw_bake_area(args["scene"], args["area"], args["tp"], n, p["pos"], p["nrm"], stride, ids_p, first, rounds, p["sums"], p["out"], None)

    for null in ("scene", "area", "tp"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("pos", "nrm"):
        assert _said(lib, call(_area(samples=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for word, a in (("samples", _area(samples=0)), ("samples", _area(samples=(1 << 20) + 1)), ("bias", _area(bias=-0.5)), ("bias", _area(bias=NAN))):
        assert _said(lib, call(a, n=0), word) == A.FW_ERR_BAD_ARG, word                               # the description before n
    assert _said(lib, call(_area(samples=0, bias=-1.0)), "samples") == A.FW_ERR_BAD_ARG and "bias" not in lib.fw_last_error().decode()
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, rounds=0), "stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(rounds=0, first=0xFFFFFFFF), "rounds must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=0xFFFFFFFF, rounds=1, sums=None), "overflows") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(first=2, sums=None, on_device=1, out=C.c_void_p(good["out"] + 4)), "first_round > 0") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("out", 4), ("out", 8), ("pos", 2), ("nrm", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(sums=None, out=None) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert call(_area(samples=1 << 20), n=1 << 11) == A.FW_ERR_NO_DEVICE                          # (the size needs the scene's Ln: after the device)
        assert all(np.all(v == 7.0) for v in buf.values())


def test_gather_flag_bits():
    """FW_GATHER_NO_LIGHTS passes the flag check where bits 2 and 8 are still refused (bit 2 stays unassigned)"""
    lib = _lib.load()
    buf = dict(pos=np.full((4, 3), 7.0, F32), nrm=np.full((4, 3), 7.0, F32), sums=np.full((4, 4), 7.0, F32), out=np.full((4, 4), 7.0, F32),
               sh=np.full((8, 9, 3), 7.0, F32))
    grid = A.fw_probe_grid()
    for k in range(3):
        grid.lo[k], grid.hi[k], grid.counts[k] = 0.0, 1.0, 2
    grid.flags = A.FW_PROBE_WRAP

    def call(flags, directions=5, n=4):
        g = A.fw_gather()
        g.directions, g.jitter, g.bias, g.direct_bias, g.flags = directions, 1, 1e-3, 1e-3, flags
        tp = A.fw_trace_params()
        tp.use_bvh = 1
        return lib.fw_bake_gather(C.c_void_p(0x1000), C.byref(g), C.byref(tp), C.byref(grid), buf["sh"].ctypes.data, None, None, 0.0, None, n,
                                  buf["pos"].ctypes.data, buf["nrm"].ctypes.data, 3, None, 0, 1, buf["sums"].ctypes.data, buf["out"].ctypes.data, None)

    for flags in (2, 8, 2 | A.FW_GATHER_NO_LIGHTS, 8 | A.FW_GATHER_DIRECT, 1 << 31):
        assert _said(lib, call(flags), "gather flags") == A.FW_ERR_BAD_ARG, flags
    # the new bit reaches the check after the flags': the size
    for flags in (A.FW_GATHER_NO_LIGHTS, A.FW_GATHER_NO_LIGHTS | A.FW_GATHER_DIRECT):
        assert _said(lib, call(flags, directions=1 << 20, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED, flags
        if _lib.device_count() == 0:
            assert call(flags) == A.FW_ERR_NO_DEVICE
    assert all(np.all(v == 7.0) for v in buf.values())


def test_python_entry_points_check_and_fail_loudly():
    rng = np.random.default_rng(0)
    w, hits, surface, objects = R.synthetic_entries(2, 2, 3, rng)
    hd = np.zeros(12, _lib.HIT_DTYPE)
    with pytest.raises(ValueError, match="surface"):
        _lib.area_reduce(w[:11], hd[:11], surface[:11], objects, 3, np.zeros((2, 4), F32))
    with pytest.raises(ValueError, match="sums"):
        _lib.area_reduce(w, hd, surface, objects, 3, np.zeros((1, 4), F32))
    with pytest.raises(ValueError, match="weights"):
        _lib.area_reduce(w[:11], hd, surface, objects, 3, np.zeros((2, 4), F32))
    with pytest.raises(ValueError, match="surface"):
        _lib.area_mask(hd, surface.astype(np.float64), objects)
    from firework_amd.api import Renderer
    assert "area" in Renderer.render_probe_lit.__code__.co_varnames and hasattr(Renderer, "render_area")
    if _lib.device_count() == 0:
        with pytest.raises(_lib.FireworkError) as e:
            _lib.area_reduce(w, hd, surface, objects, 3, np.zeros((2, 4), F32))
        assert e.value.status == A.FW_ERR_NO_DEVICE
        with pytest.raises(_lib.FireworkError) as e:
            _lib.area_rays(AreaLight(3), R.mixed_records(2, rng), np.zeros((2, 3), F32), np.ones((2, 3), F32))
        assert e.value.status == A.FW_ERR_NO_DEVICE


# ---- the CLI's refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, word", [
    (["--probe-lit", "p.npz", "--area-light", "16", "-o", "x.png"], "count it twice"),
    (["--area-bias", "0.1", "-o", "x.png"], "needs --area-light"),
    (["--area-light", "0", "-o", "x.png"], "S[,ROUNDS]"), (["--area-light", "x", "-o", "x.png"], "S[,ROUNDS]"),
    (["--area-light", str((1 << 20) + 1), "-o", "x.png"], "S[,ROUNDS]"), (["--area-light", "16,0", "-o", "x.png"], "S[,ROUNDS]"),
    (["--area-light", "16,2,1", "-o", "x.png"], "S[,ROUNDS]"),
    (["--area-light", "16", "--area-bias", "-1", "-o", "x.png"], "--area-bias"), (["--area-light", "16", "--area-bias", "inf", "-o", "x.png"], "--area-bias"),
    (["--area-light", "16", "--ao", "2", "-o", "x.png"], "cannot be combined"), (["--area-light", "16", "--direct-light", "-o", "x.png"], "cannot be combined"),
    (["--area-light", "16", "--denoise", "-o", "x.png"], "cannot be combined"),
    (["--area-light", "16"], "-o FILE.png")])
def test_cli_refusals_come_before_the_device(args, word, capsys):
    """argparse's exit 2 with a message naming the flag; the scene file does not exist, so nothing was loaded, let alone a device asked"""
    from firework_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "none.yml", "-s", "1"] + args)
    assert e.value.code == 2 and word in capsys.readouterr().err, args
