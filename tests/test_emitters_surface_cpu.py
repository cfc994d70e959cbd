"""CPU-side checks of every emitter sampled at surface points (fw_selftest_emitters_records, fw_scene_emitters, fw_emitters_cdf,
fw_emitters_rays, fw_emitters_reduce, fw_bake_emitters and FW_GATHER_NO_EMITTERS): the exports and fw_emitters' layout
at ABI 8; every argument error of the calls in the header's order and the new flag bit beside the refused ones; the records of §9i's
every-kind scene against fw_selftest_emitters, fw_selftest_lights and a float64 restatement; the CDF; the numpy statements — the picks'
stratification, sampled points on their primitives, dead cases beside live twins, closed-form known answers with a measured tolerance
and their convergence, api.emitters_reduce against a plain loop; the CLI's refusals.  fw_scene_emitters needs a resident scene: its
checks are tests/test_gpu_emitters_surface.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import EmitterLights, FinalGather

import area_ref as AR
import emitters_surface_ref as R
from test_all_emitters_cpu import every_kind_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F32 = np.float32
NAMES = ["fw_bake_emitters", "fw_emitters_cdf", "fw_emitters_rays", "fw_emitters_reduce", "fw_scene_emitters", "fw_selftest_emitters_records"]


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.EMITTERS_PROTOTYPES) == NAMES
    for name in NAMES:
        assert hasattr(lib, name), name
        assert len(re.findall(rf"\bint {name}\s*\(", text)) == 1, name


def test_struct_layout_and_round_trip(tmp_path):
    names = ["samples", "jitter", "bias", "chunk_points", "seed"]
    assert [f for f, _ in A.fw_emitters._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("' + "%zu " * (len(names) + 3) + '\\n",sizeof(fw_emitters)' +
           "".join(f",offsetof(fw_emitters,{f})" for f in names) + ",(size_t)FW_GATHER_NO_EMITTERS,(size_t)FW_EMITTERS_RECORD_FLOATS);return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_emitters)] + [getattr(A.fw_emitters, f).offset for f in names] + [A.FW_GATHER_NO_EMITTERS, A.FW_EMITTERS_RECORD_FLOATS]
    assert A.FW_GATHER_NO_EMITTERS == 16 and A.FW_EMITTERS_RECORD_FLOATS == 16
    em = EmitterLights(33, 0.25).seed((7 << 32) | 5).jitter(False)
    em.chunk_points = 9
    a = em.to_abi()
    assert (a.samples, a.jitter, a.bias, a.chunk_points, a.seed) == (33, 0, 0.25, 9, (7 << 32) | 5)
    assert EmitterLights().to_abi().jitter == 1 and EmitterLights().samples == 16 and EmitterLights(bias=0.1).bias == float(F32(0.1))
    assert FinalGather(8, no_emitters=True).to_abi().flags == A.FW_GATHER_NO_EMITTERS
    assert FinalGather(8, direct=True, no_emitters=True).to_abi().flags == A.FW_GATHER_DIRECT | A.FW_GATHER_NO_EMITTERS
    assert FinalGather(8).to_abi().flags == 0 and FinalGather(8, no_lights=True).to_abi().flags == A.FW_GATHER_NO_LIGHTS
    for bad, word in ((EmitterLights(0), "samples"), (EmitterLights((1 << 20) + 1), "samples"), (EmitterLights(4, -1.0), "bias"),
                      (EmitterLights(4, NAN), "bias"), (EmitterLights(4, INF), "bias")):
        with pytest.raises(ValueError, match=word):
            bad.check()
    assert EmitterLights(1 << 20, 0.0).check().samples == 1 << 20


# ---- the records ----------------------------------------------------------------------------------------------------------------------
def test_records_of_the_every_kind_scene():
    """§9i's scene — a rotated mesh shared by two objects, a partial annular disk, a Rect3d, a black emitter, a NaN-channel emitter, an
    emissive cone: fw_selftest_emitters' entries, order and weights; spheres and rectangles fw_selftest_lights' floats; every other
    record a float64 restatement rounded once"""
    scene = every_kind_scene()
    desc = scene.to_desc()
    rec, codes = _lib.emitters_records(desc)
    st = _lib.selftest_emitters(desc)
    assert rec.shape == (st["obj"].size, 16) and rec.dtype == F32 and codes.shape == (st["obj"].size, 2) and codes.dtype == np.uint32
    assert np.array_equal(rec[:, 0], st["obj"]) and np.array_equal(rec[:, 1], st["kind"])
    assert np.array_equal(codes[:, 0], st["obj"]) and np.array_equal(codes[:, 1], st["prim"])
    assert np.array_equal(rec[:, 14].astype(np.float64), st["area"]) and np.array_equal(rec[:, 15].astype(np.float64), st["weight"])
    lights = _lib.light_records(desc)
    seen = 0
    for l in lights:
        at = np.nonzero(rec[:, 0] == l[0])[0]
        if at.size:                                                                          # (the black sphere is a light but has no entry)
            assert at.size == 1 and np.array_equal(AR.u32(rec[at[0], :14]), AR.u32(l[:14]))
            seen += 1
    assert seen == 3 and lights.shape[0] == 4
    want, wcodes = R.records_ref(scene)
    other = ~np.isin(rec[:, 1], [0, 1, 2, 3])
    assert other.sum() == 6 + 1 + 36 and np.array_equal(codes, wcodes)
    assert np.array_equal(AR.u32(rec[other, 2:14]), AR.u32(want[other, 2:14]))
    # the rotated mesh's vertices moved, the unrotated one's only shifted
    mesh = scene.render_objects[7].obj
    tri0 = mesh.verts[mesh.indicies[:3]].astype(np.float64) + (3.0, 5.0, -1.0)
    assert np.array_equal(rec[np.nonzero(rec[:, 0] == 7)[0][0], 2:11], tri0.astype(F32).reshape(-1))
    # caps: the first records only, and the count still
    lib = _lib.load()
    n = C.c_uint32()
    part, pc = np.full((9, 16), 7.0, F32), np.full((9, 2), 7, np.uint32)
    assert lib.fw_selftest_emitters_records(desc.ptr(), part.ctypes.data, pc.ctypes.data, 5, C.byref(n)) == 0
    assert n.value == rec.shape[0] and np.array_equal(AR.u32(part[:5]), AR.u32(rec[:5])) and np.all(part[5:] == 7.0) and np.all(pc[5:] == 7)
    for args in ((None, part.ctypes.data, pc.ctypes.data, 5, C.byref(n)), (desc.ptr(), None, pc.ctypes.data, 5, C.byref(n)),
                 (desc.ptr(), part.ctypes.data, None, 5, C.byref(n)), (desc.ptr(), part.ctypes.data, pc.ctypes.data, 5, None)):
        assert lib.fw_selftest_emitters_records(*args) == A.FW_ERR_BAD_ARG
    for args in ((None, part.ctypes.data, pc.ctypes.data, 5, C.byref(n)), (C.c_void_p(0x1000), None, pc.ctypes.data, 5, C.byref(n)),
                 (C.c_void_p(0x1000), part.ctypes.data, pc.ctypes.data, 5, None)):
        assert lib.fw_scene_emitters(*args) == A.FW_ERR_BAD_ARG


# ---- the CDF --------------------------------------------------------------------------------------------------------------------------
def test_cdf():
    rng = np.random.default_rng(3)
    for w in (rng.uniform(0.0, 5.0, 1000).astype(F32), np.array([0, 0, 2.5, NAN, -1, 0.5, INF, 3, 0, -0.0], F32), np.array([1e-30], F32),
              np.array([3e38, 3e38, 3e38], F32)):
        got, total = _lib.emitters_cdf(w)
        want, wt = api.emitters_cdf(w)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)) and total == wt > 0
        ok = np.isfinite(w) & (w > 0)
        last = np.nonzero(ok)[0][-1]
        assert got[last] == 1.0 and np.all(got[last:] == 1.0) and np.all(np.diff(got) >= 0) and got[0] >= 0
        # zero, negative and non-finite weights at the start, in the middle and at the end are never picked
        xi = np.concatenate([rng.uniform(0, 1, 4000), [0.0, 1.0 - 2.0 ** -53], got[:-1][got[:-1] < 1.0]])
        picks = np.searchsorted(got, xi, side="right")
        assert picks.max() <= last and np.all(ok[picks])
        flat = np.concatenate([[0.0], got])
        assert np.all((np.diff(flat) > 0) == ok)
    for w in (np.zeros(5, F32), np.array([-1, NAN, 0], F32)):
        got, total = _lib.emitters_cdf(w)
        assert total == 0.0 == api.emitters_cdf(w)[1] and np.all(got == 0) and np.all(api.emitters_cdf(w)[0] == 0)
    lib = _lib.load()
    w, c = np.ones(3, F32), np.zeros(3)
    assert lib.fw_emitters_cdf(None, 3, c.ctypes.data, None) == A.FW_ERR_BAD_ARG and lib.fw_emitters_cdf(w.ctypes.data, 3, None, None) == A.FW_ERR_BAD_ARG
    assert lib.fw_emitters_cdf(w.ctypes.data, 0, c.ctypes.data, None) == A.FW_ERR_BAD_ARG and lib.fw_emitters_cdf(w.ctypes.data, 3, c.ctypes.data, None) == 0


# ---- the numpy statement --------------------------------------------------------------------------------------------------------------
def _statement(n_entries, S, n_points=7, seed=3, jitter=True, round=0, bias=1e-3):
    rng = np.random.default_rng(100 * n_entries + S)
    rec, codes = R.mixed_records(n_entries, rng)
    cdf, _t = api.emitters_cdf(rec[:, 15])
    P = rng.uniform(-1.0, 1.0, (n_points, 3)).astype(F32)
    N = np.tile(np.array([[0.0, 1.0, 0.0]], F32), (n_points, 1))
    em = EmitterLights(S, bias).seed(seed).jitter(jitter)
    return rec, codes, cdf, P, N, em, api.emitters_rays(em, rec, cdf, P, N, round=round)


@pytest.mark.parametrize("n_entries, S", [(1, 16), (3, 16), (5, 64), (12, 200), (40, 7)])
def test_picks_are_stratified(n_entries, S):
    """the S samples of a point partition in proportion to p within +-1 per entry, whatever the jitter: the CDF keeps the strata"""
    rec, _codes, cdf, P, N, em, _out = _statement(n_entries, S, bias=0.0)
    p = np.diff(np.concatenate([[0.0], cdf]))
    for r in (0, 3):
        # (count the picks before liveness: a dead sample still occupied its stratum)
        xj = api.texel_jitter(em._seed, r, np.arange(P.shape[0]))
        a1 = (np.arange(S)[None, :] + xj[:, 0:1]) / float(S)
        xi = a1 - np.floor(a1)
        picks = np.searchsorted(cdf, xi, side="right")
        for q in range(P.shape[0]):
            count = np.bincount(picks[q], minlength=n_entries)
            assert np.all(np.abs(count - S * p) <= 1.0 + 1e-9), (q, count, S * p)
            assert np.all(count[rec[:, 15] == 0] == 0)
        _rays, w, live_picks = api.emitters_rays(em, rec, cdf, P, N, round=r)
        live = w > 0
        assert np.array_equal(live_picks[live], picks.reshape(-1)[live]) and np.all(live_picks[~live] == R.DEAD)


def test_sampled_points_lie_on_their_primitive():
    """a live ray ends on its entry at t = 1: inside the triangle, inside the sector, in the face's plane and inside its edges, on the
    sphere's near side; ids permute points, not draws; without jitter seed and round do not matter"""
    rec, _codes, cdf, P, N, em, (rays, w, picks) = _statement(10, 50, n_points=9)
    assert rays.shape == (9 * 50, 6) and rays.dtype == F32 and w.shape == (450,) and w.dtype == F32 and picks.dtype == np.uint32
    live = w > 0
    assert live.sum() > 150 and np.all(rays[~live] == 0) and np.all(picks[~live] == R.DEAD) and np.all(np.any(rays[live, 3:] != 0, axis=1))
    end = rays[:, 0:3].astype(np.float64) + rays[:, 3:6]
    kinds = set()
    for e in np.nonzero(live)[0]:
        r = rec[picks[e]].astype(np.float64)
        g, x = r[2:14], end[e]
        kinds.add(int(r[1]))
        if r[1] == 0:
            assert abs(np.linalg.norm(x - g[0:3]) - g[3]) < 1e-5 and (x - g[0:3]) @ (rays[e, 0:3] - g[0:3]) > 0
        elif r[1] == 5:
            e1, e2 = g[3:6] - g[0:3], g[6:9] - g[0:3]
            M = np.stack([e1, e2], 1)
            (b1, b2), *_ = np.linalg.lstsq(M, x - g[0:3], rcond=None)
            assert b1 > -1e-5 and b2 > -1e-5 and b1 + b2 < 1 + 1e-5 and np.linalg.norm(M @ [b1, b2] - (x - g[0:3])) < 1e-5
        elif r[1] == 9:
            d = x - g[0:3]
            a, b = d @ g[3:6], d @ g[6:9]
            rad, phi = np.hypot(a, b), np.arctan2(b, a) % (2 * np.pi)
            assert abs(d @ np.cross(g[3:6], g[6:9])) < 1e-5 and g[10] - 1e-5 < rad < g[9] + 1e-5 and phi < g[11] + 1e-5
        else:
            e1, e2 = g[3:6] - g[0:3], g[9:12] - g[0:3]
            a, b = (x - g[0:3]) @ e1 / (e1 @ e1), (x - g[0:3]) @ e2 / (e2 @ e2)
            assert -1e-5 < a < 1 + 1e-5 and -1e-5 < b < 1 + 1e-5 and abs((x - g[0:3]) @ np.cross(e1, e2)) < 1e-5
    assert kinds == {0, 1, 2, 3, 4, 5, 9} or kinds >= {0, 4, 5, 9}
    ids = np.array([4, 0, 7], np.uint32)
    r2, w2, p2 = api.emitters_rays(em, rec, cdf, P, N, ids=ids)
    assert np.array_equal(r2.reshape(3, 50, 6), rays.reshape(9, 50, 6)[ids]) and np.array_equal(w2.reshape(3, 50), w.reshape(9, 50)[ids])
    assert np.array_equal(p2.reshape(3, 50), picks.reshape(9, 50)[ids])
    a = api.emitters_rays(EmitterLights(5, 0.0).seed(1).jitter(False), rec, cdf, P, N, round=0)
    b = api.emitters_rays(EmitterLights(5, 0.0).seed(2).jitter(False), rec, cdf, P, N, round=3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_one_entry_is_the_area_lattice():
    """with a single sphere or rectangle the statement is api.area_rays at Ln = 1, bit for bit"""
    rng = np.random.default_rng(8)
    P = rng.uniform(-1.0, 1.0, (11, 3)).astype(F32)
    N = rng.normal(size=(11, 3)).astype(F32) + (0, 2, 0)
    for rec in (R.sphere_record(4, (0.2, 2.0, -0.1), 0.5, power=3.0), R.rect_record(2, (-1, 2, -1), (1, 2.2, -1), (1, 2.2, 1), (-1, 2, 1), power=0.2)):
        for S, r in ((1, 0), (5, 0), (64, 3)):
            rays, w, picks = api.emitters_rays(EmitterLights(S, 1e-3).seed(9), [rec], [1.0], P, N.astype(F32), round=r)
            ar, aw = api.area_rays(api.AreaLight(S, 1e-3).seed(9), [rec], P, N.astype(F32), round=r)
            assert np.array_equal(AR.u32(rays), AR.u32(ar)) and np.array_equal(AR.u32(w), AR.u32(aw)) and (w > 0).sum() > 0
            assert np.all(picks[w > 0] == 0)


def test_dead_cases():
    """each gives six zeros, the weight 0 and the pick 0xffffffff, beside a live twin: §9zb's list, a triangle and a sector without area"""
    up, down = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)
    sphere = R.sphere_record(0, (0.0, 2.0, 0.0), 0.5)
    rect = R.rect_record(1, (-1.0, 2.0, -1.0), (1.0, 2.0, -1.0), (1.0, 2.0, 1.0), (-1.0, 2.0, 1.0), A.FW_SHAPE_RECT3D)
    tri = R.tri_record(2, (-1.0, 2.0, -1.0), (1.0, 2.0, -1.0), (0.0, 2.0, 1.0))
    disk = R.disk_record(3, (0.0, 2.0, 0.0), (1, 0, 0), (0, 0, 1), 0.8, 0.2, 4.0)
    thin = R.tri_record(2, (-1.0, 2.0, -1.0), (1.0, 2.0, -1.0), (3.0, 2.0, -1.0))            # collinear: no area
    shut = R.disk_record(3, (0.0, 2.0, 0.0), (1, 0, 0), (0, 0, 1), 0.8, 0.2, 0.0)            # phi_max 0: no area
    ring0 = R.disk_record(3, (0.0, 2.0, 0.0), (1, 0, 0), (0, 0, 1), 0.8, 0.8, 4.0)           # r_in = r: no area
    em = EmitterLights(3, 0.0).seed(1)

    def weights(rec, p, n):
        rec = np.array(rec, F32)
        rec[15] = 1.0                                                                        # (picked all the same: the geometry is what kills it)
        rays, w, picks = api.emitters_rays(em, [rec], [1.0], np.array([p], F32), np.array([n], F32))
        assert np.all(rays[w == 0] == 0) and np.all(picks[w == 0] == R.DEAD) and np.all(picks[w > 0] == 0)
        assert np.all(np.isfinite(rays)) and np.all(np.isfinite(w))
        return w

    for live in (sphere, rect, tri, disk):
        assert np.all(weights(live, (0, 0, 0), up) > 0)
        assert np.all(weights(live, (0, 0, 0), down) == 0)                                   # back-facing
        assert np.all(weights(live, (NAN, 0, 0), up) == 0) and np.all(weights(live, (0, INF, 0), up) == 0)
        assert np.all(weights(live, (0, 0, 0), (0, NAN, 0)) == 0) and np.all(weights(live, (0, 0, 0), (0, 0, 0)) == 0)
    assert np.all(weights(sphere, (0.1, 2.0, 0.2), up) == 0) and np.all(weights(sphere, (0.0, 1.5, 0.0), up) == 0)     # inside it, on it
    for flat in (rect, tri, disk):
        assert np.all(weights(flat, (5.0, 2.0, 0.0), (-1, 0, 0)) == 0)                       # in the plane
        assert np.all(weights(flat, (0, 4.0, 0), down) > 0)                                  # both sides emit
    for dead in (thin, shut, ring0):
        assert np.all(weights(dead, (0, 0, 0), up) == 0)


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_known_answers(name):
    """every sample that faces the receiver visible and the emission constant: the estimate at the tests' S and rounds against the closed
    form, within MARGIN x the error recorded in emitters_surface_ref.MEASURED — this test is where that error is measured"""
    point, normal, E = R.cases()[name]
    got, v = R.statement_estimate(R.case_scene(name), point, normal)
    err = float(np.max(np.abs(got.astype(np.float64) - E) / E))
    print(f"{name}: closed form {E}, estimate {got}, relative error {err:.4e} (recorded {R.MEASURED[name]:.4e}), vis {v}")
    assert err <= R.MARGIN * R.MEASURED[name]
    assert (v == 1.0) == (name not in ("face", "five"))                                      # (a box's far faces are sampled and hidden)


def test_known_answers_converge():
    """the closed forms are the estimator's limit: at S = 16 384 every case is within MARGIN x what was recorded there"""
    for name, (point, normal, E) in R.cases().items():
        got, _v = R.statement_estimate(R.case_scene(name), point, normal, samples=16384, rounds=1)
        err = float(np.max(np.abs(got.astype(np.float64) - E) / E))
        print(f"{name}: S = 16384: relative error {err:.4e} (recorded {R.CONVERGED[name]:.4e})")
        assert err <= R.MARGIN * R.CONVERGED[name] and R.CONVERGED[name] < 1e-4, name


# ---- the reduction --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5, 15, 64, 200])
def test_reduce_keeps_the_statements_order(S):
    rng = np.random.default_rng(S)
    picks, w, hits, surface, codes = R.synthetic_entries(5, S, rng)
    ho, hp = hits.view(np.uint32)[:, 10], hits.view(np.uint32)[:, 11]
    got, want = api.emitters_reduce(picks, w, ho, hp, surface, codes, S), R.reduce_loop(picks, w, ho, hp, surface, codes, S)
    assert got.shape == (5, 4) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all(got[:, 3] > 0) or S < 5


def test_reduce_by_hand():
    codes = np.array([[7, 0], [9, 4], [9, 5]], np.uint32)
    surface = np.zeros((6, 16), F32)
    surface[:, 3] = [3, 3, 3, 0, 3, 3]
    surface[:, 12:15] = [[2, 4, 8], [1, 1, 1], [5, 5, 5], [3, 0, 1], [7, 7, 7], [1, 2, 3]]
    w = np.array([0.5, 0.25, 1.0, 2.0, 0.0, 4.0], F32)
    picks = np.array([0, 1, 1, 2, R.DEAD, 2], np.uint32)
    ho = np.array([7, 9, 8, 9, 7, A.FW_NO_HIT], np.uint32)      # visible; right object, wrong prim; another object; not an emitter; dead; a miss
    hp = np.array([0, 5, 4, 5, 0, 0], np.uint32)
    out = api.emitters_reduce(picks, w, ho, hp, surface, codes, 6)
    assert np.array_equal(out[0], [(1.0 / 6) * (2 * 0.5), (1.0 / 6) * (4 * 0.5), (1.0 / 6) * (8 * 0.5), (1.0 / 6) * 1.0])
    hp[1] = 4                                                    # ... and with the right prim the second entry counts
    out = api.emitters_reduce(picks, w, ho, hp, surface, codes, 6)
    assert np.array_equal(out[0], [(1.0 / 6) * (2 * 0.5 + 1 * 0.25), (1.0 / 6) * (4 * 0.5 + 0.25), (1.0 / 6) * (8 * 0.5 + 0.25), (1.0 / 6) * 2.0])
    assert api.emitters_resolve is api.area_resolve


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def _said(lib, st, word):
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def _em(samples=5, bias=1e-3):
    a = A.fw_emitters()
    a.samples, a.jitter, a.bias = samples, 1, bias
    return a


def test_emitters_rays_argument_checks():
    lib = _lib.load()
    rec = np.array([R.sphere_record(0, (0, 2, 0), 0.5), R.tri_record(3, (-1, 2, -1), (1, 2, -1), (1, 2, 1))], F32)
    cdf = np.array([0.25, 1.0])
    buf = dict(pos=np.full((4, 3), 7.0, F32), nrm=np.full((4, 3), 7.0, F32), rays=np.full((4 * 5, 6), 7.0, F32), w=np.full(4 * 5, 7.0, F32),
               picks=np.full(4 * 5, 7, np.uint32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = dict({k: v.ctypes.data for k, v in buf.items()}, rec=rec.ctypes.data, cdf=cdf.ctypes.data)

    def call(a=None, ne=2, n=4, stride=3, device=0, on_device=0, ids_p=None, null=None, **ptrs):
        p = dict(good, **ptrs)
        return lib.fw_emitters_rays(None if null == "em" else C.byref(a if a is not None else _em()), p["rec"], p["cdf"], ne, device, 0, n, p["pos"],
                                    p["nrm"], stride, ids_p, p["rays"], p["w"], p["picks"], on_device, None)

    assert _said(lib, call(_em(samples=0), null="em"), "null") == A.FW_ERR_BAD_ARG
    for name in ("rec", "cdf", "pos", "nrm", "rays", "w", "picks"):
        assert _said(lib, call(_em(samples=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name    # NULL before the description
    for word, a in (("samples", _em(samples=0)), ("samples", _em(samples=(1 << 20) + 1)), ("bias", _em(bias=-0.5)), ("bias", _em(bias=NAN)),
                    ("bias", _em(bias=INF))):
        assert _said(lib, call(a, ne=0), word) == A.FW_ERR_BAD_ARG, word                             # the description before the list
    for ne in (0, (1 << 24) + 1):
        assert _said(lib, call(ne=ne, n=0), "n_entries") == A.FW_ERR_BAD_ARG                         # the list before n
    odd = rec.copy()
    odd[1, 1] = 7.0                                                                                  # a cone is never an entry
    assert _said(lib, call(rec=odd.ctypes.data, n=0), "kind") == A.FW_ERR_BAD_ARG and "records[1]" in lib.fw_last_error().decode()
    for bad, word in (([0.5, 0.25], "decrease"), ([0.5, 1.5], "[0, 1]"), ([-0.1, 1.0], "[0, 1]"), ([NAN, 1.0], "decrease"), ([0.25, 0.75], "end in 1"),
                      ([0.0, 0.0], "end in 1")):
        c = np.array(bad)
        assert _said(lib, call(cdf=c.ctypes.data, n=0), word) == A.FW_ERR_BAD_ARG, bad
    assert _said(lib, call(n=0, stride=2), "n must") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(stride=2, device=-1), "stride") == A.FW_ERR_BAD_ARG
    for name in ("pos", "nrm", "rays", "w", "picks"):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + 2)}), "aligned") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_em(samples=1 << 20), n=1 << 11), "samples must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(_em(samples=1 << 20), n=1 << 11, device=-1), "samples must be below") == A.FW_ERR_UNSUPPORTED   # the size before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7) for v in buf.values())
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_emitters_reduce_argument_checks():
    lib = _lib.load()
    codes = np.array([[0, 0], [3, 2]], np.uint32)
    buf = dict(picks=np.full(4 * 5, 7, np.uint32), w=np.full(4 * 5, 7.0, F32), hits=np.full((4 * 5, 12), 7.0, F32), surface=np.full((4 * 5, 16), 7.0, F32),
               sums=np.full((4, 4), 7.0, F32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = dict({k: v.ctypes.data for k, v in buf.items()}, codes=codes.ctypes.data)

    def call(S=5, ne=2, n=4, device=0, on_device=0, ids_p=None, **ptrs):
        p = dict(good, **ptrs)
        return lib.fw_emitters_reduce(device, S, p["codes"], ne, n, ids_p, p["picks"], p["w"], p["hits"], p["surface"], p["sums"], on_device, None)

    for name in ("codes", "picks", "w", "hits", "surface", "sums"):
        assert _said(lib, call(S=0, **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for S in (0, (1 << 20) + 1):
        assert _said(lib, call(S=S, ne=0), "samples") == A.FW_ERR_BAD_ARG
    for ne in (0, (1 << 24) + 1):
        assert _said(lib, call(ne=ne, n=0), "n_entries") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n=0, device=-1), "n must") == A.FW_ERR_BAD_ARG
    for name, off in (("sums", 4), ("sums", 8), ("hits", 4), ("hits", 8), ("surface", 4), ("surface", 8), ("w", 2), ("picks", 2)):
        assert _said(lib, call(on_device=1, **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, (name, off)
    assert _said(lib, call(on_device=1, ids_p=C.c_void_p(ids.ctypes.data + 2)), "aligned") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(S=1 << 20, n=1 << 11), "samples must be below") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(S=1 << 20, n=1 << 11, device=-1), "samples must be below") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE and call(ids_p=ids.ctypes.data) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7) for v in buf.values())
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG


def test_bake_emitters_argument_checks():
    """fw_bake_area's pattern and order, all before the scene is looked at: a handle that is never dereferenced will do"""
    lib = _lib.load()
    buf = dict(pos=np.full((4, 3), 7.0, F32), nrm=np.full((4, 3), 7.0, F32), sums=np.full((4, 4), 7.0, F32), out=np.full((4, 4), 7.0, F32))
    ids = np.array([2, 0, 3, 1], np.uint32)
    good = {k: v.ctypes.data for k, v in buf.items()}
    scene = C.c_void_p(0x1000)

    def call(a=None, n=4, stride=3, first=0, rounds=1, on_device=0, null=None, ids_p=None, **ptrs):
        p = dict(good, **ptrs)
        tp = A.fw_trace_params()
        tp.use_bvh, tp.on_device = 1, on_device
        args = dict(scene=scene, em=C.byref(a if a is not None else _em()), tp=C.byref(tp))
        if null:
            args[null] = None
        return lib.fw_bake_emitters(args["scene"], args["em"], args["tp"], n, p["pos"], p["nrm"], stride, ids_p, first, rounds, p["sums"], p["out"], None)

    for null in ("scene", "em", "tp"):
        assert _said(lib, call(null=null), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("pos", "nrm"):
        assert _said(lib, call(_em(samples=0), **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for word, a in (("samples", _em(samples=0)), ("samples", _em(samples=(1 << 20) + 1)), ("bias", _em(bias=-0.5)), ("bias", _em(bias=NAN))):
        assert _said(lib, call(a, n=0), word) == A.FW_ERR_BAD_ARG, word
    assert _said(lib, call(_em(samples=0, bias=-1.0)), "samples") == A.FW_ERR_BAD_ARG and "bias" not in lib.fw_last_error().decode()
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
        assert call(_em(samples=1 << 20), n=1 << 11) == A.FW_ERR_NO_DEVICE                            # (the size check comes after the device's)
        assert all(np.all(v == 7.0) for v in buf.values())


def test_gather_flag_bits():
    """FW_GATHER_NO_EMITTERS passes the flag check; bits 2 and 8, both complements together and bit 31 are refused"""
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

    for flags in (2, 8, 4 | 16, 4 | 16 | 1, 2 | 16, 1 << 31):
        assert _said(lib, call(flags), "gather flags") == A.FW_ERR_BAD_ARG, flags
    for flags in (16, 16 | A.FW_GATHER_DIRECT):
        assert _said(lib, call(flags, directions=1 << 20, n=1 << 11), "directions must be below") == A.FW_ERR_UNSUPPORTED, flags
        if _lib.device_count() == 0:
            assert call(flags) == A.FW_ERR_NO_DEVICE
    assert all(np.all(v == 7.0) for v in buf.values())


def test_python_entry_points_check_and_fail_loudly():
    rng = np.random.default_rng(0)
    picks, w, hits, surface, codes = R.synthetic_entries(2, 3, rng)
    hd = np.zeros(6, _lib.HIT_DTYPE)
    with pytest.raises(ValueError, match="surface"):
        _lib.emitters_reduce(picks[:5], w[:5], hd[:5], surface[:5], codes, 3, np.zeros((2, 4), F32))
    with pytest.raises(ValueError, match="sums"):
        _lib.emitters_reduce(picks, w, hd, surface, codes, 3, np.zeros((1, 4), F32))
    with pytest.raises(ValueError, match="weights"):
        _lib.emitters_reduce(picks, w[:5], hd, surface, codes, 3, np.zeros((2, 4), F32))
    with pytest.raises(ValueError, match="cdf"):
        _lib.emitters_rays(EmitterLights(3), np.zeros((2, 16), F32), [1.0], np.zeros((2, 3), F32), np.ones((2, 3), F32))
    from firework_amd.api import Renderer
    names = Renderer.render_probe_lit.__code__.co_varnames
    assert "emitters" in names and "emitters_rounds" in names and hasattr(Renderer, "render_emitters")
    assert hasattr(_lib.DeviceScene, "emitters") and hasattr(_lib.DeviceScene, "bake_emitters")
    if _lib.device_count() == 0:
        rec, _c = R.mixed_records(2, rng)
        with pytest.raises(_lib.FireworkError) as e:
            _lib.emitters_reduce(picks, w, hd, surface, codes, 3, np.zeros((2, 4), F32))
        assert e.value.status == A.FW_ERR_NO_DEVICE
        with pytest.raises(_lib.FireworkError) as e:
            _lib.emitters_rays(EmitterLights(3), rec, api.emitters_cdf(rec[:, 15])[0], np.zeros((2, 3), F32), np.ones((2, 3), F32))
        assert e.value.status == A.FW_ERR_NO_DEVICE


# ---- the CLI's refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, word", [
    (["--probe-lit", "p.npz", "--emitter-light", "16", "-o", "x.png"], "count it twice"),
    (["--emitter-bias", "0.1", "-o", "x.png"], "needs --emitter-light"),
    (["--emitter-light", "16", "--area-light", "16", "-o", "x.png"], "sampled twice"),
    (["--emitter-light", "0", "-o", "x.png"], "S[,ROUNDS]"), (["--emitter-light", "x", "-o", "x.png"], "S[,ROUNDS]"),
    (["--emitter-light", str((1 << 20) + 1), "-o", "x.png"], "S[,ROUNDS]"), (["--emitter-light", "16,0", "-o", "x.png"], "S[,ROUNDS]"),
    (["--emitter-light", "16,2,1", "-o", "x.png"], "S[,ROUNDS]"),
    (["--emitter-light", "16", "--emitter-bias", "-1", "-o", "x.png"], "--emitter-bias"),
    (["--emitter-light", "16", "--emitter-bias", "inf", "-o", "x.png"], "--emitter-bias"),
    (["--emitter-light", "16", "--ao", "2", "-o", "x.png"], "cannot be combined"),
    (["--emitter-light", "16", "--direct-light", "-o", "x.png"], "cannot be combined"),
    (["--emitter-light", "16", "--denoise", "-o", "x.png"], "cannot be combined"),
    (["--emitter-light", "16"], "-o FILE.png")])
def test_cli_refusals_come_before_the_device(args, word, capsys):
    from firework_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "none.yml", "-s", "1"] + args)
    assert e.value.code == 2 and word in capsys.readouterr().err, args
