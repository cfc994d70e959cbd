"""Vacuity guards for the coordinate / scale family (tests/coord_scenes.py), oracle only: the GPU parity tests of
tests/test_gpu_coordinates.py prove something only if the family reaches the regime it targets — far origins relative to the
triangles, rays that take the fast walks rather than the exact one, rays that straddle the decisions at edges and box corners."""
import numpy as np
import pytest

import coord_scenes as C

FAMILY = C.family()
IDS = [f[0] for f in FAMILY]
FAST = [f for f in FAMILY if f[0][0] in "abc" or f[0] == "spread_mesh"]


def _desc_bytes(sc):
    d = sc.to_desc()
    return d.content_hash()


@pytest.mark.parametrize("sid", ["a_o3e4", "b_o1e4_rot", "c_far", "d_R2_2^-10", "d_C3_2^12"])
def test_generators_are_deterministic(oracle, sid):
    fn = dict((f[0], f[1]) for f in FAMILY)[sid]
    (s1, r1), (s2, r2) = fn(), fn()
    assert _desc_bytes(s1) == _desc_bytes(s2)
    assert r1.settings == r2.settings
    g1, u1 = C.grazing_set(s1, r1, oracle)
    g2, u2 = C.grazing_set(s2, r2, oracle)
    assert g1.tobytes() == g2.tobytes() and u1.tobytes() == u2.tobytes()


@pytest.mark.parametrize("base", C.BASES)
def test_rescalings_are_exact(base):
    """every length of the description is the base scene's times exactly 2^k, densities divided by it, everything else unchanged"""
    ref = C.geometric_floats(*C.base_scene(base))
    for k in C.SCALES:
        got = C.geometric_floats(*C.rescaled(base, k))
        assert [g[0] for g in got] == [r[0] for r in ref]
        f = 2.0 ** k
        for (kind, a), (_, b) in zip(got, ref):
            a32, b32 = a.astype(np.float32), b.astype(np.float32)
            assert np.array_equal(a32, a) or kind == "X"
            want = {"L": b32 * np.float32(f), "D": b32 / np.float32(f), "X": b}[kind]
            assert np.array_equal(a if kind == "X" else a32, want), (base, k, kind)
        assert any(kind == "L" and np.any(a != 0) for kind, a in got)


@pytest.mark.parametrize("sid,fn,modes", FAMILY, ids=IDS)
def test_camera_rays_hit(oracle, sid, fn, modes):
    sc, r = fn()
    rays = C.camera_ray_set(r, oracle)
    for m in modes:
        rate = float(oracle.trace(sc, rays, m)[:, 0].mean())
        assert rate >= 0.3, (sid, m, rate)


def split_pairs(ora, ulps):
    """per (+n, -n) pair of a grazing set: did the nudge across the edge change the decision — hit against miss, another material,
    or another surface (a normal that turns by more than 1e-3: the patch's triangles are flat-shaded)?"""
    a, b = ora[0::2], ora[1::2]
    assert (ulps[0::2] == -ulps[1::2]).all()
    turn = np.abs(np.nan_to_num(a[:, 5:8]) - np.nan_to_num(b[:, 5:8])).max(axis=1) > 1e-3
    return (a[:, 0] != b[:, 0]) | (a[:, 8] != b[:, 8]) | turn


@pytest.mark.parametrize("sid,fn,modes", FAMILY, ids=IDS)
def test_grazing_rays_straddle_the_decisions(oracle, sid, fn, modes):
    """the oracle's decision changes inside some of the +-n ulp pairs: the rays do sit on edges and corners"""
    sc, r = fn()
    rays, ulps = C.grazing_set(sc, r, oracle)
    assert rays.shape[0] >= 8
    for m in modes:
        ora = oracle.trace(sc, rays, m)
        hit = ora[:, 0] == 1
        split = split_pairs(ora, ulps)
        near = np.abs(ulps[0::2]) <= 4
        print(f"{sid} use_bvh={m}: hits {int(hit.sum())}/{hit.size}, pairs split {int(split.sum())}/{split.size}, "
              f"within 4 ulps {int(split[near].sum())}")
        assert hit.any() and split[near].any(), (sid, m, float(hit.mean()))


@pytest.mark.parametrize("sid,fn,modes", FAST, ids=[f[0] for f in FAST])
def test_fast_walk_regime(oracle, sid, fn, modes):
    """(a)-(c): the rays start within far_r of far_c (fw_runtime.cpp, DExact) — not on the exact list by the far rule — and the
    meshes' rays are below the shear threshold 2^10 (EXACT_SHEAR_LOG2)"""
    sc, r = fn()
    rays = C.camera_ray_set(r, oracle)
    graze, _ = C.grazing_set(sc, r, oracle)
    far_c, far_r = C.far_rule(oracle, sc)
    for what, x in (("camera", rays), ("grazing", graze)):
        near = np.abs(x[:, :3].astype(np.float64) - far_c).max(axis=1) <= far_r
        assert near.mean() >= 0.9, (sid, what, float(near.mean()), far_c, far_r)
        if sid.startswith("a_") or sid == "spread_mesh":
            assert (C.shear(x[:, 3:]) < 2.0 ** 10).mean() >= 0.9, (sid, what)


def test_far_rule_restatement_matches_the_cluster():
    """the numpy far rule on the far cluster: the smallest item is a sphere (disks count by their enclosing box), far_r = 256 x it"""
    from oracle import oracle_binding as ob
    sc, _ = C.far_cluster("c_far")
    _, far_r = C.far_rule(ob, sc)
    assert 12.0 < far_r < 80.0


def test_far_offsets_reach_the_regime():
    """|O| / typical triangle reaches 2^18 and beyond (where 2^-24 |O| passes the walked boxes' growth of 2^-6 of a triangle)"""
    ratios = [C.mesh_ratio(off, h) for _, off, h in C.MESH_CASES]
    assert max(ratios) >= 2.0 ** 18 and min(r for r in ratios if r > 0) <= 2.0 ** 10
    print("largest |O| / triangle: 2^%.2f" % np.log2(max(ratios)))


def test_spread_mesh_reaches_the_mesh_from_far_unflagged(oracle):
    """the far-origin rays of spread_mesh start ~1e4 from the mesh, within far_r of far_c (so not flagged), and some hit the mesh"""
    sc, _ = C.spread_mesh()
    rays = C.far_origin_set(sc)
    far_c, far_r = C.far_rule(oracle, sc)
    assert far_r > 1e4
    assert (np.abs(rays[:, :3].astype(np.float64) - far_c).max(axis=1) <= far_r).all()
    assert np.abs(rays[:, :3]).max(axis=1).mean() > 3e3
    ora = oracle.trace(sc, rays, 1)
    assert (ora[:, 0] == 1).mean() > 0.3


@pytest.mark.parametrize("sid", ["d_C2_2^12", "d_R2_2^12"])
def test_inplane_rays_meet_the_plane_at_nan(oracle, sid):
    """the in-plane set reaches its regime: the oracle reports NaN-t hits among them"""
    sc, _ = dict((f[0], f[1]) for f in FAMILY)[sid]()
    rays = C.inplane_set(sc)
    ora = oracle.trace(sc, rays, 1)
    assert np.isnan(ora[ora[:, 0] == 1, 1]).any()
