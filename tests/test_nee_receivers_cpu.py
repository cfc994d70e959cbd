"""The float64 restatement tests/nee_receivers_ref.py, pinned without a GPU: the general density p_b(w; n) against 10^6 rejection-sampled
directions of n + u for |n| = 0, 0.05, 0.3, 1, 1.7 and 4 (binned chi^2, as test_light_sampling_cpu.py does for |n| = 1), its integral, its two
closed forms, its support; the quadrature sets against each other and against closed forms; and the composition of every probe table that
tests/test_gpu_nee_receivers.py renders, built from the reference alone: nothing is dropped from a table after GPU output has been seen."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_lights_ref as DR  # noqa: E402
import env_dist_ref as VR  # noqa: E402
import nee_receivers_ref as R  # noqa: E402

from firework_amd import _lib  # noqa: E402

LENGTHS = (0.0, 0.05, 0.3, 1.0, 1.7, 4.0)
AXIS = np.array([0.3, 0.8, -0.52]) / np.linalg.norm([0.3, 0.8, -0.52])


def _unit_ball(rng, n):
    """util.rs:36-43: 2 u - 1 for u uniform in the unit cube, rejected until |p|^2 < 1"""
    out = np.empty((0, 3))
    while out.shape[0] < n:
        p = 2.0 * rng.random((2 * n, 3)) - 1.0
        out = np.concatenate([out, p[(p * p).sum(1) < 1.0]])
    return out[:n]


def _bin_mass(length, edges, sub=2000):
    """P(cos in bin) = int p_b(c |n|, |n|^2) 2 pi dc, midpoint rule"""
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        c = a + (np.arange(sub) + 0.5) / sub * (b - a)
        out.append(float(R.density_cn(c * length, length * length).sum() * 2 * np.pi * (b - a) / sub))
    return np.array(out)


# ---- 1. the density ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", LENGTHS)
def test_density_matches_rejection_sampling(length):
    rng = np.random.default_rng(17)
    n = length * AXIS
    d = n[None, :] + _unit_ball(rng, 10 ** 6)
    cos = (d @ AXIS) / np.linalg.norm(d, axis=1)
    edges = np.linspace(-1.0, 1.0, 81)
    counts, _ = np.histogram(cos, edges)
    expected = _bin_mass(length, edges) * cos.size
    assert expected.sum() == pytest.approx(cos.size, rel=1e-4)
    assert np.all(counts[expected == 0] == 0)                       # nothing outside the support
    big = expected >= 5
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(expected[big], expected[~big].sum())
    keep = exp > 0
    chi2 = float(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum())
    dof = int(keep.sum()) - 1
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (length, chi2, dof)


@pytest.mark.parametrize("length", LENGTHS)
def test_density_integrates_to_one(length):
    m = 400000
    c = -1.0 + (np.arange(m) + 0.5) / m * 2.0
    total = float(R.density_cn(c * length, length * length).sum() * 2 * np.pi * 2.0 / m)
    assert total == pytest.approx(1.0, abs=2e-5), (length, total)


def test_density_closed_forms():
    rng = np.random.default_rng(3)
    w = rng.normal(size=(1000, 3))
    w /= np.linalg.norm(w, axis=1)[:, None]
    c = w @ AXIS
    assert np.allclose(R.scatter_density(AXIS, w), 2 * np.clip(c, 0, None) ** 3 / np.pi, rtol=1e-9, atol=1e-15)
    assert np.all(R.scatter_density(AXIS, w)[c <= 0] == 0.0)
    assert np.allclose(R.scatter_density(np.zeros(3), w), 1 / (4 * np.pi), rtol=1e-15)
    # the scalar form the delta-light reference already has agrees
    for k in range(0, 1000, 50):
        for length in LENGTHS:
            assert R.scatter_density(length * AXIS, w[k]) == pytest.approx(DR.scatter_pdf(length * AXIS, w[k]), rel=1e-12, abs=1e-30)


@pytest.mark.parametrize("length", [1.7, 4.0])
def test_density_is_zero_outside_the_cone(length):
    rng = np.random.default_rng(4)
    w = rng.normal(size=(20000, 3))
    w /= np.linalg.norm(w, axis=1)[:, None]
    cos = w @ AXIS
    sin = np.sqrt(1 - cos ** 2)
    p = R.scatter_density(length * AXIS, w)
    assert np.all(p[(sin > 1 / length) | (cos <= 0)] == 0.0)
    inside = (sin < (1 - 1e-9) / length) & (cos > 0)
    assert inside.sum() > 100 and np.all(p[inside] > 0)


@pytest.mark.parametrize("length", [0.05, 0.3])
def test_density_is_positive_below_the_surface(length):
    rng = np.random.default_rng(5)
    w = rng.normal(size=(20000, 3))
    w /= np.linalg.norm(w, axis=1)[:, None]
    p = R.scatter_density(length * AXIS, w)
    assert np.all(p > 0) and (w @ AXIS < 0).sum() > 5000
    assert np.all(R.scatter_density(length * AXIS, -w)[w @ AXIS > 0] < p[w @ AXIS > 0])       # less than towards the normal's side


def test_kappa():
    """|n| = 1: p_b = 2 c^3 / pi, so c alone gives 3 and |n|^2 adds 3 / (4 c^2); n = 0: the density does not depend on c"""
    w = np.array([0.6, 0.8, 0.0])
    assert R.kappa((0, 1.0, 0), w) == pytest.approx(3 + 0.75 / 0.64, rel=1e-3)
    assert R.kappa((0, 0, 0), w) == 1.0
    assert R.kappa((0, 4.0, 0), (0, 1.0, 0)) > 16           # why |n| = 4 has no deterministic probe


# ---- 2. the quadrature sets -------------------------------------------------------------------------------------------------------------------
P0 = np.array([0.2, -0.1, 0.3])
N0 = np.array([0.1, 1.3, -0.2])


def _rect_light():
    return dict(corners=np.array([[-0.3, 1.5, -0.2], [0.3, 1.5, -0.2], [0.3, 1.5, 0.2], [-0.3, 1.5, 0.2]]), p_pick=1.0)


def test_flat_sets_agree():
    """one quad as a rectangle, as two triangles and as the bottom face of a box: three point rules, one integral and one density"""
    a = R.moments(R.rect_set(_rect_light(), P0, R.LE), N0, R.ALB)
    verts = _rect_light()["corners"]
    b = R.moments(R.mesh_set(verts, R.QUAD_TRIS, P0, R.LE), N0, R.ALB)
    assert np.allclose(a["want"], b["want"], rtol=1e-5) and np.allclose(a["var_nee"], b["var_nee"], rtol=1e-4)
    under = np.array([0.1, -0.1, 0.05])
    box = R.box_set((-0.3, 1.5, -0.2), (0.6, 0.1, 0.4), under, R.LE)
    total = 2 * (0.6 * 0.1 + 0.6 * 0.4 + 0.1 * 0.4)
    rect = R.rect_set(_rect_light(), under, R.LE)
    assert box.dw.sum() == pytest.approx(rect.dw.sum(), rel=1e-5)            # from below only the bottom face is seen
    assert box.pl.min() * total == pytest.approx(rect.pl.min() * 0.24, rel=1e-3)   # p_omega = d^2 / (cos A_total): the faces are picked by area


def test_disk_and_sphere_sets_subtend_their_solid_angles():
    h, r = 1.3, 0.7
    q = R.disk_set((0, h, 0), np.eye(3), r, 0.0, 2 * np.pi, (0, 0, 0), R.LE)
    assert q.dw.sum() == pytest.approx(2 * np.pi * (1 - h / np.hypot(h, r)), rel=1e-4)
    half = R.disk_set((0, h, 0), np.eye(3), r, 0.0, np.pi, (0, 0, 0), R.LE)
    assert half.dw.sum() == pytest.approx(q.dw.sum() / 2, rel=1e-4)
    assert (q.pl * q.dw).sum() == pytest.approx(1.0, rel=1e-4)                # a density over the light
    s = R.sphere_set(dict(centre=np.array([0.5, 2.0, 0.1]), radius=0.4, p_pick=1.0), P0, R.LE)
    d = np.linalg.norm(np.array([0.5, 2.0, 0.1]) - P0)
    assert s.dw.sum() == pytest.approx(2 * np.pi * (1 - np.sqrt(1 - (0.4 / d) ** 2)), rel=1e-12)
    assert np.allclose(np.linalg.norm(s.w, axis=1), 1.0) and (s.pl * s.dw).sum() == pytest.approx(1.0)


def test_map_set_generalises_the_floor_quadrature():
    """for n = +y the per-texel numeric quadrature meets env_dist_ref.floor_answer's closed form; the picks are a density"""
    m = R.probe_map()
    q = R.map_set(m)
    mo = R.moments(q, (0, 1.0, 0), R.ALB)
    mean, var = VR.floor_answer(m, R.ALB[0])
    assert np.allclose(mo["want"], mean, rtol=2e-4)
    assert np.allclose(mo["var_default"], var, rtol=2e-4)
    assert (q.pl * q.dw).sum() == pytest.approx(1.0, rel=1e-9)
    assert np.array_equal(VR.env_texel(q.w, m.shape[1], m.shape[0]) // m.shape[1] == 1, q.w[:, 1] > 0)    # the directions look their texel up


def test_moments_split():
    mo = R.moments(R.rect_set(_rect_light(), P0, R.LE), N0, R.ALB)
    assert np.allclose(mo["parts"][0] + mo["parts"][1], mo["want"], rtol=1e-12)
    assert np.all(mo["var_nee"] > 0) and np.all(mo["var_nee"] < mo["var_default"])


@pytest.mark.parametrize("recv,light", [("mesh_1.7", "rect"), ("mesh_4", "sphere"), ("mesh_0.3", "box"), ("mesh_1.7", "map_rect"), ("mesh_1.7", "quad")])
def test_quadrature_has_converged(recv, light):
    """twice the points per axis move no answer by more than 2e-4 of it and no variance by more than 1 %: far inside the 1 % the probes test"""
    scene = R.build_scene(recv, light)
    for p in R.receiver(recv).probes[:3]:
        a = R.moments(R.quadrature(recv, light, p.P, scene), p.n, R.ALB)
        b = R.moments(R.quadrature(recv, light, p.P, scene, fine=2), p.n, R.ALB)
        assert np.allclose(a["want"], b["want"], rtol=2e-4), (a["want"], b["want"])
        assert np.allclose(a["var_nee"], b["var_nee"], rtol=1e-2)


# ---- 3. the tables ----------------------------------------------------------------------------------------------------------------------------
RECEIVERS = sorted({r for r, _ in R.RECEIVER_LIGHTS})


def test_every_receiver_and_light_of_the_issue_is_there():
    assert {"mesh_%s" % s for s in R.MESH_SIZES} <= set(RECEIVERS)
    assert {"mesh_rot_1.7", "mesh_vn_1", "rect_rotated", "sphere", "rect_below", "rect_flipped", "metal"} <= set(RECEIVERS)
    for s in ("mesh_0.3", "mesh_1.7"):
        assert {l for r, l in R.RECEIVER_LIGHTS if r == s} == set(R.AREA_LIGHTS + R.DELTA_LIGHTS)
    assert all(R.receiver("mesh_%s" % s).bvh == (True, False) for s in R.MESH_SIZES)
    assert min(abs(float(x)) for x in R.RAY_DIR) >= 0.2 and max(R.RAY_DIR) >= 0.2       # the signed largest component shears the triangle test


@pytest.mark.parametrize("recv", RECEIVERS)
def test_receiver_geometry(recv):
    rc = R.receiver(recv)
    assert 3 <= len(rc.probes) <= 9
    nn = np.array([np.linalg.norm(p.n) for p in rc.probes])
    assert np.allclose(nn, rc.nn, rtol=1e-5), nn
    if recv.startswith("mesh_") and not recv.startswith("mesh_rot"):
        verts = R.mesh_vertices(float(recv.split("_")[-1]))[0].astype(np.float64)
        for p in rc.probes:                                          # inside the triangle, away from its edges
            (b0, b1), *_ = np.linalg.lstsq(np.stack([verts[0] - verts[2], verts[1] - verts[2]], 1), p.P - verts[2], rcond=None)
            assert min(b0, b1, 1 - b0 - b1) > 0.005, (recv, b0, b1)
    if recv == "mesh_vn_1":                                          # tilted away from the geometric normal, and interpolated
        tilt = [np.degrees(np.arccos(p.n @ R.TILT)) for p in rc.probes]
        assert min(tilt) > 5 and max(tilt) - min(tilt) > 3, tilt
    if recv in ("mesh_rot_1.7", "rect_rotated"):                     # OF_ROTATED: cos of the rotation's angle below 0.999
        import emitters_ref as ER
        rot = ER.rotation(R.MESH_ROTOR if recv.startswith("mesh") else R.RECT_ROTOR)
        assert 0.5 * (np.trace(rot) - 1) < 0.9
    if recv == "rect_flipped":
        assert all(p.n[1] == -1.0 for p in rc.probes)
    if recv == "rect_below":
        assert all(p.n[1] == 1.0 and p.ray[1] < 0 < p.ray[4] for p in rc.probes)
    if recv == "sphere":
        lat = sorted(np.degrees(np.arccos(p.n[1])) for p in rc.probes)
        assert lat[0] < 15 < lat[1] < 40 < lat[2]
    if recv == "metal":
        assert len({float(x) for x in R.METAL}) == 3 and all(np.array_equal(p.beta, R.METAL) for p in rc.probes)


@pytest.mark.parametrize("recv", RECEIVERS)
def test_table_composition(recv):
    rc = R.receiver(recv)
    positive = zeros = 0
    for light in [l for r, l in R.RECEIVER_LIGHTS if r == recv]:
        t = R.table(recv, light)
        pos = t.want[:, 0] > 0
        assert np.array_equal(pos, (t.want > 0).all(1))
        assert np.all(t.zero_safe[~pos]), (recv, light)                 # an answer of 0 is 0 by a margin float32 cannot bridge
        assert not np.any(t.zero_safe[pos])
        assert np.all(t.need <= R.N_MAX), (recv, light, t.need)        # 4 standard errors within 1 % of the answer at 2^18 samples or fewer
        assert np.all(t.kappa <= 16), (recv, light, t.kappa)
        assert np.all(t.var_nee[pos] > 0) if t.stochastic else np.all(t.var_nee == 0)
        if recv != "rect_flipped":
            assert pos.sum() >= 3, (recv, light)
        positive += int(pos.sum())
        if light not in ("map", "map_rect", "sun"):                    # (a direction shared by every probe is inside the cone for all or none)
            zeros += int((~pos).sum())
            if rc.nn > 1:
                assert (~pos).sum() >= 2, (recv, light)
        if light == "spot":                                             # every probe inside the inner cone: s = 1 exactly
            lt = R.delta_light("spot", rc)
            ci = float(lt.to_abi().cos_inner)
            assert all(DR.spot_cosine(lt, p.P) >= ci + 1e-3 for p in rc.probes)
    if recv == "rect_flipped":
        assert positive == 0 and zeros >= 6
    else:
        assert positive >= 3
    if rc.nn > 1:
        assert zeros >= 2


def test_flipped_floor_has_back_facing_lights_at_every_angle():
    """float32 (c^2 - 1) + 1 equals c^2 only while c^2 >= 1/2: the probes behind the flipped floor reach down to c = -0.4"""
    rc = R.receiver("rect_flipped")
    c = [float(DR.incident(R.delta_light("point", rc), p.P)[0] @ p.n) for p in rc.probes]
    assert max(c) < -0.3 and min(c) < -0.99 and -0.5 < max(c)


def test_mirror_is_clear_of_the_light():
    """no segment from a floor point to the light, or to the light's mirror image, crosses the mirror: the probe's value is the metal's
    albedo times the floor's one-bounce answer and nothing else"""
    rc = R.receiver("metal")
    (l,) = _lib.selftest_lights(R.build_scene("metal", "rect").to_desc())
    c = l["corners"]
    S, T = R._grid(40)
    pts = c[0] + S[:, None] * (c[1] - c[0]) + T[:, None] * (c[3] - c[0])
    pts = np.concatenate([pts, rc.light_at[None, :]])
    image = pts * [-1.0, 1.0, 1.0] + [2 * R.MIRROR["x"], 0, 0]
    for p in rc.probes:
        assert p.P[1] == pytest.approx(0.0, abs=1e-12) and p.P[0] > R.MIRROR["x"]
        assert not R.crosses_mirror(p.P, pts) and not R.crosses_mirror(p.P, image)
    assert R.crosses_mirror((0.0, 0.7, 0.0), np.array([[-3.0, 0.7, 0.0]]))      # (the check can see a crossing)


@pytest.mark.parametrize("recv", ["mesh_0.3", "mesh_1.7"])
def test_rectangle_hides_no_bright_texel(recv):
    """bits 4 + 8: the two sets are joined as disjoint directions, so no direction of a bright texel may meet the rectangle"""
    (l,) = _lib.selftest_lights(R.build_scene(recv, "map_rect").to_desc())
    c = l["corners"]
    e1, e2 = c[1] - c[0], c[3] - c[0]
    nl = np.cross(e1, e2)
    w = R.map_set(R.probe_map()).w
    for p in R.receiver(recv).probes:
        t = ((c[0] - p.P) @ nl) / (w @ nl)
        X = p.P + t[:, None] * w - c[0]
        a, b = (X @ e1) / (e1 @ e1), (X @ e2) / (e2 @ e2)
        assert not np.any((t > 0) & (a > -0.05) & (a < 1.05) & (b > -0.05) & (b < 1.05))


@pytest.mark.parametrize("light", ["point", "sun"])
def test_medium_table(light):
    t = R.medium_table(light)
    assert t.rays.shape == (3, 6) and np.all(t.want > 0)
    assert np.all(t.need <= R.N_MAX), t.need
    tol = 4 * np.sqrt(t.var_nee / t.N)
    assert np.all(tol <= 0.01 * t.want)
    assert np.all(t.higher <= 0.1 * tol), (t.higher / tol).max()       # every order beyond the first: under a tenth of the tolerance
    assert R.MEDIUM_ALB == 2.0 ** -14 and R.MEDIUM_RHO == 0.5


def test_medium_answer_closed_form():
    """a directional light along the probe's own chord, from behind it: l(x_s) = s, so the integral is
    albedo E / 4 pi x rho ln10 int 10^(-2 rho s) ds = albedo E / 8 pi x (1 - 10^(-2 rho chord))"""
    from firework_amd.api import DirectionalLight
    ray = np.array([0.0, 5.0, 0.0, 0.0, -1.0, 0.0])
    mean, var, _ = R.medium_answer(ray, (0, 0, 0), 2.0, 0.5, 0.25, DirectionalLight((0.0, -1.0, 0.0), (3.0, 2.0, 1.0)))
    want = 0.25 * np.array([3.0, 2.0, 1.0]) / (8 * np.pi) * (1 - 10.0 ** (-2 * 0.5 * 4.0))
    assert np.allclose(mean, want, rtol=1e-6) and np.all(var > 0)
