"""GgxMat (FW_MAT_GGX) on the GPU, against the float64 restatement tests/ggx_ref.py.

The float32 budget of checks 1 and 2.  e = 2^-24.  The device forms f cos and p_b from the local directions wo, wi (three-term dot products
of unit vectors with the basis: absolute error at most 16 e per component, from 2.5 e in the normalised ray, 4 e in the basis and 3 e in
the sum, with sum |terms| <= sqrt 3) and their half vector h = (wo + wi) / |wo + wi|, |wo + wi| = 2 wo.h: the tangential part of h
carries an absolute error d <= 32 e / (2 wo.h).  D = alpha^2 / (pi s^2), s = |h_t|^2 + alpha^2 h_n^2, turns that into a relative error
2 |ds| / s <= 4 |h_t| d / s <= 2 d / (alpha h_n) (s >= 2 |h_t| alpha h_n), so

    budget(entry) = K e (1 / (alpha wo.h) + 2),  K = 32,

the second term for everything else (Lambda, Schlick, the quotients: fewer than 64 roundings).  This is the conditioning of D on float32
directions, whatever the evaluation: a lobe of roughness 0.03 seen at mu = 0.1 cannot be evaluated to better than about 1e-2 relative, one
of roughness 0.3 to 1e-5.  It is a worst case (the error of h_t in the worst direction, at |h_t| = alpha h_n).  Measured on an MI355X over
check 1's 512 entries: K = 2.34 for f cos and K = 1.96 for p_b (largest relative error 3.7e-4, at roughness 0.03); the test asserts
K = 9 for f cos and K = 7.5 for p_b, each under 4 x its own measured figure and under the derived 32.  Check 2's probes take f cos's bound
as it is, nothing added (roughness 0.3: about 1.2e-5 at wo.h = 0.5; measured: see DESIGN.md §9m).
The attenuation F G2 / G1 does not pass through D: its h comes from the sampler, not from a difference of directions, so it has a budget
of its own without the conditioning term.  Derived: Schlick's F takes wo.h's absolute error of about 20 e as 5 (1 - wo.h)^4 (1 - F0) / F
of it, at most 100 e at F0 >= 0.5; Lambda(wi) = (sqrt(1 + alpha^2 tan^2) - 1) / 2 takes up to twice the relative error of wi.n, 32 e / wi.n,
weighted by Lambda_i / (1 + Lambda_o + Lambda_i) <= 1, which no float32 form avoids towards grazing wi: attenuations are compared where
the restatement's wi.n >= 0.05, 1280 e at the worst; the rest is fewer than 64 roundings.  Measured: 1.34e-6 = 22.5 e relative at most over
the 474 compared entries; asserted: 80 e, under 4 x measured and far under the derived worst case.  The evaluated directions omega keep
omega.n >= 0.05 for the same reason (they are chosen that way).
The sampled direction itself is compared by components, |error| <= C e (1 + 1 / sin(theta_o)), C = 64 derived: the sampler builds its
tangent T1 from the stretched view's tangential part, whose direction carries the relative error 16 e / sin(theta_o) of wo's; that turns h
about n and wi by at most twice as much, and the components themselves carry 16 e from wo and h's error doubled by the reflection.  The
lobe is isotropic, so nothing else feels the azimuth; at exactly normal incidence it is arbitrary, and the entries there are the axis-aligned
ones, where wo = n exactly on both sides and both take the fixed tangent; all others keep sin(theta_o) > 0.3.  Measured: at most 9.4 of
C's units (18.7 e absolute); asserted C = 36, under 4 x measured.
The alive flag (wi.n > 0) may differ from the restatement's only where |wi.n| <= 64 e (16 e in wo, and h's error doubled by the
reflection); such entries are excluded by that rule, and at most 2 % may be."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import (CameraSettings, ColorEnv, DirectionalLight, EmissiveMat, GgxMat, HdrEnvironment, LambertianMat, PointLight,
                              Renderer, RenderObject, Scene, SpotLight, Sphere, XZRect)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_lights_ref as DL  # noqa: E402
import ggx_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
K_FCOS, K_PB = 9.0, 7.5            # measured 2.34 and 1.96: each under 4 x its own figure and under the derived 32 (module docstring)
E_ATTEN, C_WI = 80.0, 36.0         # units of e; measured 22.5 and 9.4


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _with(r, **kw):
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    for k, v in kw.items():
        getattr(rr, k)(v)
    return rr


def _same(a, b):
    assert np.array_equal(a.rgb8, b.rgb8)
    assert np.array_equal(_u32(a.gamma), _u32(b.gamma)) and np.array_equal(_u32(a.linear), _u32(b.linear))


def _budget(alpha, oh, k):
    return k * EPS * (1.0 / (alpha * oh) + 2.0)


# ---- 1. the lobe on the device --------------------------------------------------------------------------------------------------------
F0 = np.array([0.9, 0.7, 0.5], np.float32)
NORMALS = [(0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1),
           (0.3, 0.9, 0.1), (-0.2, 0.1, -0.95), (1, 0, 0)]


def _entries():
    """512 entries: 8 x 8 xi midpoints x 8 (roughness, incidence cosine, normal) combinations that cover the five roughnesses, cosines from
    1 down to 0.1 and every octant with both axis-aligned z normals; omega = a direction inside the lobe (the restatement's sample for a
    random xi) for three entries of four, and a broad one for the fourth; both kept at omega.n >= 0.05"""
    combos = [(0.03, 1.0, 0), (0.03, 0.3, 3), (0.1, 0.1, 1), (0.1, 0.7, 5), (0.3, 0.5, 2), (0.3, 0.1, 7), (0.6, 0.25, 9), (1.0, 0.1, 11)]
    extra = [(1.0, 0.9, 4), (0.6, 0.95, 6), (0.3, 0.8, 8), (0.1, 0.4, 10), (0.03, 0.6, 12)]          # the fourth-entry slots' own combos
    rng = np.random.default_rng(11)
    g = (np.arange(8) + 0.5) / 8
    rows = []
    for ci, (rough, mu, ni) in enumerate(combos):
        for a in range(8):
            for b in range(8):
                k = len(rows)
                if k % 4 == 3:
                    rough_, mu_, ni_ = extra[(k // 4) % len(extra)]
                else:
                    rough_, mu_, ni_ = rough, mu, ni
                n = np.array(NORMALS[ni_], np.float64)
                n = (n / np.linalg.norm(n)).astype(np.float32).astype(np.float64)
                t, bt = G.basis(n)
                phi = 2.0 * np.pi * rng.random()
                s = np.sqrt(max(1.0 - mu_ * mu_, 0.0))
                wo = mu_ * n + s * (np.cos(phi) * t + np.sin(phi) * bt)
                side = -1.0 if (k % 7 == 0) else 1.0                       # some normals face away from the ray: the flip
                d = (-wo * (0.5 + 2.0 * rng.random())).astype(np.float32)   # the ray, unnormalised
                xi1, xi2 = np.float32(g[a]), np.float32(g[b])
                if k % 4 == 3:
                    z = 0.05 + 0.95 * rng.random()
                    ph = 2.0 * np.pi * rng.random()
                    om = z * n + np.sqrt(1 - z * z) * (np.cos(ph) * t + np.sin(ph) * bt)
                else:
                    om = None
                    for tries in range(256):
                        cand, _, alive, wz = G.sample(side * n, d, rough_, 1.0, rng.random(), rng.random())
                        if alive and wz >= 0.05:
                            om = cand
                            break
                    assert om is not None
                rows.append(np.concatenate([side * n, d, [rough_], F0, [xi1, xi2], om * (0.7 + rng.random())]).astype(np.float32))
    return np.stack(rows)


def test_lobe_against_the_restatement():
    e = _entries()
    assert e.shape == (512, A.FW_GGX_IN_FLOATS)
    n, d, rough, f0, xi1, xi2, om = e[:, 0:3], e[:, 3:6], e[:, 6], e[:, 7:10], e[:, 10], e[:, 11], e[:, 12:15]
    assert set(np.round(rough.astype(np.float64), 2)) == {0.03, 0.1, 0.3, 0.6, 1.0}
    wi, att, alive, wz = G.sample(n, d, rough, f0, xi1, xi2)
    fcos, pb = G.evaluate(n, d, rough, f0, om)
    fr = G.frame(n, d)
    alpha = G.alpha_of(rough)
    wo = fr[3]
    assert wo[:, 2].min() > 0.09 and wo[:, 2].max() > 0.999
    om_l = G.to_local(fr, om / np.linalg.norm(om.astype(np.float64), axis=1)[:, None])
    assert om_l[:, 2].min() >= 0.049 and np.all(pb > 0)
    unsure = np.abs(wz) <= 64 * EPS
    assert unsure.mean() <= 0.02, unsure.mean()                                # (checked on the CPU, before anything runs)
    got = _lib.selftest_ggx(e)
    keep = ~unsure
    assert np.array_equal(got["alive"][keep], alive[keep])
    assert np.all(got["atten"][~got["alive"]] == 0)
    # the sampled direction: unit-vector components, absolute; the azimuth term of the module docstring (sin = 0 only where the incidence
    # is exactly normal in float32 too, the axis-aligned entries: both sides then take the fixed tangent)
    sin_o = np.sqrt(wo[:, 0] ** 2 + wo[:, 1] ** 2)
    assert np.all((sin_o == 0) | (sin_o > 0.3)) and (sin_o == 0).sum() >= 32
    bound_wi = C_WI * EPS * (1.0 + np.where(sin_o > 0, 1.0 / np.maximum(sin_o, 1e-30), 0.0))
    err_wi = np.abs(got["wi"].astype(np.float64) - wi).max(1)
    # the attenuation, where wi is not grazing
    cmp_a = keep & alive & (wz >= 0.05)
    assert cmp_a.sum() >= 0.6 * len(e)
    rel_a = (np.abs(got["atten"].astype(np.float64) - att) / np.where(att > 0, att, 1.0)).max(1)
    ea = rel_a[cmp_a].max() / EPS
    # f cos and p_b of omega
    h_e = wo + om_l
    oh_e = np.sum(wo * h_e / np.linalg.norm(h_e, axis=1)[:, None], -1)
    rel_f = (np.abs(got["fcos"].astype(np.float64) - fcos) / fcos).max(1)
    rel_p = np.abs(got["pb"].astype(np.float64) - pb) / pb
    kf, kp = (rel_f / _budget(alpha, oh_e, 1.0)).max(), (rel_p / _budget(alpha, oh_e, 1.0)).max()
    print(f"ggx lobe, 512 entries: |wi - ref| max {err_wi.max():.3g} ({err_wi.max() / EPS:.1f} e, C = {(err_wi / bound_wi).max() * C_WI:.3g}); attenuation {ea:.3g} e over {cmp_a.sum()} "
          f"entries (largest relative error {rel_a[cmp_a].max():.3g}); f cos K = {kf:.3g} (largest relative error {rel_f.max():.3g}); "
          f"p_b K = {kp:.3g} (largest relative error {rel_p.max():.3g}); alive flags excluded {int(unsure.sum())}")
    assert np.all(err_wi <= bound_wi)
    assert ea <= E_ATTEN and kf <= K_FCOS and kp <= K_PB


# ---- 2. exact probes ------------------------------------------------------------------------------------------------------------------
ROUGH, F0_FLOOR = 0.3, (0.9, 0.7, 0.5)
SAMPLES = 16
POINT = PointLight((0.3, 2.0, -0.2), (9.0, 6.0, 3.0))
SPOT = SpotLight((0.0, 3.0, 0.0), (0.2, -1.0, 0.1), (30.0, 20.0, 10.0), 30.0, 50.0)
SUN = DirectionalLight((0.3, -1.0, 0.2), (2.0, 1.5, 1.0))
UP = (0.0, 1.0, 0.0)


def _floor_scene(blocker=None, env=(0.0, 0.0, 0.0), emitter=None):
    scene = Scene.new()
    floor = scene.add_material(GgxMat.new(F0_FLOOR, ROUGH))
    scene.add_object(RenderObject.new(XZRect.new(-50, 50, -50, 50, 0, floor)))
    if blocker is not None:
        black = scene.add_material(EmissiveMat.with_color((0.0, 0.0, 0.0)))
        scene.add_object(RenderObject.new(Sphere.new(blocker[1], black)).position(*blocker[0]))
    if emitter is not None:
        em = scene.add_material(EmissiveMat.with_color((emitter[2],) * 3))
        scene.add_object(RenderObject.new(Sphere.new(emitter[1], em)).position(*emitter[0]))
    scene.set_environment(ColorEnv(env))
    return scene


def _probe_set():
    """14 floor points x 3 directions (vertical and two oblique ones): rays from above onto (x, 0, z)"""
    pts = [(x, z) for x in (-1.4, -0.5, 0.4, 1.3) for z in (-1.1, 0.2, 1.2)] + [(0.3, -0.2), (2.2, 1.9)]
    dirs = [(0.0, -1.0, 0.0), (0.6, -0.7, 0.2), (-0.3, -0.4, -0.8)]
    rays, hit = [], []
    for p in pts:
        for d in dirs:
            d = np.array(d)
            o = np.array([p[0], 0.0, p[1]]) - d * (0.9 / -d[1])
            rays.append(np.concatenate([o, d]))
            hit.append((p[0], 0.0, p[1]))
    return np.array(rays, np.float32), hit


def _probe(light, blocker=None):
    rays, hit = _probe_set()
    scene = _floor_scene(blocker)
    scene.add_light(light)
    ds = _lib.DeviceScene(scene.to_desc())
    return ds.render_rays(rays, SAMPLES, seed=7).linear.astype(np.float64), rays, hit


def _want(light, rays, hit):
    """f cos L / p (one light: p = 1) at the hit the float32 ray reaches, and the entry's budget"""
    out, bud = [], []
    for r, x in zip(rays.astype(np.float64), hit):
        t = -r[1] / r[4]
        x = r[0:3] + t * r[3:6]
        x[1] = 0.0
        w, L, _ = DL.incident(light, x)
        fcos, pb = G.evaluate(UP, r[3:6], ROUGH, np.array(F0_FLOOR, np.float32), w)
        fr = G.frame(np.array(UP), r[3:6])
        h = fr[3] + G.to_local(fr, w)
        oh = float(np.sum(fr[3] * h) / np.linalg.norm(h))
        out.append(fcos * L)
        bud.append(_budget(float(G.alpha_of(ROUGH)), oh, K_FCOS))          # check 1's bound for f cos, as it is
    return np.array(out), np.array(bud)


def _check_exact(got, want, bud, name):
    lit = want.max(1) > 0
    err = np.abs(got - want)[lit] / want[lit]
    print(f"{name}: {len(want)} probes, {int(lit.sum())} lit, largest relative error {err.max():.3g}, largest error / bound {(err / bud[lit, None]).max():.3g}")
    assert np.all(err <= bud[lit, None])
    assert np.all(got[~lit] == 0.0)


@pytest.mark.parametrize("name,light", [("point", POINT), ("spot", SPOT), ("directional", SUN)])
def test_probes(name, light):
    """The bounced ray leaves into the black environment (or ends below the floor), so a probe's value is its light sample alone, the same
    number in every sample — also for the samples whose own scattered direction ended the path"""
    got, rays, hit = _probe(light)
    want, bud = _want(light, rays, hit)
    assert (want.max(1) > 0).sum() >= 30
    assert np.ptp(want[:, 0][want[:, 0] > 0]) > 0.5 * want[:, 0].max()            # (F, G and D vary over the probes)
    _check_exact(got, want, bud, name)


def test_probe_zero_below_the_floor_and_in_the_umbra():
    rays, hit = _probe_set()
    scene = _floor_scene()
    scene.add_light(PointLight((0.0, -2.0, 0.0), (9.0, 9.0, 9.0)))          # under the floor: wi.n < 0 at every probe
    assert np.all(_lib.DeviceScene(scene.to_desc()).render_rays(rays, SAMPLES, seed=7).linear == 0.0)
    light = PointLight((0.0, 4.0, 0.0), (9.0, 6.0, 3.0))
    umbra = np.array([[x, 0.5, z, 0.0, -1.0, 0.0] for x, z in [(0.0, 0.0), (0.5, 0.3), (-0.7, 0.0), (0.0, 0.9)]], np.float32)
    out = np.array([[x, 0.5, z, 0.0, -1.0, 0.0] for x, z in [(1.5, 0.0), (0.0, -1.6), (2.0, 2.0)]], np.float32)
    res = {}
    for blocker in (None, ((0.0, 2.0, 0.0), 0.5)):           # the umbra on the floor: radius 4 tan(asin(0.25)) = 1.033
        scene = _floor_scene(blocker)
        scene.add_light(light)
        res[blocker is None] = _lib.DeviceScene(scene.to_desc()).render_rays(np.concatenate([umbra, out]), SAMPLES, seed=7).linear
    assert np.all(res[True] > 0)
    assert np.all(res[False][:4] == 0.0) and np.array_equal(_u32(res[False][4:]), _u32(res[True][4:]))


# ---- 3. sampling against evaluation (furnace) -----------------------------------------------------------------------------------------
def test_furnace():
    """A unit sphere of GgxMat, F0 = 1, inside a white environment: a path that survives the vertex leaves (the sphere is convex), so a sample
    is the attenuation in [0, 1] or 0, its mean E(mu, alpha) and its variance at most E (1 - E)"""
    mus, roughs, spp = (1.0, 0.8, 0.5, 0.25, 0.1), (0.1, 0.3, 0.6, 1.0), 4096
    rays = np.array([[np.sqrt(1 - mu * mu), 0.0, 5.0, 0.0, 0.0, -1.0] for mu in mus], np.float32)          # meets the sphere at n.wo = mu
    worst = 0.0
    for rough in roughs:
        scene = Scene.new()
        m = scene.add_material(GgxMat.new((1.0, 1.0, 1.0), rough))
        scene.add_object(RenderObject.new(Sphere.new(1.0, m)))
        scene.set_environment(ColorEnv((1.0, 1.0, 1.0)))
        got = _lib.DeviceScene(scene.to_desc()).render_rays(rays, spp, seed=11).linear.astype(np.float64)
        for k, mu in enumerate(mus):
            mu32 = float(np.sqrt(1.0 - float(rays[k, 0]) ** 2))
            e = G.albedo(mu32, rough)
            bound = 4.5 * np.sqrt(max(e * (1 - e), 0.0) / spp) + 1e-5
            z = abs(got[k, 0] - e) / bound
            worst = max(worst, z)
            print(f"furnace roughness {rough} mu {mu}: mean {got[k, 0]:.5f} E {e:.5f} |diff| / bound {z:.2f}")
            assert np.all(got[k] == got[k, 0]) and abs(got[k, 0] - e) <= bound
    print(f"furnace: largest |diff| / bound {worst:.2f}")


# ---- 4. MIS ---------------------------------------------------------------------------------------------------------------------------
def test_light_sampling_agrees_and_lowers_the_variance():
    seeds, spp = 8, 1024
    scene = _floor_scene(emitter=((0.0, 2.0, 0.0), 0.5, 10.0))
    ds = _lib.DeviceScene(scene.to_desc())
    rays = np.array([[x - 0.45 * dx, 0.9, z - 0.45 * dz, 0.5 * dx, -1.0, 0.5 * dz]
                     for (x, z), (dx, dz) in zip([(a, b) for a in (-1.2, -0.3, 0.5, 1.4) for b in (-1.0, -0.2, 0.6, 1.5)],
                                                 [(0, 0), (1, 0), (0, 1), (-1, 1)] * 4)], np.float32)
    a = np.stack([ds.render_rays(rays, spp, seed=s, flags=A.FW_FLAG_LIGHT_SAMPLING).linear.astype(np.float64).mean(1) for s in range(seeds)])
    b = np.stack([ds.render_rays(rays, spp, seed=s).linear.astype(np.float64).mean(1) for s in range(seeds)])
    se = np.sqrt((a.var(0, ddof=1) + b.var(0, ddof=1)) / seeds)
    z = np.abs(a.mean(0) - b.mean(0)) / np.maximum(se, 1e-12)
    lower = a.var(0, ddof=1) < b.var(0, ddof=1)
    print("MIS: with the flag", np.array2string(a.mean(0), precision=4), "without", np.array2string(b.mean(0), precision=4), "z",
          np.array2string(z, precision=2), "variance lower on", int(lower.sum()), "of 16")
    assert b.mean(0).min() > 0
    assert z.max() <= 4.0, z
    assert lower.sum() >= 12


# ---- 5. paths -------------------------------------------------------------------------------------------------------------------------
def _ggx_cornell(w=32, h=32, spp=16):
    scene, r = scenes.config("C2_cornell_box", w, h, spp)
    g = scene.add_material(GgxMat.new((0.9, 0.8, 0.6), 0.3))
    for ro in scene.render_objects[6:8]:
        ro.obj.material = g
    return scene, r


def test_same_paths_with_a_point_light():
    scene, r = _ggx_cornell()
    ds = _lib.DeviceScene(scene.to_desc())
    a = ds.render(r)
    ds.set_lights([PointLight((278.0, 400.0, 278.0), (60000.0, 50000.0, 40000.0))])
    b = ds.render(r)
    assert a.stats["rays"] == b.stats["rays"]
    assert [int(x) for x in a.stats["rays_per_depth"]] == [int(x) for x in b.stats["rays_per_depth"]]
    assert b.linear.astype(np.float64).mean() > 1.05 * a.linear.astype(np.float64).mean()
    c = ds.render(_with(r, light_sampling=True))
    assert [int(x) for x in a.stats["rays_per_depth"]] == [int(x) for x in c.stats["rays_per_depth"]]


# ---- 6. off means off, and composition --------------------------------------------------------------------------------------------------
_FRESH = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from firework_amd import _lib, scenes
scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
res = _lib.DeviceScene(scene.to_desc()).render(r)
np.savez(sys.argv[2], rgb8=res.rgb8, gamma=res.gamma, linear=res.linear)
"""


def test_cornell_after_a_ggx_scene_is_a_fresh_process_frame(tmp_path):
    gs, gr = _ggx_cornell()
    _lib.DeviceScene(gs.to_desc()).render(_with(gr, light_sampling=True))
    scene, r = scenes.config("C2_cornell_box", 64, 64, 16)
    here = _lib.DeviceScene(scene.to_desc()).render(r)
    out = tmp_path / "fresh.npz"
    subprocess.run([sys.executable, "-c", _FRESH, ROOT, str(out)], check=True, timeout=120)
    f = np.load(out)
    assert np.array_equal(here.rgb8, f["rgb8"]) and np.array_equal(_u32(here.gamma), _u32(f["gamma"])) and np.array_equal(_u32(here.linear), _u32(f["linear"]))


@pytest.mark.parametrize("ls", [False, True])
def test_composition(ls):
    scene, r = _ggx_cornell(64, 64, 16)
    scene.add_light(PointLight((278.0, 400.0, 278.0), (60000.0, 50000.0, 40000.0)))
    r = _with(r, light_sampling=ls)
    ds = _lib.DeviceScene(scene.to_desc())
    full = ds.render(r)
    ids = np.random.default_rng(5).choice(64 * 64, 700, replace=False).astype(np.uint32)
    sub = ds.render(r, pixel_ids=ids)
    assert np.array_equal(sub.rgb8, full.rgb8[ids]) and np.array_equal(_u32(sub.linear), _u32(full.linear[ids]))
    accum = np.zeros((64 * 64, 4), np.float32)
    r4 = _with(r, samples=4)
    for k in range(4):
        res = ds.render_progressive(r4, 4 * k, accum)
    _same(res, full)
    rays = np.stack([ds.camera_rays(r, s) for s in range(16)])
    rr = ds.render_rays(rays, 16, seed=r.settings["seed"], use_bvh=bool(r.settings["use_bvh"]), flags=A.FW_FLAG_LIGHT_SAMPLING if ls else 0)
    assert np.array_equal(rr.rgb8, full.rgb8) and np.array_equal(_u32(rr.linear), _u32(full.linear))


def test_one_shot_equals_the_resident_scene():
    scene, r = _ggx_cornell(64, 64, 16)
    for rr in (r, _with(r, light_sampling=True)):
        _same(_lib.render_scene(scene.to_desc(), rr), _lib.DeviceScene(scene.to_desc()).render(rr))


def test_env_sampling_queues_no_shadow_rays_at_ggx_vertices():
    """A GgxMat sphere alone under an HDR map: under FW_FLAG_ENV_SAMPLING its vertices take no light sample, so the frame walks the rays of
    the unflagged frame and, every vertex being a GgxMat one, is that frame"""
    rng = np.random.default_rng(2)
    env = (rng.random((16, 32, 3)) ** 4 * 20.0).astype(np.float32)
    scene = Scene.new()
    m = scene.add_material(GgxMat.new((0.9, 0.8, 0.6), 0.4))
    scene.add_object(RenderObject.new(Sphere.new(1.0, m)))
    scene.set_environment(HdrEnvironment(env))
    cam = CameraSettings.default().cam_pos((0.0, 1.0, 4.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = Renderer.default().width(32).height(32).samples(16).use_bvh(True).camera(cam)
    ds = _lib.DeviceScene(scene.to_desc())
    plain, flagged = ds.render(r), ds.render(_with(r, env_sampling=True))
    assert flagged.stats["rays"] == plain.stats["rays"]
    assert [int(x) for x in flagged.stats["rays_per_depth"]] == [int(x) for x in plain.stats["rays_per_depth"]]
    assert np.array_equal(_u32(flagged.linear), _u32(plain.linear)) and plain.linear.max() > 0


@pytest.mark.parametrize("env", [False, True])
def test_all_emitters_queue_no_shadow_rays_at_ggx_vertices(env):
    """The same under FW_FLAG_ALL_EMITTERS (k_shade_gx_nee's PL and ENV + PL forms): a GgxMat sphere beside an emissive sphere, every
    scattering vertex a GgxMat one, so the flagged frame walks the unflagged frame's rays and is that frame, bit for bit"""
    scene = Scene.new()
    m = scene.add_material(GgxMat.new((0.9, 0.8, 0.6), 0.4))
    em = scene.add_material(EmissiveMat.with_color((6.0, 5.0, 4.0)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, m)))
    scene.add_object(RenderObject.new(Sphere.new(0.5, em)).position(1.2, 1.6, 0.8))
    if env:
        rng = np.random.default_rng(2)
        scene.set_environment(HdrEnvironment((rng.random((16, 32, 3)) ** 4 * 20.0).astype(np.float32)))
    else:
        scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    cam = CameraSettings.default().cam_pos((0.0, 1.0, 4.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    r = Renderer.default().width(32).height(32).samples(16).use_bvh(True).camera(cam)
    ds = _lib.DeviceScene(scene.to_desc())
    plain = ds.render(r)
    rf = _with(r, light_sampling=True, all_emitters=True)
    if env:
        rf = _with(rf, env_sampling=True)
    flagged = ds.render(rf)
    assert rf.to_params().flags & A.FW_FLAG_ALL_EMITTERS
    assert [int(x) for x in flagged.stats["rays_per_depth"]] == [int(x) for x in plain.stats["rays_per_depth"]]
    assert np.array_equal(_u32(flagged.linear), _u32(plain.linear)) and plain.linear.max() > 0


def _checker_below(scene):
    """a checker-textured sphere under the floor, where no ray goes (the probes come from above and a surviving ray leaves upwards): the
    scene now holds an expensive texture, so its frames take the in-line shading mode 0 (k_shade_gx<., 0> and k_shade_gx_nee<., 0, ...>)
    instead of mode 1, and nothing else about them changes"""
    from firework_amd.api import CheckerTexture
    c = scene.add_material(LambertianMat.new(CheckerTexture.with_colors((0.2, 0.4, 0.1), (0.9, 0.9, 0.9), 10.0)))
    scene.add_object(RenderObject.new(Sphere.new(1.0, c)).position(0.0, -5.0, 0.0))


def test_probes_in_shading_mode_0():
    """The point light's probes again in a scene that also holds a checker texture (mode 0 with delta lights): the same bound"""
    rays, hit = _probe_set()
    scene = _floor_scene()
    _checker_below(scene)
    scene.add_light(POINT)
    got = _lib.DeviceScene(scene.to_desc()).render_rays(rays, SAMPLES, seed=7).linear.astype(np.float64)
    want, bud = _want(POINT, rays, hit)
    _check_exact(got, want, bud, "point, mode 0")


def test_light_sampling_in_shading_mode_0_equals_mode_1():
    """The MIS scene with and without the unreachable checker sphere, under FW_FLAG_LIGHT_SAMPLING and without it: mode 0 and mode 1 do the
    same float32 operations on the same paths (no contraction), so the frames are equal bit for bit"""
    rays = np.array([[x, 0.9, z, 0.1, -1.0, 0.2] for x in (-1.0, 0.0, 1.0) for z in (-1.0, 0.5)], np.float32)
    out = {}
    for checker in (False, True):
        scene = _floor_scene(emitter=((0.0, 2.0, 0.0), 0.5, 10.0))
        if checker:
            _checker_below(scene)
        ds = _lib.DeviceScene(scene.to_desc())
        out[checker] = (ds.render_rays(rays, 64, seed=3, flags=A.FW_FLAG_LIGHT_SAMPLING), ds.render_rays(rays, 64, seed=3))
    for k in (0, 1):
        assert [int(x) for x in out[True][k].stats["rays_per_depth"]] == [int(x) for x in out[False][k].stats["rays_per_depth"]]
        assert np.array_equal(_u32(out[True][k].linear), _u32(out[False][k].linear))
    assert np.all(out[True][0].linear.max(1) > 0)


# ---- 7. AOVs --------------------------------------------------------------------------------------------------------------------------
def test_aov_albedo_is_f0():
    f0 = (0.9, 0.7, 0.5)
    scene = Scene.new()
    m = scene.add_material(GgxMat.new(f0, 0.3))
    scene.add_object(RenderObject.new(Sphere.new(1.0, m)))
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    cam = CameraSettings.default().cam_pos((0.0, 0.0, 1.2)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)       # the sphere fills the frame
    r = Renderer.default().width(16).height(16).samples(4).use_bvh(True).camera(cam)
    aov = _lib.DeviceScene(scene.to_desc()).aovs(r, 4)
    assert np.all(aov[:, 3] == 1.0)                                                     # coverage: every sample hit
    assert np.array_equal(_u32(aov[:, 0:3]), _u32(np.tile(np.float32(f0), (256, 1))))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("roughness", 0.02), ("roughness", 1.5), ("albedo", (0.5, 1.2, 0.5)), ("albedo", (0.5, float("nan"), 0.5))])
def test_out_of_range_is_refused(field, value):
    scene = _floor_scene()
    scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    g = scene.add_material(GgxMat.new((0.5, 0.5, 0.5), 0.5))
    scene.add_object(RenderObject.new(Sphere.new(1.0, g)).position(0.0, 1.0, 0.0))
    desc = scene.to_desc()
    mat = desc.materials[g]
    if field == "roughness":
        mat.roughness = value
    else:
        mat.albedo = A.vec3(value)
    with pytest.raises(_lib.FireworkError) as e:
        _lib.DeviceScene(desc)
    assert e.value.status == A.FW_ERR_BAD_ARG and f"material {g}" in str(e.value) and "GgxMat" in str(e.value)
    good = _lib.DeviceScene(scene.to_desc())                                            # a scene created afterwards renders
    rays = np.array([[0.2, 3.0, 0.1, 0.0, -1.0, 0.0]], np.float32)
    scene2 = _floor_scene()
    scene2.add_light(POINT)
    assert _lib.DeviceScene(scene2.to_desc()).render_rays(rays, 4, seed=1).linear.max() > 0
    good.close()
