"""GgxMat (FW_MAT_GGX) without a GPU: the float64 restatement the GPU tests measure the device against (tests/ggx_ref.py)
on values computed by hand and on its own invariants — normalisation of the density, reciprocity, energy, and the sampler's expectation
against the quadrature of what it is meant to sample —, and the host layers: the ABI constant, Scene.to_desc, the range errors, the YAML
tag (round trip; files without it dump as before) and the example scene."""
import os
import sys

import numpy as np
import pytest
import yaml

from firework_amd import _abi as A
from firework_amd import scenes, yaml_io
from firework_amd.api import ColorEnv, GgxMat, LambertianMat, MetalMat, RenderObject, Scene, Sphere

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ggx_ref as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = np.array([0.0, 0.0, 1.0])


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_basis_is_orthonormal_on_both_sides_of_the_sign_branch():
    rng = np.random.default_rng(3)
    n = rng.normal(size=(200, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    n = np.concatenate([n, [[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0], [0, -1.0, 0], [1e-9, 0, -1.0]]])
    n /= np.linalg.norm(n, axis=1)[:, None]
    t, b = G.basis(n)
    for u, v, want in ((t, t, 1), (b, b, 1), (t, b, 0), (t, n, 0), (b, n, 0)):
        assert np.abs(np.sum(u * v, -1) - want).max() < 1e-12
    assert np.abs(np.cross(t, b) - n).max() < 1e-12


@pytest.mark.parametrize("roughness", [0.03, 0.3, 1.0])
def test_normal_incidence_by_hand(roughness):
    """wo = wi = n: h = n, D = 1 / (pi alpha^2), Lambda = 0 and G2 = G1 = 1, F = F0: f cos = F0 / (4 pi alpha^2), p_b = 1 / (4 pi alpha^2)"""
    f0 = np.array([0.9, 0.7, 0.5])
    a = float(G.alpha_of(roughness))
    fcos, pb = G.eval_local(UP, UP, a, f0)
    assert np.allclose(fcos, f0 / (4 * np.pi * a * a), rtol=1e-14) and np.isclose(pb, 1 / (4 * np.pi * a * a), rtol=1e-14)
    # through the world-space entry, with a normal that has to be flipped and an unnormalised ray
    fcos2, pb2 = G.evaluate((0.0, -1.0, 0.0), (0.0, -3.0, 0.0), roughness, f0, (0.0, 2.0, 0.0))
    assert np.allclose(fcos2, fcos, rtol=1e-13) and np.isclose(pb2, pb, rtol=1e-13)


def test_schlick_ends():
    f0 = np.array([0.04, 0.5, 1.0])
    assert np.array_equal(G.schlick(f0, 1.0), f0) and np.array_equal(G.schlick(f0, 0.0), np.ones(3))
    assert np.allclose(G.schlick(f0, 0.5), f0 + (1 - f0) / 32)


def test_below_the_surface_is_zero():
    fcos, pb = G.eval_local(G.wo_of(0.5), np.array([0.6, 0.0, -0.8]), 0.09, 1.0)
    assert np.all(fcos == 0) and pb == 0


@pytest.mark.parametrize("roughness", [0.03, 0.1, 0.3, 0.6, 1.0])
@pytest.mark.parametrize("mu", [1.0, 0.5, 0.1])
def test_density_integrates_to_one(mu, roughness):
    """Over all wi, the mass below the horizon included (those samples end the path).  The midpoint rule on the 512 x 1024 grid of
    ggx_ref.half_vector_grid leaves |integral - 1| <= 1.6e-6 in float64 over these fifteen cases (its second-order error in theta_h; measured
    on the restatement alone, largest at mu = 1); the bound is 10 x that."""
    res = G.pdf_mass(mu, roughness) - 1.0
    print(f"mu {mu} roughness {roughness}: integral - 1 = {res:.3e}")
    assert abs(res) <= 1.6e-5


def test_reciprocity():
    """f(wo, wi) = f(wi, wo): f cos / cos(theta_i) is symmetric"""
    rng = np.random.default_rng(5)
    w = rng.normal(size=(2, 300, 3))
    w[..., 2] = np.abs(w[..., 2]) + 0.05
    w /= np.linalg.norm(w, axis=-1)[..., None]
    for a in (0.0009, 0.09, 1.0):
        f_ab = G.eval_local(w[0], w[1], a, np.array([0.9, 0.7, 0.5]))[0] / w[1][:, 2:3]
        f_ba = G.eval_local(w[1], w[0], a, np.array([0.9, 0.7, 0.5]))[0] / w[0][:, 2:3]
        assert np.allclose(f_ab, f_ba, rtol=1e-12, atol=0)


CASES = [(mu, r) for mu in (1.0, 0.5, 0.1) for r in (0.1, 0.5, 1.0)]


@pytest.mark.parametrize("mu,roughness", CASES)
def test_albedo_at_most_one_and_sampler_expectation(mu, roughness):
    """E(mu, alpha) <= 1 at F0 = 1 (single scattering loses energy, never gains), and the mean of the sampled attenuation over 2^16
    stratified (xi1, xi2) equals it: each sample lies in [0, 1], so its variance is at most E (1 - E) (Bhatia-Davis) and stratification
    only lowers the mean's; 4.5 standard errors of 2^16 independent samples plus 10 x the quadrature's 1.6e-6."""
    e = G.albedo(mu, roughness)
    s = G.expected_attenuation(mu, roughness, m=256)
    bound = 4.5 * np.sqrt(max(e * (1.0 - e), 0.0) / 65536) + 1.6e-5
    print(f"mu {mu} roughness {roughness}: E {e:.6f} sampled {s:.6f} bound {bound:.2e}")
    assert 0.0 < e <= 1.0 + 1.6e-5
    assert abs(s - e) <= bound


def test_sample_matches_its_own_density_direction():
    """A sampled wi evaluated again: alive samples have positive f cos and p_b, and attenuation = f cos / p_b (the estimator's weight)"""
    rng = np.random.default_rng(9)
    n = 500
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    d = rng.normal(size=(n, 3))
    f0 = np.array([0.9, 0.7, 0.5])
    for r in (0.1, 0.5, 1.0):
        wi, att, alive, _ = G.sample(nrm, d, r, f0, rng.random(n), rng.random(n))
        fcos, pb = G.evaluate(nrm, d, r, f0, wi)
        assert alive.sum() > n // 2
        assert np.all(pb[alive] > 0) and np.allclose(att[alive], fcos[alive] / pb[alive][:, None], rtol=1e-9)
        assert np.all(att[~alive] == 0)


# ---- the host layers ------------------------------------------------------------------------------------------------------------------
def _scene(albedo=(0.9, 0.7, 0.5), roughness=0.3):
    scene = Scene.new()
    scene.add_material(LambertianMat.with_color((0.5, 0.5, 0.5)))
    m = scene.add_material(GgxMat.new(albedo, roughness))
    scene.add_object(RenderObject.new(Sphere.new(1.0, m)))
    scene.set_environment(ColorEnv((0.0, 0.0, 0.0)))
    return scene


def test_to_desc_carries_kind_5():
    assert A.FW_MAT_GGX == 5
    src = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert "FW_MAT_GGX = 5" in src and "fw_selftest_ggx" in src
    m = _scene().to_desc().materials[1]
    assert m.kind == A.FW_MAT_GGX and m.texture == -1
    assert (m.albedo.x, m.albedo.y, m.albedo.z) == tuple(np.float32([0.9, 0.7, 0.5]).tolist())
    assert m.roughness == float(np.float32(0.3))
    for r in (0.03, 1.0):                                       # the ends of the range are inside it
        assert _scene(roughness=r).to_desc().materials[1].roughness == float(np.float32(r))


@pytest.mark.parametrize("kw,word", [(dict(roughness=0.02), "roughness"), (dict(roughness=1.5), "roughness"),
                                     (dict(roughness=float("nan")), "roughness"), (dict(albedo=(0.5, 1.2, 0.5)), "albedo"),
                                     (dict(albedo=(-0.1, 0.5, 0.5)), "albedo"), (dict(albedo=(0.5, 0.5, float("nan"))), "albedo")])
def test_range_errors(kw, word):
    with pytest.raises(ValueError) as e:
        _scene(**kw).to_desc()
    assert "material 1" in str(e.value) and "GgxMat" in str(e.value) and word in str(e.value)


def test_yaml_round_trip(tmp_path):
    scene = _scene()
    p = tmp_path / "ggx.yml"
    yaml_io.save_scene(scene, str(p))
    y = yaml.safe_load(p.read_text())
    assert y["materials"][1] == {"material": "GgxMat", "albedo": {"x": float(np.float32(0.9)), "y": float(np.float32(0.7)), "z": 0.5},
                                 "roughness": 0.3}
    back = yaml_io.load_scene(str(p))
    assert isinstance(back.materials[1], GgxMat) and not isinstance(back.materials[1], MetalMat)
    assert bytes(back.to_desc().materials[1]) == bytes(scene.to_desc().materials[1])
    p2 = tmp_path / "again.yml"
    yaml_io.save_scene(back, str(p2))
    assert p2.read_bytes() == p.read_bytes()


def test_yaml_without_the_material_is_unchanged(tmp_path):
    """Scenes that do not hold the material are written as before: the same dict through the same dumper, and the committed example of
    §9l loads and dumps to the bytes it has"""
    scene, _ = scenes.cornell_box()
    d = yaml_io.scene_to_dict(scene)
    assert all(m["material"] != "GgxMat" for m in d["materials"])
    p = tmp_path / "plain.yml"
    yaml_io.save_scene(scene, str(p))
    assert p.read_text() == yaml.safe_dump(d, sort_keys=False, default_flow_style=False)
    old = os.path.join(ROOT, "scenes", "three_lights.yml")
    p3 = tmp_path / "three.yml"
    yaml_io.save_scene(yaml_io.load_scene(old), str(p3))
    assert p3.read_bytes() == open(old, "rb").read()


def test_example_scene_loads():
    """scenes/ggx_lights.yml, the README's example: GgxMat spheres of several roughnesses on a Lambertian floor under one light of each
    kind, in front of the command line's fixed camera"""
    path = os.path.join(ROOT, "scenes", "ggx_lights.yml")
    scene = yaml_io.load_scene(path)
    ggx = [m for m in scene.materials if isinstance(m, GgxMat)]
    assert len(ggx) >= 3 and len({m.roughness for m in ggx}) == len(ggx)
    assert isinstance(scene.materials[0], LambertianMat)
    assert sorted(type(l).__name__ for l in scene.lights) == ["DirectionalLight", "PointLight", "SpotLight"]
    desc = scene.to_desc()                                      # (the ranges hold)
    assert sum(m.kind == A.FW_MAT_GGX for m in desc.materials) == len(ggx)
    assert yaml.safe_load(open(path).read()) == yaml_io.scene_to_dict(scene)
    for ro in scene.render_objects[1:]:
        assert np.abs(ro._position).max() <= 40
    assert "scenes/ggx_lights.yml" in open(os.path.join(ROOT, "README.md")).read()
