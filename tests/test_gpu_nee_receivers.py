"""Known-answer probes for light sampling at every kind of receiver (DESIGN.md §9g "Tests").  One receiver, one light, a black environment
unless the map is the light, 3-7 probe rays through fw_render_rays: every path is one bounce.  The receivers report normals that are not the
unit +y of a floor hit from above: a one-triangle mesh without vertex normals scaled to |n| = 0.05, 0.3, 1, 1.7 and 4 (with and without the
BVH, and one copy under OF_ROTATED), the triangle with interpolated vertex normals, a rotated XZRect, a sphere at three latitudes, an XZRect
hit from below and one with flip_normals, and a floor seen in a mirror MetalMat.  The lights: a rectangle and a sphere (bit 4), a two-triangle
quad and a box (bits 4 + 16), a map with one bright texel above the horizon and one below (bit 8, and bits 4 + 8 beside a rectangle), a point,
a spot and a directional light.  Tables, variances, sample counts and condition numbers come from tests/nee_receivers_ref.py alone and are
pinned by tests/test_nee_receivers_cpu.py.

Stochastic probes: the NEE estimator within 4 standard errors of the reference's MIS variance at N samples, N the power of two at which that
is at most 1 % of the answer (at most 2^18); the default estimator within 4 of its own standard errors of the same answer.  SEED was written
down before the first run and is never changed to pass: a comparison that fails is repeated once with 16 N samples and the same seed (a real
bias grows fourfold in sigma units, chance does not) and has to hold there.

Delta-light probes are deterministic: relative error <= kappa x B x 2^-24, kappa the reference's condition number of p_b (<= 16, pinned on
the CPU) and B = 96 the count of float32 roundings between the scene and the pixel, each entering p_b's inputs at most once:
    the hit point: ray_point or the barycentric sum (5), rot_fwd and the position (6)                                       11
    the normal: two edges (2), the cross product (3), rot_fwd with a float32 matrix (5 + 4); or interpolation (5) and
        normalisation (7) in their place                                                                                     14
    delta_sample: d (1), d . d (5), sqrt (1), w = d / |d| (1); the spot's cosine is clamped to s = 1 inside the inner cone    8
    scatter_pdf's inputs: c = n . w (5, counted twice: a dot product's error is relative to |n|, not to c, and kappa's term
        3 / (4 cos^2) in |n|^2 already grows as fast towards grazing incidence), |n|^2 (5), c^2, - |n|^2, + 1 (3)           18
    scatter_pdf after the root: sqrt, t+, t-, two cubes (4), their difference, 1 / 4 pi (each amplified by at most
        (t+^3 + t-^3) / (t+^3 - t-^3) <= kappa / 3)                                                                           9
    L = s / d^2 x I (3), beta x albedo (1), x L (1), p_b / p (3), x (1)                                                       9
    the mean of 16 equal samples and the resolve                                                                               3
    the reference's own float32 inputs (light position, vertices, matrix entries taken as float32 of the api's values)       24
The existing floor probes derive 1e-5 (fewer than 100 roundings) the same way.  Exact zeros — a light outside the cone sin(theta) > 1 / |n| of
a long normal, or behind a flipped floor — must come out as 0.0 from both estimators."""
import os
import sys

import numpy as np
import pytest

from firework_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nee_receivers_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20261
B = 96
U = 2.0 ** -24
DELTA_SAMPLES = 16


def _render(ds, rays, n, flags, bvh):
    return ds.render_rays(rays, n, seed=SEED, flags=flags, use_bvh=bvh).linear.astype(np.float64)


def _z(got, want, var, n):
    """|got - want| in standard errors, per probe and channel; exact zeros are compared apart"""
    se = np.sqrt(var / n)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(se > 0, np.abs(got - want) / se, 0.0)


def _stochastic(ds, t, flags, bvh, var, tag):
    """one estimator of one table: 4 standard errors, once more at 16 N where that fails; the answers that are exactly 0 are exactly 0.0"""
    pos = t.want > 0
    got = _render(ds, t.rays, t.N, flags, bvh)
    z = _z(got, t.want, var, t.N)
    print(f"{tag}: N = 2^{int(np.log2(t.N))}, max |z| {z[pos].max() if pos.any() else 0.0:.2f}, "
          f"max relative error {(np.abs(got - t.want)[pos] / t.want[pos]).max() if pos.any() else 0.0:.2e}")
    assert np.all(got[~pos] == 0.0), (tag, got[~pos])
    if pos.any() and z[pos].max() > 4.0:
        n16 = 16 * t.N
        got16 = _render(ds, t.rays, n16, flags, bvh)
        z16 = _z(got16, t.want, var, n16)
        print(f"{tag}: repeated at 16 N: max |z| {z16[pos].max():.2f} (was {z[pos].max():.2f})")
        assert z16[pos].max() <= 4.0, (tag, "N", z[pos].max(), "16 N", z16[pos].max(), got16, t.want)
    return z


def _deterministic(ds, t, bvh, tag):
    got = _render(ds, t.rays, DELTA_SAMPLES, t.flags, bvh)
    pos = t.want > 0
    assert np.all(got[~pos] == 0.0), (tag, got[~pos])
    if not pos.any():
        return 0.0
    bound = (t.kappa * B * U)[:, None] * np.ones(3)
    err = np.abs(got - t.want) / np.where(pos, t.want, 1.0)
    ratio = float((err / bound)[pos].max())
    print(f"{tag}: max relative error {err[pos].max():.3g}, max error / (kappa B 2^-24) = {ratio:.4f} (kappa up to {t.kappa.max():.1f})")
    assert np.all(err[pos] <= bound[pos]), (tag, err.max(), ratio)
    return ratio


def _check(recv, light, extras=(), tag=""):
    t = R.table(recv, light)
    ds = _lib.DeviceScene(R.build_scene(recv, light, extras).to_desc())
    for bvh in t.bvh:
        name = f"{recv} / {light}{tag}{'' if bvh else ' / no bvh'}"
        if t.stochastic:
            _stochastic(ds, t, t.flags, bvh, t.var_nee, name + " / nee")
            _stochastic(ds, t, 0, bvh, t.var_default, name + " / default")
        else:
            _deterministic(ds, t, bvh, name)


@pytest.mark.parametrize("recv,light", R.RECEIVER_LIGHTS, ids=[f"{r}-{l}" for r, l in R.RECEIVER_LIGHTS])
def test_probe(recv, light):
    _check(recv, light)


# ---- kernel coverage ----------------------------------------------------------------------------------------------------------------------
# The |n| = 0.3 and |n| = 1.7 mesh probes again where the frame takes other kernels: shading mode 0 (an expensive texture in the scene, as
# test_gpu_ggx.py::test_probes_in_shading_mode_0 forces it), the GX kernels (a GgxMat in the scene: they shade the Lambertian vertex too), and
# both.  The extra object is out of every path's reach (nee_receivers_ref.unreachable), so the answers and their bounds are unchanged.
@pytest.mark.parametrize("extras", [("checker",), ("ggx",), ("checker", "ggx")], ids=["mode0", "gx", "gx_mode0"])
@pytest.mark.parametrize("light", ["rect", "point"])
@pytest.mark.parametrize("recv", ["mesh_0.3", "mesh_1.7"])
def test_probe_under_other_kernels(recv, light, extras):
    _check(recv, light, extras, " / " + "+".join(extras))


# ---- the isotropic vertex -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", ["point", "sun"])
def test_isotropic_vertex(light):
    """Single scattering in a spherical medium of density 0.5 under a point and under a directional light outside it, along three chords:
    p_b = 1 / 4 pi, the free path by log10, the shadow ray's own draw as the transmittance (nee_receivers_ref.medium_answer).  The orders
    beyond the first are bounded in the reference by albedo^2 / (1 - albedo) x max L / 4 pi, under 2 % of the tolerance at albedo = 2^-14.

    The point light's case is the one that finds a shadow ray's start inside a medium: with the ray (x, light - x) begun at t_min = 0.001
    of its own length (before shade_path moved it back) the transmittance was high by 10^(0.001 rho |d|): got / want 1.0091, 1.0068, 1.0077 and
    |z| = 19.2 at 2^22 samples ("What the probes found", 2)."""
    t = R.medium_table(light)
    ds = _lib.DeviceScene(R.medium_scene(light).to_desc())
    got = _render(ds, t.rays, t.N, 0, True)
    z = _z(got, t.want, t.var_nee, t.N)
    print(f"isotropic / {light}: N = 2^{int(np.log2(t.N))}, max |z| {z.max():.2f}, max relative error {(np.abs(got - t.want) / t.want).max():.2e}")
    print(f"isotropic / {light}: got / want per chord {np.array2string((got / t.want)[:, 0], precision=5)}")
    if z.max() > 4.0:
        n16 = 16 * t.N
        z16 = _z(_render(ds, t.rays, n16, 0, True), t.want, t.var_nee, n16)
        print(f"isotropic / {light}: repeated at 16 N: max |z| {z16.max():.2f} (was {z.max():.2f})")
        assert z16.max() <= 4.0, (light, z.max(), z16.max())
