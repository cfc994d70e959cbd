"""What each _lib wrapper hands to its C entry point for host (numpy) arrays: the bound C function is replaced by a recorder that returns
FW_OK, and the recorded argument tuple is compared with the caller's arrays — scalars, structs passed by reference, (0, None) as
on_device and stream, every input pointer the caller's own (no copy of a contiguous float32 array), every in-place pointer the caller's
own object, every output pointer the returned array's, None for each optional array left out.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib
from firework_amd.api import (AmbientOcclusion, CameraModel, CameraSettings, DirectLight, GgxTable, Lightmap, PointLight, ProbeDepth, ProbeRadiance,
                              ProbeRelocation, ProbeSet, SunSky, TriangleMesh)

F = np.float32
N, W, H, D, R = 4, 2, 2, 2, 4
PROBES = ProbeSet.grid((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2, 1, 1), directions=D)
DEPTH, RADIANCE = ProbeDepth(R), ProbeRadiance(R)
M = int(RADIANCE.texels)


def arr(*shape, dtype=F):
    return np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape).astype(dtype)


SH, POS, NRM, AOV, SPEC, VIEW = arr(2, 9, 3), arr(N, 3), arr(N, 3) + 1, arr(N, 12), arr(N, 4), arr(N, 3) + 2
MOMENTS, PLACEMENT, MAPS, TABLE = arr(2, R, R, 2), arr(2, 4), arr(2, M, 4), arr(2, 2, 2)
RAYS, ACCUM, HITS = arr(2 * D, 6), arr(2 * D, 4), np.zeros(2 * D, _lib.HIT_DTYPE)


def P(a):
    return None if a is None else a.ctypes.data


class Recorder:
    """stands in for a bound C function: keeps each call's arguments and, for peek = {argument index: bytes}, what those pointers held"""

    def __init__(self, peek=None):
        self.calls, self.peek, self.peeked = [], peek or {}, {}

    def __call__(self, *args):
        self.calls.append(args)
        for i, nbytes in self.peek.items():
            self.peeked[i] = C.string_at(args[i], nbytes)
        return A.FW_OK

    @property
    def args(self):
        assert len(self.calls) == 1, len(self.calls)
        return self.calls[0]


@pytest.fixture
def record(monkeypatch):
    lib = _lib.load()

    def patch(name, peek=None):
        assert hasattr(lib, name), name
        r = Recorder(peek)
        monkeypatch.setattr(lib, name, r)
        return r
    return patch


def S(a):
    """the struct behind a byref argument"""
    return a._obj


def host_tail(args):
    assert args[-2:] == (0, None), args[-2:]


def host_params(p):
    assert p.on_device == 0 and p.stream is None


def is_grid(a):
    g = S(a)
    assert list(g.counts) == [2, 1, 1] and list(g.lo) == [0.0, 0.0, 0.0] and list(g.hi) == [1.0, 0.0, 0.0] and g.flags == A.FW_PROBE_WRAP


def is_depth(a):
    assert S(a).resolution == R and bytes(S(a)) == bytes(DEPTH.to_abi())


def is_radiance(a):
    assert bytes(S(a)) == bytes(RADIANCE.to_abi())


# ---------------------------------------------------------------------------------------------------------------- the probe lookups
@pytest.mark.parametrize("form", ["plain", "vis", "placed", "placed_vis"])
def test_probe_irradiance(record, form):
    entry = {"plain": "fw_probe_irradiance", "vis": "fw_probe_irradiance_vis"}.get(form, "fw_probe_irradiance_placed")
    rec = record(entry)
    if form == "plain":
        out = _lib.probe_irradiance(PROBES, SH, POS, NRM, device=1)
    elif form == "vis":
        out = _lib.probe_irradiance_vis(PROBES, SH, DEPTH, MOMENTS, POS, NRM, normal_bias=0.25, device=1)
    elif form == "placed":
        out = _lib.probe_irradiance_placed(PROBES, SH, PLACEMENT, POS, NRM, device=1)
    else:
        out = _lib.probe_irradiance_placed(PROBES, SH, PLACEMENT, POS, NRM, DEPTH, MOMENTS, 0.25, device=1)
    a = rec.args
    is_grid(a[0])
    assert a[1] == P(SH)
    if form == "vis":
        is_depth(a[2])
        assert a[3:5] == (P(MOMENTS), 0.25)
        tail = a[5:]
    elif form == "placed":
        assert a[2:6] == (None, None, 0.0, P(PLACEMENT))
        tail = a[6:]
    elif form == "placed_vis":
        is_depth(a[2])
        assert a[3:6] == (P(MOMENTS), 0.25, P(PLACEMENT))
        tail = a[6:]
    else:
        tail = a[2:]
    assert isinstance(out, np.ndarray) and out.shape == (N, 3) and out.dtype == F
    assert tail == (1, N, P(POS), P(NRM), 3, P(out), 0, None)


def test_probe_irradiance_fills_the_callers_out_and_reads_columns_of_records(record):
    rec = record("fw_probe_irradiance")
    mine = np.zeros((N, 3), F)
    assert _lib.probe_irradiance(PROBES, SH, POS, NRM, out=mine) is mine
    assert rec.args[2:] == (0, N, P(POS), P(NRM), 3, P(mine), 0, None)
    with pytest.raises(ValueError):
        _lib.probe_irradiance(PROBES, SH, POS, NRM, out=np.zeros((N, 3), np.float64))
    with pytest.raises(ValueError):
        _lib.probe_irradiance(PROBES, SH, POS, NRM, out=np.zeros((N + 1, 3), F))


def shade_call(form, **kw):
    if form == "plain":
        return _lib.probe_shade(PROBES, SH, AOV, W, H, gamma=2.0, device=1, **kw)
    if form == "vis":
        return _lib.probe_shade_vis(PROBES, SH, DEPTH, MOMENTS, AOV, W, H, normal_bias=0.25, gamma=2.0, device=1, **kw)
    if form == "placed":
        return _lib.probe_shade_placed(PROBES, SH, PLACEMENT, AOV, W, H, gamma=2.0, device=1, **kw)
    if form == "placed_vis":
        return _lib.probe_shade_placed(PROBES, SH, PLACEMENT, AOV, W, H, DEPTH, MOMENTS, 0.25, gamma=2.0, device=1, **kw)
    if form == "glossy":
        return _lib.probe_shade_glossy(PROBES, SH, RADIANCE, MAPS, AOV, SPEC, VIEW, W, H, gamma=2.0, device=1, **kw)
    if form == "glossy_all":
        return _lib.probe_shade_glossy(PROBES, SH, RADIANCE, MAPS, AOV, SPEC, VIEW, W, H, DEPTH, MOMENTS, 0.25, PLACEMENT, gamma=2.0, device=1, **kw)
    if form == "split":
        return _lib.probe_shade_split(PROBES, SH, RADIANCE, MAPS, AOV, SPEC, VIEW, TABLE, W, H, flags=A.FW_SPLIT_ENERGY, gamma=2.0, device=1, **kw)
    return _lib.probe_shade_split(PROBES, SH, RADIANCE, MAPS, AOV, SPEC, VIEW, TABLE, W, H, 0, DEPTH, MOMENTS, 0.25, PLACEMENT, gamma=2.0, device=1, **kw)


SHADE_ENTRY = dict(plain="fw_probe_shade", vis="fw_probe_shade_vis", placed="fw_probe_shade_placed", placed_vis="fw_probe_shade_placed",
                   glossy="fw_probe_shade_glossy", glossy_all="fw_probe_shade_glossy", split="fw_probe_shade_split", split_all="fw_probe_shade_split")


@pytest.mark.parametrize("form", list(SHADE_ENTRY))
def test_probe_shade_family(record, form):
    rec = record(SHADE_ENTRY[form])
    rgb8, gam, lin = shade_call(form)
    a = rec.args
    is_grid(a[0])
    assert a[1] == P(SH)
    if form in ("plain", "vis", "placed", "placed_vis"):
        if form == "vis":
            is_depth(a[2])
            assert a[3:5] == (P(MOMENTS), 0.25)
            k = 5
        elif form == "placed":
            assert a[2:6] == (None, None, 0.0, P(PLACEMENT))
            k = 6
        elif form == "placed_vis":
            is_depth(a[2])
            assert a[3:6] == (P(MOMENTS), 0.25, P(PLACEMENT))
            k = 6
        else:
            k = 2
        p, rest = S(a[k]), a[k + 1:]
        assert rest == (P(AOV), P(lin), P(gam), P(rgb8))
    else:
        is_radiance(a[2])
        assert a[3] == P(MAPS)
        if form.endswith("_all"):
            is_depth(a[4])
            assert a[5:8] == (P(MOMENTS), 0.25, P(PLACEMENT))
        else:
            assert a[4:8] == (None, None, 0.0, None)
        p = S(a[8])
        assert a[9:13] == (P(AOV), P(SPEC), P(VIEW), 3)
        if form.startswith("split"):
            assert a[13:17] == (P(TABLE), 2, 2, A.FW_SPLIT_ENERGY if form == "split" else 0)
            assert a[17:] == (P(lin), P(gam), P(rgb8))
        else:
            assert a[13:] == (P(lin), P(gam), P(rgb8))
    assert (p.width, p.height, p.gamma, p.device) == (W, H, 2.0, 1)
    host_params(p)
    assert rgb8.shape == gam.shape == lin.shape == (N, 3) and rgb8.dtype == np.uint8 and gam.dtype == lin.dtype == F


@pytest.mark.parametrize("form", ["plain", "glossy", "split"])
def test_probe_shade_outputs_left_out_are_null(record, form):
    rec = record(SHADE_ENTRY[form])
    rgb8, gam, lin = shade_call(form, outputs=("linear",))
    assert rgb8 is None and gam is None and lin.shape == (N, 3)
    assert rec.args[-3:] == (P(lin), None, None)


def test_probe_radiance_lookup(record):
    rec = record("fw_probe_radiance_lookup")
    rough = arr(N)
    out = _lib.probe_radiance_lookup(PROBES, RADIANCE, MAPS, POS, NRM, VIEW, rough, device=1)
    a = rec.args
    is_grid(a[0])
    is_radiance(a[1])
    assert a[2:] == (P(MAPS), None, None, 0.0, None, 1, N, P(POS), P(NRM), 3, P(VIEW), P(rough), P(out), 0, None)
    rec.calls.clear()
    mine = np.zeros((N, 3), F)
    assert _lib.probe_radiance_lookup(PROBES, RADIANCE, MAPS, POS, NRM, VIEW, rough, DEPTH, MOMENTS, 0.5, PLACEMENT, out=mine) is mine
    a = rec.args
    is_depth(a[3])
    assert a[2] == P(MAPS) and a[4:] == (P(MOMENTS), 0.5, P(PLACEMENT), 0, N, P(POS), P(NRM), 3, P(VIEW), P(rough), P(mine), 0, None)
    with pytest.raises(ValueError, match="together"):
        _lib.probe_radiance_lookup(PROBES, RADIANCE, MAPS, POS, NRM, VIEW, rough, depth=DEPTH)


# ---------------------------------------------------------------------------------------------------------------- rays and reductions
def test_model_probe_and_lightmap_rays(record):
    rec = record("fw_model_rays")
    model = CameraModel.panorama((0.0, 0.0, 0.0), W, H).seed(5)
    rays = _lib.model_rays(model, first_sample=3, n_samples=2, device=1)
    a = rec.args
    assert bytes(S(a[0])) == bytes(model.to_abi()) and a[1:] == (1, 3, 2, P(rays), 0, None) and rays.shape == (2, W * H, 6)
    rec = record("fw_probe_rays")
    rays = _lib.probe_rays(PROBES, round=2, first_probe=1, device=1)
    a = rec.args
    assert S(a[0]).n_probes == 2 and S(a[0]).directions == D and a[1:] == (1, 2, 1, 1, P(rays), 0, None) and rays.shape == (D, 6)
    rec = record("fw_lightmap_rays")
    lm = _lightmap()
    rays = _lib.lightmap_rays(lm, round=2, first=1, n=3, device=1)
    a = rec.args
    assert (S(a[0]).width, S(a[0]).height, S(a[0]).directions) == (W, H, D) and a[1:] == (1, 2, 1, 3, P(rays), 0, None) and rays.shape == (3 * D, 6)


def test_probe_project(record):
    rec = record("fw_probe_project")
    sums = _lib.probe_project(RAYS, ACCUM, 7, D, device=1)
    assert rec.args == (1, 2, D, 7, P(RAYS), P(ACCUM), P(sums), 0, None)
    assert sums.shape == (2, 9, 3) and not sums.any()                                    # new sums are zeros
    rec.calls.clear()
    mine = np.ones((2, 9, 3), F)
    assert _lib.probe_project(RAYS, ACCUM, 7, D, sums=mine) is mine
    assert rec.args[6] == P(mine)


def test_probe_survey_and_relocate_step(record):
    rec = record("fw_probe_survey")
    out = _lib.probe_survey(RAYS, HITS, D, device=1)
    assert rec.args == (1, 2, D, P(RAYS), P(HITS), P(out), 0, None) and out.shape == (2, 3, 4)
    rec.calls.clear()
    mine = np.zeros((2, 3, 4), F)
    assert _lib.probe_survey(RAYS, HITS, D, out=mine) is mine and rec.args[5] == P(mine)
    with pytest.raises(ValueError, match="HIT_DTYPE"):
        _lib.probe_survey(RAYS, np.zeros((2 * D, 12), F), D)
    rec = record("fw_probe_relocate_step")
    rl = ProbeRelocation(0.1, 0.25, 0.4)
    survey, placement = arr(2, 3, 4), arr(2, 4)
    assert _lib.probe_relocate_step(rl, survey, placement, D, move=False, device=1) is placement
    a = rec.args
    assert bytes(S(a[1])) == bytes(rl.to_abi()) and (a[0],) + a[2:] == (1, 2, D, P(survey), P(placement), 0, 0, None)
    with pytest.raises(ValueError, match="placement"):
        _lib.probe_relocate_step(rl, survey, np.zeros((2, 4), np.float64), D)


def test_probe_depth_and_radiance_reduce_and_prefilter(record):
    rec = record("fw_probe_depth_reduce")
    sums = _lib.probe_depth_reduce(DEPTH, RAYS, HITS, D, device=1)
    a = rec.args
    is_depth(a[1])
    assert (a[0],) + a[2:] == (1, 2, D, P(RAYS), P(HITS), P(sums), 0, None) and sums.shape == (2, R, R, 4) and not sums.any()
    rec = record("fw_probe_radiance_reduce")
    mine = np.ones((2, R, R, 4), F)
    assert _lib.probe_radiance_reduce(RADIANCE, RAYS, ACCUM, 7, D, sums=mine, device=1) is mine
    a = rec.args
    is_radiance(a[1])
    assert (a[0],) + a[2:] == (1, 2, D, 7, P(RAYS), P(ACCUM), P(mine), 0, None)
    rec = record("fw_probe_radiance_prefilter")
    maps = _lib.probe_radiance_prefilter(RADIANCE, mine, device=1)
    a = rec.args
    is_radiance(a[1])
    assert (a[0],) + a[2:] == (1, 2, P(mine), P(maps), 0, None) and maps.shape == (2, M, 4)


def _lightmap():
    mesh = TriangleMesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([0, 1, 2], np.uint32), uvs=np.array([[0, 0], [1, 0], [0, 1]], F))
    return Lightmap(mesh, W, H, D)


def test_lightmap_texels_reduce_and_dilate(record):
    rec = record("fw_lightmap_texels")
    records, owner, count = _lib.lightmap_texels(_lightmap(), device=1)
    a = rec.args
    assert a[1:4] == (1, P(records), P(owner)) and S(a[4]).value == 0 == count
    host_tail(a)
    assert records.shape == (W * H, 8) and np.isnan(records).all() and owner.dtype == np.uint32 and not owner.any()
    rec = record("fw_lightmap_reduce")
    sums, ids = np.zeros((H, W, 4), F), np.array([3, 0], np.uint32)
    assert _lib.lightmap_reduce(ACCUM, 7, D, sums, ids, device=1) is sums
    assert rec.args == (1, 2, D, 7, P(ids), P(ACCUM), P(sums), W * H, 0, None)
    rec.calls.clear()
    flat = np.zeros((2, 4), F)
    _lib.lightmap_reduce(ACCUM, 7, D, flat)
    assert rec.args == (0, 2, D, 7, None, P(ACCUM), P(flat), 2, 0, None)
    with pytest.raises(ValueError, match="sums"):
        _lib.lightmap_reduce(ACCUM, 7, D, np.zeros((2, 4), np.float64))
    rec = record("fw_lightmap_dilate")
    assert _lib.lightmap_dilate(sums, 3, device=1) is sums
    assert rec.args == (1, W, H, 3, P(sums), 0, None)
    with pytest.raises(ValueError, match="image"):
        _lib.lightmap_dilate(np.zeros((H, W, 4), np.float64), 1)


def test_ao_rays_and_reduce(record):
    rec = record("fw_ao_rays")
    ao = AmbientOcclusion(1.0, D)
    ids = np.array([2, 0], np.uint32)
    rays = _lib.ao_rays(ao, POS, NRM, ids, round=3, device=1)
    a = rec.args
    assert bytes(S(a[0])) == bytes(ao.to_abi()) and a[1:] == (1, 3, 2, P(POS), P(NRM), 3, P(ids), P(rays), 0, None) and rays.shape == (2 * D, 6)
    rec.calls.clear()
    rays = _lib.ao_rays(ao, AOV[:, 8:11], AOV[:, 4:7])                                 # columns of one array of records: read in place
    assert rec.args[1:] == (0, 0, N, P(AOV) + 32, P(AOV) + 16, 12, None, P(rays), 0, None) and rays.shape == (N * D, 6)
    rec = record("fw_ao_reduce")
    sums = np.zeros((N, 4), F)
    assert _lib.ao_reduce(ao, RAYS, HITS, sums, ids, device=1) is sums
    a = rec.args
    assert bytes(S(a[1])) == bytes(ao.to_abi()) and (a[0],) + a[2:] == (1, 2, P(ids), P(RAYS), P(HITS), P(sums), 0, None)
    with pytest.raises(ValueError, match="id"):
        _lib.ao_reduce(ao, RAYS, HITS, sums, np.array([0, N], np.uint32))
    with pytest.raises(ValueError, match="sums"):
        _lib.ao_reduce(ao, RAYS, HITS, np.zeros((N, 4), np.float64))


LIGHTS = [PointLight((0.0, 1.0, 0.0), (1.0, 1.0, 1.0)), PointLight((0.0, 2.0, 0.0), (1.0, 1.0, 1.0))]


def test_direct_rays_and_reduce(record):
    rec = record("fw_direct_rays")
    d = DirectLight()
    rays = _lib.direct_rays(d, LIGHTS, POS, NRM, device=1)
    a = rec.args
    assert bytes(S(a[0])) == bytes(d.to_abi()) and bytes(a[1]) == bytes(_lib._light_array(LIGHTS)[0])
    assert a[2:] == (2, 1, N, P(POS), P(NRM), 3, None, None, 3, None, P(rays), 0, None) and rays.shape == (N * 2, 6)
    rec.calls.clear()
    big, ids = arr(N, 6), np.array([1, 3], np.uint32)
    rays = _lib.direct_rays(d, LIGHTS, POS, NRM, ids, view=big[:, 3:6], spec=SPEC)      # view: a column range of a ray buffer, read in place
    assert rec.args[2:] == (2, 0, 2, P(POS), P(NRM), 3, P(ids), P(big) + 12, 6, P(SPEC), P(rays), 0, None)
    rec = record("fw_direct_reduce")
    rays8, hits8, sums = arr(N * 2, 6), np.zeros(N * 2, _lib.HIT_DTYPE), np.zeros((N, 8), F)
    assert _lib.direct_reduce(d, LIGHTS, POS, NRM, rays8, hits8, sums, view=VIEW, spec=SPEC, device=1) is sums
    a = rec.args
    assert a[0] == 1 and bytes(S(a[1])) == bytes(d.to_abi())
    assert a[3:] == (2, N, P(POS), P(NRM), 3, None, P(VIEW), 3, P(SPEC), P(rays8), P(hits8), P(sums), 0, None)


def test_sky_map_and_radiance(record):
    rec = record("fw_sky_map")
    sky = SunSky(35.0, 60.0)
    rgb = _lib.sky_map(sky, 8, 4, device=1)
    a = rec.args
    assert bytes(S(a[0])) == bytes(sky.to_abi()) and a[1:] == (1, 8, 4, P(rgb), 0, None) and rgb.shape == (4, 8, 3)
    rec = record("fw_sky_radiance")
    rgb = _lib.sky_radiance(sky, VIEW, device=1)
    assert rec.args[1:] == (1, N, P(VIEW), 3, P(rgb), 0, None) and rgb.shape == (N, 3)
    rec.calls.clear()
    rays = arr(N, 6)
    rgb = _lib.sky_radiance(sky, rays[:, 3:])                                           # read in place
    assert rec.args[1:] == (0, N, P(rays) + 12, 6, P(rgb), 0, None)


def test_ggx_terms_table_and_lookup(record):
    rec = record("fw_ggx_terms")
    mu, rho = arr(3), arr(3) + 1
    out = _lib.ggx_terms((8, 4), mu, rho, device=1)
    a = rec.args
    assert (S(a[0]).m1, S(a[0]).m2) == (8, 4) and a[1:] == (1, 3, P(mu), P(rho), P(out), 0, None) and out.shape == (3, 2)
    mine = np.zeros((3, 2), F)
    rec.calls.clear()
    assert _lib.ggx_terms((8, 4), mu, rho, out=mine) is mine and rec.args[5] == P(mine)
    with pytest.raises(ValueError, match="out"):
        _lib.ggx_terms((8, 4), mu, rho, out=np.zeros((3, 2), np.float64))
    rec = record("fw_ggx_table")
    table = _lib.ggx_table(GgxTable(2, 3, 8, 4), device=1)
    a = rec.args
    assert (S(a[0]).m1, S(a[0]).m2) == (8, 4) and a[1:] == (1, 2, 3, P(table), 0, None) and table.shape == (3, 2, 2)
    rec = record("fw_ggx_table_lookup")
    out = _lib.ggx_table_lookup(table, mu, rho, device=1)
    assert rec.args == (1, 2, 3, P(table), 3, P(mu), P(rho), P(out), 0, None) and out.shape == (3, 2)


def test_denoise_and_temporal(record):
    rec = record("fw_denoise")
    color, mom = arr(N, 3), arr(N, 4)
    rgb8, gam, lin = _lib.denoise(color, AOV, mom, W, H, iterations=3, gamma=2.0, device=1)
    a = rec.args
    p = S(a[0])
    assert (p.width, p.height, p.iterations, p.gamma, p.device) == (W, H, 3, 2.0, 1)
    host_params(p)
    assert a[1:] == (P(color), P(AOV), P(mom), P(lin), P(gam), P(rgb8)) and rgb8.dtype == np.uint8
    rec.calls.clear()
    rgb8, gam, lin = _lib.denoise(color, AOV, None, W, H)
    assert rec.args[1:] == (P(color), P(AOV), None, P(lin), P(gam), P(rgb8))
    rec = record("fw_temporal")
    cam = CameraSettings.default()
    hist = (arr(N, 3), arr(N, 4), arr(N, 12))
    prev = arr(N, 3)
    oc, om, oh = _lib.temporal(color, AOV, mom, hist, prev, W, H, cam, samples=5, max_history=8.0, device=1)
    a = rec.args
    p = S(a[0])
    assert (p.width, p.height, p.samples, p.max_history, p.device) == (W, H, 5, 8.0, 1) and bytes(p.camera) == bytes(cam.to_abi()) == bytes(p.prev_camera)
    host_params(p)
    assert a[1:] == (P(color), P(mom), P(AOV), P(hist[0]), P(hist[1]), P(hist[2]), P(prev), P(oc), P(om), P(oh))
    assert (oc.shape, om.shape, oh.shape) == ((N, 3), (N, 4), (N,))
    rec.calls.clear()
    oc, om, oh = _lib.temporal(color, AOV, width=W, height=H, camera=cam)
    assert rec.args[1:] == (P(color), None, P(AOV), None, None, None, None, P(oc), P(om), P(oh))


# ---------------------------------------------------------------------------------------------------------------- DeviceScene
def _scene(lib):
    scene = _lib.DeviceScene.__new__(_lib.DeviceScene)                                  # no device, no handle: nothing to destroy
    scene._lib, scene.handle, scene.device = lib, None, 1
    return scene


def test_scene_bakers(record):
    scene = _scene(_lib.load())
    rec = record("fw_bake_probes")
    sh, sums, stats = scene.bake_probes(PROBES, 3, 5, seed=9, chunk=1)
    a = rec.args
    p = S(a[2])
    assert a[0] is None and S(a[1]).n_probes == 2 and S(a[1]).chunk_probes == 1 and (p.samples, p.seed, p.use_bvh, p.gamma) == (5, 9, 1, 1.0)
    host_params(p)
    assert a[3:7] == (0, 3, P(sums), P(sh)) and sh.shape == sums.shape == (2, 9, 3) and not sums.any() and isinstance(stats, dict)
    rec.calls.clear()
    mine = np.ones((2, 9, 3), F)
    assert scene.bake_probes(PROBES, 1, 5, first_round=3, sums=mine)[1] is mine and rec.args[3:6] == (3, 1, P(mine))
    with pytest.raises(ValueError, match="sums"):
        scene.bake_probes(PROBES, 1, 5, sums=np.ones((2, 9, 3), np.float64))
    rec = record("fw_bake_lightmap")
    irr, sums, _ = scene.bake_lightmap(_lightmap(), 3, 5, dilate=4)
    a = rec.args
    host_params(S(a[2]))
    assert a[3:8] == (0, 3, 4, P(sums), P(irr)) and irr.shape == sums.shape == (H, W, 4)
    rec = record("fw_bake_probe_depth")
    mom, sums, _ = scene.bake_probe_depth(PROBES, DEPTH, rounds=2, seed=9, rays_per_batch=64)
    a = rec.args
    is_depth(a[2])
    p = S(a[3])
    assert (p.use_bvh, p.flags, p.seed, p.rays_per_batch) == (1, 0, 9, 64)
    host_params(p)
    assert a[4:8] == (0, 2, P(sums), P(mom)) and mom.shape == (2, R, R, 2) and sums.shape == (2, R, R, 4) and not sums.any()
    rec = record("fw_bake_probe_radiance")
    maps, sums, _ = scene.bake_probe_radiance(PROBES, RADIANCE, 2, 5)
    a = rec.args
    is_radiance(a[2])
    host_params(S(a[3]))
    assert a[4:10] == (0, 2, P(sums), P(maps), None, None) and maps.shape == (2, M, 4) and sums.shape == (2, R, R, 4)
    rec.calls.clear()
    mine = np.ones((2, 9, 3), F)
    maps, sums, sh, sh_sums, _ = scene.bake_probe_radiance(PROBES, RADIANCE, 2, 5, sh_sums=mine)
    assert sh_sums is mine and rec.args[4:10] == (0, 2, P(sums), P(maps), P(mine), P(sh)) and sh.shape == (2, 9, 3)
    rec = record("fw_relocate_probes")
    rl = ProbeRelocation(0.1, 0.25, 0.4, steps=3)
    placement, survey, _ = scene.relocate_probes(PROBES, rl)
    a = rec.args
    assert a[4:8] == (0, 3, P(placement), P(survey)) and placement.tolist() == [[0, 0, 0, 1]] * 2 and survey.shape == (2, 3, 4)


def test_scene_ao_and_direct(record):
    scene = _scene(_lib.load())
    rec = record("fw_bake_ao")
    ao = AmbientOcclusion(1.0, D)
    ids = np.array([2, 0], np.uint32)
    out, sums, _ = scene.bake_ao(ao, POS, NRM, ids, rounds=2, chunk=1)
    a = rec.args
    assert a[0] is None and S(a[1]).chunk_points == 1 and S(a[1]).directions == D
    host_params(S(a[2]))
    assert a[3:12] == (2, P(POS), P(NRM), 3, P(ids), 0, 2, P(sums), P(out)) and out.shape == sums.shape == (N, 4) and not sums.any() and not out.any()
    rec.calls.clear()
    mine, mine_out = np.ones((H, W, 4), F), np.ones((H, W, 4), F)
    o, s, _ = scene.bake_ao(ao, POS, NRM, first_round=2, sums=mine, out=mine_out)
    assert o is mine_out and s is mine and rec.args[3:12] == (N, P(POS), P(NRM), 3, None, 2, 1, P(mine), P(mine_out))
    with pytest.raises(ValueError, match="sums"):
        scene.bake_ao(ao, POS, NRM, sums=np.ones((N, 4), np.float64))
    rec = record("fw_bake_direct")
    d = DirectLight()
    out, sums, _ = scene.bake_direct(d, POS, NRM, view=VIEW, spec=SPEC, rounds=2)
    a = rec.args
    host_params(S(a[2]))
    assert a[3:15] == (N, P(POS), P(NRM), 3, None, P(VIEW), 3, P(SPEC), 0, 2, P(sums), P(out)) and out.shape == sums.shape == (N, 8)


def test_scene_render_rays_render_model_and_trace(record):
    scene = _scene(_lib.load())
    rec = record("fw_render_rays")
    rays, keys = arr(3, N, 6), np.arange(N, dtype=np.uint32)
    res = scene.render_rays(rays, 3, keys=keys, seed=9, gamma=2.0)
    a = rec.args
    p = S(a[1])
    assert (p.n_rays, p.first_sample, p.samples, p.per_sample_rays, p.seed, p.gamma) == (N, 0, 3, 1, 9, 2.0)
    assert C.cast(p.keys, C.c_void_p).value == P(keys)
    host_params(p)
    assert a[0] is None and a[2:7] == (P(rays), P(res.accum), P(res.rgb8), P(res.gamma), P(res.linear)) and not res.accum.any()
    rec.calls.clear()
    mine = np.ones((N, 4), F)
    res = scene.render_rays(rays[0], 2, first_sample=3, accum=mine)
    p = S(rec.args[1])
    assert res.accum is mine and rec.args[2:4] == (P(rays), P(mine)) and (p.per_sample_rays, p.first_sample) == (0, 3) and not p.keys
    with pytest.raises(ValueError, match="accum"):
        scene.render_rays(rays[0], 2, accum=np.ones((N, 4), np.float64))
    rec = record("fw_render_model")
    model = CameraModel.panorama((0.0, 0.0, 0.0), W, H)
    res = scene.render_model(model, 3, chunk=2)
    a = rec.args
    p = S(a[2])
    assert S(a[1]).chunk_samples == 2 and (p.n_rays, p.samples, p.per_sample_rays) == (N, 3, 1)
    host_params(p)
    assert a[3:7] == (P(res.accum), P(res.rgb8), P(res.gamma), P(res.linear)) and res.accum.shape == (N, 4) and not res.accum.any()
    rec = record("fw_trace_rays")
    hits = scene.trace(RAYS, True, seed=9, key_base=5)
    a = rec.args
    p = S(a[1])
    assert (p.use_bvh, p.seed, p.key_base) == (1, 9, 5)
    host_params(p)
    assert a[2:5] == (P(RAYS), 2 * D, P(hits)) and hits.dtype == _lib.HIT_DTYPE and hits.shape == (2 * D,)


# ---------------------------------------------------------------------------------------------------------------- what is refused or copied
def test_a_non_contiguous_input_is_copied_once_and_the_call_sees_contiguous_data(record):
    wide = arr(2 * D, 12)
    rays = wide[:, ::2]
    rec = record("fw_probe_project", peek={4: rays.size * 4})
    _lib.probe_project(rays, ACCUM, 7, D)
    assert rec.args[4] not in (P(wide), P(rays)) and rec.args[5] == P(ACCUM)
    assert rec.peeked[4] == np.ascontiguousarray(rays).tobytes()
    rec = record("fw_probe_shade", peek={3: AOV.size * 4})
    _lib.probe_shade(PROBES, SH, AOV.astype(np.float64), W, H)                          # another dtype: converted once
    assert rec.peeked[3] == AOV.tobytes()


def test_a_cpu_torch_tensor_is_not_a_device_tensor(record):
    import torch
    rec = record("fw_probe_project")
    with pytest.raises(ValueError, match="must be a contiguous torch.float32 tensor of shape .* on cuda:0"):
        _lib.probe_project(torch.zeros((2 * D, 6)), torch.zeros((2 * D, 4)), 7, D)
    rec2 = record("fw_probe_shade")
    with pytest.raises(ValueError, match="on cuda:0"):
        _lib.probe_shade(PROBES, torch.zeros((2, 9, 3)), torch.zeros((N, 12)), W, H)
    rec3 = record("fw_lightmap_dilate")
    with pytest.raises(ValueError, match="on cuda:0"):
        _lib.lightmap_dilate(torch.zeros((H, W, 4)), 1)
    assert not rec.calls and not rec2.calls and not rec3.calls
