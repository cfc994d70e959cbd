"""The fw_stats of fw_bake_direct against the same work made by hand, one public call per chunk, in the pattern of
tests/test_gpu_bake_stats.py: every counter is the sum over the chunks' traces, the generator and the reducer add no bytes of their own,
the tree sizes and `reserved` are the last chunk's, and the two kernels' times are reported with FW_FLAG_TIME_KERNELS and zero without
it.  The shapes are the smallest with a chunk boundary and a ragged last chunk; the sums are compared bit for bit as well, so the hand-made
chunks are known to be the call's own."""
import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import DirectionalLight, DirectLight, PointLight, SpotLight

from test_gpu_bake_stats import POSITIONS, SCENES, _trace_chunk, _u32, _with, assert_trace_counters, assert_trace_times

pytestmark = pytest.mark.gpu

LIGHTS = {"conics": [PointLight((0.0, 8.0, 0.0), (60.0, 50.0, 40.0)), SpotLight((3.0, 6.0, 2.0), (-0.4, -1.0, -0.3), (90.0, 90.0, 90.0), 20.0, 50.0),
                     DirectionalLight((0.2, -1.0, 0.1), (2.0, 1.5, 1.0))],
          "C3_suzanne": [PointLight((0.0, 6.0, 4.0), (60.0, 50.0, 40.0)), SpotLight((3.0, 5.0, 5.0), (-0.4, -1.0, -0.6), (90.0, 90.0, 90.0), 20.0, 50.0),
                         DirectionalLight((0.2, -1.0, -0.3), (2.0, 1.5, 1.0))]}


@pytest.mark.parametrize("name,bvh", SCENES)
def test_bake_direct_stats_are_its_chunks(name, bvh):
    import torch
    N, ROUNDS, CHUNK = 5, 2, 2
    scene, r = scenes.config(name, 8, 8, 1)
    r = _with(r, use_bvh=bvh, seed=11)
    s = r.settings
    lights = LIGHTS[name]
    Ln = len(lights)
    pos = np.array(POSITIONS[name], np.float32)
    nrm = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (N, 1))            # up, towards each scene's lights
    nrm[2] = 0.0                                                            # no rays are generated for it: its chunk traces fewer
    ok = api.ao_usable(pos, nrm)
    assert ok.tolist() == [True, True, False, True, True]
    d = DirectLight(1e-3)
    ds = _lib.DeviceScene(scene.to_desc())
    try:
        ds.set_lights(lights)
        d_pos, d_nrm = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
        sums = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
        parts, live = [], []
        for rnd in range(ROUNDS):
            for q0 in range(0, N, CHUNK):
                k = min(CHUNK, N - q0)
                ids = torch.arange(q0, q0 + k, dtype=torch.int32, device="cuda")      # the points [q0, q0 + k) of the call
                rays = _lib.direct_rays(d, lights, d_pos, d_nrm, ids)
                live.append(int(torch.any(rays != 0, dim=1).sum()))
                hits = _trace_chunk(ds, r, rays, rnd, q0 * Ln, parts)
                _lib.direct_reduce(d, lights, d_pos, d_nrm, rays, hits, sums, ids)
        assert len(parts) == ROUNDS * 3 and N % CHUNK
        assert [p["rays"] for p in parts] == live and 0 < live[1] < live[0]      # zero rays are not traced: the point without a normal has none
        bake = dict(seed=s["seed"], use_bvh=s["use_bvh"], chunk=CHUNK)
        _, got, plain = ds.bake_direct(d, pos, nrm, None, None, None, ROUNDS, flags=s["flags"], **bake)
        assert np.array_equal(_u32(got), _u32(sums.cpu().numpy())) and np.all(got[2] == 0.0) and np.any(got[ok] != 0.0), name
        assert_trace_counters(plain, parts, name)
        _, got_t, timed = ds.bake_direct(d, pos, nrm, None, None, None, ROUNDS, flags=s["flags"] | A.FW_FLAG_TIME_KERNELS, **bake)
        assert np.array_equal(_u32(got_t), _u32(got)), name
        assert_trace_counters(timed, parts, name + " timed")
        assert_trace_times(plain, timed, name)
    finally:
        ds.close()
