"""FUSE_SEGMENTS (DESIGN.md §5 "Fused segments"): a box-list batch's eleven (extend, shade) pairs as one launch of k_segments_boxlist.

The fused kernel runs the text of k_extend_linear_defer and k_shade<1,1,*> in a loop over a wave's own queue, so a fused frame is the unfused
frame bit for bit: every case renders FUSE_SEGMENTS=1 and FUSE_SEGMENTS=0 in one process and compares rgb8, gamma and linear as bytes and the
ray and sample counts as integers.  The launch log (_lib.last_kernels) says which path a call took: a fused call names k_segments_boxlist<...>
beside the two kernels whose text it ran, an unfused call does not.  Frames that are not eligible keep their launches under either setting."""
import copy

import numpy as np
import pytest

from firework_amd import _lib, scenes
from firework_amd.api import Cone, LambertianMat, RenderObject, TriangleMesh

pytestmark = pytest.mark.gpu

W = H = 48
FUSED = "k_segments_boxlist<"


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cornell(boxes=2, cone=False, mesh=False):
    """cornell_box with `boxes` of its two trailing boxes; `cone`: a cone ahead of them (no longer the SIMPLE set, the boxes still listed);
    `mesh`: a triangle ahead of them (a mesh anywhere takes the scene off the box lists)"""
    sc, r = scenes.cornell_box()
    tail = sc.render_objects[-2:]
    del sc.render_objects[-2:]
    if cone:
        sc.add_object(RenderObject.new(Cone.new(60.0, 120.0, 1)).position(420.0, 0.0, 120.0))
    if mesh:
        m = sc.add_material(LambertianMat.with_color((0.3, 0.6, 0.4)))
        verts = np.array([[100.0, 10.0, 100.0], [300.0, 10.0, 120.0], [180.0, 200.0, 300.0]], np.float32)
        sc.add_object(RenderObject.new(TriangleMesh.new(verts, np.array([[0, 1, 2]], np.uint32), None, None, m)))
    sc.render_objects += tail[2 - boxes:]
    return sc, r.width(W).height(H).samples(8).use_bvh(False).seed(11)


def _render(ds, r, fuse, pixel_ids=None, **opts):
    with _lib.options(FUSE_SEGMENTS=str(fuse), **opts):
        frame = ds.render(r, pixel_ids=pixel_ids)
        return frame, _lib.last_kernels()


def _fused(ran):
    return sorted(k for k in ran if k.startswith(FUSED))


def _same(a, b, what):
    assert np.array_equal(a.rgb8, b.rgb8), (what, int((a.rgb8 != b.rgb8).sum()))
    assert np.array_equal(_u32(a.gamma), _u32(b.gamma)), what
    assert np.array_equal(_u32(a.linear), _u32(b.linear)), what
    assert int(a.stats["rays"]) == int(b.stats["rays"]) and int(a.stats["samples"]) == int(b.stats["samples"]), what
    assert [int(x) for x in a.stats["rays_per_depth"]] == [int(x) for x in b.stats["rays_per_depth"]], what


def _pair(sc, r, want, what, pixel_ids=None, **opts):
    """the frame under FUSE_SEGMENTS=1 (which must name the fused instantiation `want`) against FUSE_SEGMENTS=0 (which must name none)"""
    ds = _lib.DeviceScene(sc.to_desc())
    try:
        off, ran_off = _render(ds, r, 0, pixel_ids, **opts)
        on, ran_on = _render(ds, r, 1, pixel_ids, **opts)
    finally:
        ds.close()
    assert _fused(ran_off) == [], (what, sorted(ran_off))
    assert _fused(ran_on) == [want], (what, sorted(ran_on))
    # a fused call also names the kernels whose text it ran: the unfused call's set
    assert ran_on - set(_fused(ran_on)) == ran_off, (what, sorted(ran_on), sorted(ran_off))
    assert int(on.stats["n_extend_launches"]) == int(off.stats["n_extend_launches"]), what
    assert int(on.stats["n_shade_launches"]) == int(off.stats["n_shade_launches"]), what
    _same(on, off, what)
    return on


def test_one_batch():
    """48 x 48 @8: 18 432 paths, queues of several chunks with a partial last chunk, both boxes"""
    sc, r = cornell()
    on = _pair(sc, r, "k_segments_boxlist<true,chain>", "one batch", STREAMS="1")
    assert int(on.stats["n_batches"]) == 1 and int(on.stats["rays"]) > int(on.stats["samples"])


def test_three_batches_two_lanes():
    sc, r = cornell()
    r = r.samples(64).paths_per_batch(W * H * 16)
    on = _pair(sc, r, "k_segments_boxlist<true,chain>", "batches", STREAMS="2")
    assert int(on.stats["n_batches"]) >= 3


def test_one_trailing_box():
    sc, r = cornell(boxes=1)
    _pair(sc, r, "k_segments_boxlist<true,chain>", "one box")


@pytest.mark.parametrize("opts,want", [({}, "k_segments_boxlist<false,chain>"), (dict(NO_CHAIN="1"), "k_segments_boxlist<false,no chain>")])
def test_not_the_simple_set(opts, want):
    """with the cases above, every instantiation of the fused kernel runs once"""
    sc, r = cornell(cone=True)
    _pair(sc, r, want, "cone ahead of the boxes", **opts)


def test_pixel_subset():
    """100 scattered pixels @8 in two batches of 400 paths: k_raygen deals chunks of 64 paths to the 8 queues, so six hold 64 paths, one holds
    16 and one is empty from segment 0 on"""
    sc, r = cornell()
    ids = np.sort(np.random.default_rng(5).choice(W * H, 100, replace=False)).astype(np.uint32)
    _pair(sc, r, "k_segments_boxlist<true,chain>", "pixel subset", pixel_ids=ids)


def test_pixel_subset_leaves_queues_empty():
    """5 pixels @8 are two batches of 20 paths: less than one chunk of 64, and k_raygen deals whole chunks, so queue 0 holds all of them and
    the other seven of the 8 queues have n == 0 from segment 0 on; the counters they write are zeros (rays_per_depth sums them)"""
    sc, r = cornell()
    _pair(sc, r, "k_segments_boxlist<true,chain>", "five pixels", pixel_ids=np.array([7, 500, 1001, 1500, 2303], np.uint32))


@pytest.mark.parametrize("opt,want", [("NO_HIT4", "k_segments_boxlist<true,chain>"), ("NO_CHAIN", "k_segments_boxlist<true,no chain>")])
def test_state_and_hit_record_variants(opt, want):
    """8-byte hit records; the 16-byte path state"""
    sc, r = cornell()
    _pair(sc, r, want, opt, **{opt: "1"})


def _falls_back(sc, r, what, must_run):
    ds = _lib.DeviceScene(sc.to_desc())
    try:
        off, ran_off = _render(ds, r, 0)
        on, ran_on = _render(ds, r, 1)
    finally:
        ds.close()
    assert _fused(ran_on) == [] and ran_on == ran_off, (what, sorted(ran_on))
    assert must_run in ran_on, (what, sorted(ran_on))
    _same(on, off, what)


def test_light_sampling_falls_back():
    sc, r = cornell()
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    _falls_back(sc, rr.light_sampling(True), "light sampling", "k_shade_ls<1,1>")


def test_mesh_falls_back():
    sc, r = cornell(mesh=True)
    _falls_back(sc, r, "mesh under the linear scan", "k_extend_linear")


def test_timing_falls_back():
    """per-launch timing wants the launches apart: ms_extend and ms_shade mean what they meant"""
    sc, r = cornell()
    rr = copy.copy(r)
    rr.settings = dict(r.settings)
    _falls_back(sc, rr.time_kernels(True), "FW_FLAG_TIME_KERNELS", "k_extend_linear_defer<true>")


def test_default_is_unfused():
    """FUSE_SEGMENTS unset: off (the fused frame did not clear the project's bar over the unfused launches: DESIGN.md §8)"""
    sc, r = cornell()
    ds = _lib.DeviceScene(sc.to_desc())
    try:
        frame = ds.render(r)
        ran = _lib.last_kernels()
        on, _ = _render(ds, r, 1)
    finally:
        ds.close()
    assert _fused(ran) == [] and "k_extend_linear_defer<true>" in ran, sorted(ran)
    _same(frame, on, "default, small frame")


def test_benchmark_frame():
    """The benchmark's frame (512 x 512 @1024: two batches of 2^21 chunks), where the queue counts change: unfused by default on twice the
    queues, fused under FUSE_SEGMENTS=1 on four times, the same frame bit for bit"""
    sc, r = scenes.config("C2_cornell_box", 512, 512, 1024)
    ds = _lib.DeviceScene(sc.to_desc())
    try:
        frame = ds.render(r)
        ran = _lib.last_kernels()
        on, ran_on = _render(ds, r, 1)
    finally:
        ds.close()
    assert _fused(ran) == [] and "k_extend_linear_defer<true>" in ran, sorted(ran)
    assert _fused(ran_on) == ["k_segments_boxlist<true,chain>"], sorted(ran_on)
    _same(frame, on, "the benchmark's frame")
