"""CPU-side checks of the lightmap baker (fw_lightmap_texels, fw_lightmap_rays, fw_lightmap_reduce, fw_lightmap_dilate,
fw_bake_lightmap): the exports and fw_lightmap's layout at ABI 8, every argument error in the header's order (before the
scene is looked at or HIP is called), the no-device error with the caller's buffers left as they were, the CLI's refusals, and the numpy
statements (api.Lightmap.texels / .rays, api.lightmap_reduce, api.lightmap_dilate) against hand-made cases and closed forms within the
lattice's derived C / D bound (tests/lightmap_ref.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api, scenes
from firework_amd.api import Lightmap, RenderObject, Rotor3, TriangleMesh

import lightmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NO = api.LIGHTMAP_NO_OWNER


def test_exports_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    for name, args in (
            ("fw_lightmap_texels", r"const fw_lightmap \*lm, int device, float \*records, uint32_t \*owner, uint32_t \*n_covered, int on_device, "
                                   r"void \*stream"),
            ("fw_lightmap_rays", r"const fw_lightmap \*lm, int device, uint32_t round, uint32_t first, uint32_t n, float \*rays, int on_device, "
                                 r"void \*stream"),
            ("fw_lightmap_reduce", r"int device, uint32_t n, uint32_t directions, uint32_t samples, const uint32_t \*texel_ids, "
                                   r"const float \*accum, float \*sums, uint32_t n_texels, int on_device, void \*stream"),
            ("fw_lightmap_dilate", r"int device, uint32_t width, uint32_t height, uint32_t passes, float \*image, int on_device, void \*stream"),
            ("fw_bake_lightmap", r"fw_scene \*scene, const fw_lightmap \*lm, const fw_render_rays_params \*rp, uint32_t first_round, "
                                 r"uint32_t rounds, uint32_t dilate, float \*sums, float \*irradiance, fw_stats \*stats")):
        assert hasattr(lib, name), name
        assert re.search(rf"\bint {name}\s*\({args}\);", text), name


def test_lightmap_layout(tmp_path):
    """ctypes' fw_lightmap equals the C compiler's, size and every field offset"""
    names = [f for f, _ in A.fw_lightmap._fields_]
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu' + " %zu" * len(names) +
           '\\n",sizeof(fw_lightmap)' + "".join(f",offsetof(fw_lightmap,{f})" for f in names) + ');return 0;}')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out[0] == C.sizeof(A.fw_lightmap)
    assert out[1:] == [getattr(A.fw_lightmap, f).offset for f in names]
    assert names == ["verts", "n_verts", "indices", "n_indices", "normals", "uvs", "position", "rotation", "flip_normals", "width", "height",
                     "directions", "jitter", "seed", "bias", "flip", "chunk_texels"]


def _lm(verts=None, uvs=None, normals=None, indices=None, null=(), **kw):
    """a valid 8 x 8 lightmap of a quad with 16 directions, then arrays replaced, the pointers named in `null` cleared and fields
    overwritten; returns (struct, what it points into)"""
    base = R.lightmap("quad", 8, 8, normals=True, directions=16).seed(3)
    m = base.mesh
    mesh = TriangleMesh(m.verts if verts is None else verts, m.indicies if indices is None else indices, m.normals if normals is None else normals,
                        m.uvs if uvs is None else uvs, 0)
    s, keep = Lightmap(mesh, 8, 8, 16).seed(3).to_abi()
    for k in null:
        setattr(s, k, None)
    for k, v in kw.items():
        setattr(s, k, v)
    return s, keep


def _poke(a, idx, v):
    b = np.array(a, copy=True)
    b.reshape(-1)[idx] = v
    return b


def _bad_lightmaps():
    """(what, lightmap, the words fw_last_error() must hold) for every lightmap error of the header, in its order"""
    m = R.lightmap("quad", 8, 8, normals=True).mesh
    out = [("null verts", _lm(null=("verts",)), None), ("null indices", _lm(null=("indices",)), None),
           ("null uvs", _lm(null=("uvs",)), None), ("n_verts", _lm(n_verts=0), None), ("n_indices 0", _lm(n_indices=0), None),
           ("n_indices 4", _lm(n_indices=4), None), ("width 0", _lm(width=0), None), ("width", _lm(width=16385), None),
           ("height 0", _lm(height=0), None), ("height", _lm(height=16385), None), ("directions 0", _lm(directions=0), None),
           ("directions", _lm(directions=(1 << 20) + 1), None), ("bias < 0", _lm(bias=-1.0), None), ("bias nan", _lm(bias=NAN), None),
           ("position", _lm(position=A.fw_vec3(0.0, NAN, 0.0)), None), ("rotation", _lm(rotation=A.fw_rotor3(1.0, 0.0, INF, 0.0)), None),
           ("index", _lm(indices=_poke(m.indicies, 4, 4)), "index 4 "), ("vert", _lm(verts=_poke(m.verts, 7, NAN)), "vert 2 "),
           ("uv", _lm(uvs=_poke(m.uvs, 3, -INF)), "uv 1 "), ("normal", _lm(normals=_poke(m.normals, 11, INF)), "normal 3 ")]
    return out


def _big():
    """W H D = 2^31 under a mesh that covers the whole image: the size limit"""
    return _lm(uvs=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), width=16384, height=16384, directions=8)


def _rp(**kw):
    p = A.fw_render_rays_params()
    p.samples, p.use_bvh = 2, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_the_order_of_the_lightmap_errors_is_the_headers():
    """an earlier error wins over a later one: each bad lightmap, made worse in every later way, still fails — and with the detail string
    of its own error where it has one"""
    lib = _lib.load()
    bad = _bad_lightmaps()
    rec = np.full((64, 8), 7.0, np.float32)
    for what, s, words in bad:
        assert lib.fw_lightmap_texels(C.byref(s[0]), 0, rec.ctypes.data, None, None, 0, None) == A.FW_ERR_BAD_ARG, what
        if words:
            assert words in lib.fw_last_error().decode(), (what, lib.fw_last_error())
    # an index out of range is reported before a non-finite vert, a vert before a uv, a uv before a normal
    m = R.lightmap("quad", 8, 8, normals=True).mesh
    s = _lm(indices=_poke(m.indicies, 4, 9), verts=_poke(m.verts, 0, NAN), uvs=_poke(m.uvs, 0, NAN), normals=_poke(m.normals, 0, NAN))
    assert lib.fw_lightmap_texels(C.byref(s[0]), 0, None, None, None, 0, None) == A.FW_ERR_BAD_ARG and "index 4 " in lib.fw_last_error().decode()
    s = _lm(verts=_poke(m.verts, 4, NAN), uvs=_poke(m.uvs, 0, NAN), normals=_poke(m.normals, 0, NAN))
    assert lib.fw_lightmap_texels(C.byref(s[0]), 0, None, None, None, 0, None) == A.FW_ERR_BAD_ARG and "vert 1 " in lib.fw_last_error().decode()
    s = _lm(uvs=_poke(m.uvs, 4, NAN), normals=_poke(m.normals, 0, NAN))
    assert lib.fw_lightmap_texels(C.byref(s[0]), 0, None, None, None, 0, None) == A.FW_ERR_BAD_ARG and "uv 2 " in lib.fw_last_error().decode()
    assert np.all(rec == 7.0)


def test_lightmap_texels_argument_checks():
    lib = _lib.load()
    rec = np.full((64, 8), 7.0, np.float32)
    own = np.full(64, 7, np.uint32)
    cnt = C.c_uint32(77)

    def call(s, r=rec, o=own, on_device=0, ptrs=None):
        pr, po = ptrs if ptrs else (None if r is None else r.ctypes.data, None if o is None else o.ctypes.data)
        return lib.fw_lightmap_texels(None if s is None else C.byref(s[0]), 0, pr, po, C.byref(cnt), on_device, None)

    assert call(None) == A.FW_ERR_BAD_ARG
    for what, s, _ in _bad_lightmaps():
        assert call(s) == A.FW_ERR_BAD_ARG, what
    assert rec.ctypes.data % 16 == 0
    assert call(_lm(), on_device=1, ptrs=(C.c_void_p(rec.ctypes.data + 4), C.c_void_p(own.ctypes.data))) == A.FW_ERR_BAD_ARG
    assert call(_lm(), on_device=1, ptrs=(C.c_void_p(rec.ctypes.data), C.c_void_p(own.ctypes.data + 2))) == A.FW_ERR_BAD_ARG
    # the order: bad arguments before the size limit, the size limit before the device
    assert call(_big(), on_device=1, ptrs=(C.c_void_p(rec.ctypes.data + 4), None)) == A.FW_ERR_BAD_ARG
    assert call(_big()) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call(_lm()) == A.FW_ERR_NO_DEVICE
        assert call(_lm(), r=None, o=None) == A.FW_ERR_NO_DEVICE                          # either array may be NULL
        # the limit counts covered texels, not the image: the same size under a mesh that covers a corner passes it
        small = np.array([[0, 0], [0.01, 0], [0.01, 0.01], [0, 0.01]], np.float32)
        assert call(_lm(uvs=small, width=16384, height=16384, directions=8)) == A.FW_ERR_NO_DEVICE
        assert np.all(rec == 7.0) and np.all(own == 7) and cnt.value == 77               # the caller's buffers are as they were


def test_lightmap_rays_argument_checks():
    lib = _lib.load()
    rays = np.full((4 * 16, 6), 7.0, np.float32)

    def call(s, rnd=0, first=0, n=4, r=rays, on_device=0, ptr=None):
        return lib.fw_lightmap_rays(None if s is None else C.byref(s[0]), 0, rnd, first, n, ptr if ptr is not None else (None if r is None else r.ctypes.data),
                                    on_device, None)

    assert call(None) == A.FW_ERR_BAD_ARG
    assert call(_lm(), r=None) == A.FW_ERR_BAD_ARG
    for what, s, _ in _bad_lightmaps():
        assert call(s) == A.FW_ERR_BAD_ARG, what
    assert call(_lm(), n=0) == A.FW_ERR_BAD_ARG
    assert call(_lm(), on_device=1, ptr=C.c_void_p(rays.ctypes.data + 2)) == A.FW_ERR_BAD_ARG
    assert call(_big(), n=0) == A.FW_ERR_BAD_ARG
    assert call(_big()) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call(_lm()) == A.FW_ERR_NO_DEVICE
        assert call(_lm(), rnd=0xFFFFFFFF, first=0xFFFFFFFF, n=2) == A.FW_ERR_NO_DEVICE    # (the covered list is only known on the device)
        assert np.all(rays == 7.0)


def test_lightmap_reduce_argument_checks():
    lib = _lib.load()
    acc = np.full((32, 4), 7.0, np.float32)
    sums = np.full((9, 4), 7.0, np.float32)
    ids = np.array([3, 1, 8, 0], np.uint32)

    def call(n=4, d=8, s=2, t=ids, a=acc, o=sums, nt=9, on_device=0, ptrs=None):
        pt, pa, po = ptrs if ptrs else (None if t is None else t.ctypes.data, None if a is None else a.ctypes.data, None if o is None else o.ctypes.data)
        return lib.fw_lightmap_reduce(0, n, d, s, pt, pa, po, nt, on_device, None)

    assert call(a=None) == A.FW_ERR_BAD_ARG and call(o=None) == A.FW_ERR_BAD_ARG
    assert call(n=0) == A.FW_ERR_BAD_ARG and call(nt=0) == A.FW_ERR_BAD_ARG
    assert call(d=0) == A.FW_ERR_BAD_ARG and call(d=(1 << 20) + 1) == A.FW_ERR_BAD_ARG
    assert call(s=0) == A.FW_ERR_BAD_ARG and call(s=(1 << 24) + 1) == A.FW_ERR_BAD_ARG
    assert call(t=None, nt=3) == A.FW_ERR_BAD_ARG                                           # the identity needs n <= n_texels
    assert call(t=np.array([3, 1, 9, 0], np.uint32)) == A.FW_ERR_BAD_ARG and "texel id 2 " in lib.fw_last_error().decode()
    good = (ids.ctypes.data, acc.ctypes.data, sums.ctypes.data)
    assert acc.ctypes.data % 16 == 0 and sums.ctypes.data % 16 == 0
    for k, off in ((0, 2), (1, 4), (2, 8)):
        ptrs = [C.c_void_p(x + (off if i == k else 0)) for i, x in enumerate(good)]
        assert call(on_device=1, ptrs=ptrs) == A.FW_ERR_BAD_ARG, k
    assert call(n=1 << 11, d=1 << 20, s=0, t=None, nt=1 << 11) == A.FW_ERR_BAD_ARG
    assert call(n=1 << 11, d=1 << 20, t=None, nt=1 << 11) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(t=None) == A.FW_ERR_NO_DEVICE
        assert np.all(sums == 7.0) and np.all(acc == 7.0)


def test_lightmap_dilate_argument_checks():
    lib = _lib.load()
    img = np.full((5, 17, 4), 7.0, np.float32)

    def call(w=17, h=5, passes=2, i=img, on_device=0, ptr=None):
        return lib.fw_lightmap_dilate(0, w, h, passes, ptr if ptr is not None else (None if i is None else i.ctypes.data), on_device, None)

    assert call(i=None) == A.FW_ERR_BAD_ARG
    assert call(w=0) == A.FW_ERR_BAD_ARG and call(w=16385) == A.FW_ERR_BAD_ARG and call(h=0) == A.FW_ERR_BAD_ARG and call(h=16385) == A.FW_ERR_BAD_ARG
    assert call(passes=65) == A.FW_ERR_BAD_ARG
    assert call(on_device=1, ptr=C.c_void_p(img.ctypes.data + 4)) == A.FW_ERR_BAD_ARG
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(passes=0) == A.FW_ERR_NO_DEVICE and call(passes=64) == A.FW_ERR_NO_DEVICE
        assert np.all(img == 7.0)


def test_bake_lightmap_argument_checks():
    """a 64-byte buffer that is no scene stands in for one: nothing dereferences it before the arguments are valid and a device is found"""
    lib = _lib.load()
    not_a_scene = C.create_string_buffer(64)
    sums = np.full((8, 8, 4), 7.0, np.float32)
    irr = np.full((8, 8, 4), 7.0, np.float32)

    def call(scene, s, p, first=0, rounds=1, dilate=2, o=sums, h=irr, ptrs=None):
        po, ph = ptrs if ptrs else (None if o is None else o.ctypes.data, None if h is None else h.ctypes.data)
        return lib.fw_bake_lightmap(scene, None if s is None else C.byref(s[0]), None if p is None else C.byref(p), first, rounds, dilate, po, ph, None)

    assert call(None, _lm(), _rp()) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, None, _rp()) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _lm(), None) == A.FW_ERR_BAD_ARG
    for what, s, _ in _bad_lightmaps():
        assert call(not_a_scene, s, _rp()) == A.FW_ERR_BAD_ARG, what
    assert call(not_a_scene, _lm(), _rp(), rounds=0) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _lm(), _rp(), first=0xFFFFFFFF, rounds=1) == A.FW_ERR_BAD_ARG       # first_round + rounds = 2^32
    assert call(not_a_scene, _lm(), _rp(samples=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _lm(), _rp(samples=(1 << 24) + 1)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _lm(), _rp(), dilate=65) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _lm(), _rp(), first=3, o=None) == A.FW_ERR_BAD_ARG
    assert sums.ctypes.data % 16 == 0 and irr.ctypes.data % 16 == 0
    for ptrs in ((C.c_void_p(sums.ctypes.data + 4), C.c_void_p(irr.ctypes.data)), (C.c_void_p(sums.ctypes.data), C.c_void_p(irr.ctypes.data + 8))):
        assert call(not_a_scene, _lm(), _rp(on_device=1), ptrs=ptrs) == A.FW_ERR_BAD_ARG
    # the order
    assert call(not_a_scene, _big(), _rp(), rounds=0) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _big(), _rp(samples=0)) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _big(), _rp(), dilate=65) == A.FW_ERR_BAD_ARG
    assert call(not_a_scene, _big(), _rp()) == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call(not_a_scene, _lm(), _rp()) == A.FW_ERR_NO_DEVICE
        # the ignored fields change nothing: n_rays, first_sample, per_sample_rays, key_base and gamma
        odd = _rp(n_rays=5, first_sample=0xFFFFFFFF, per_sample_rays=1, key_base=9, gamma=0.0)
        assert call(not_a_scene, _lm(), odd, first=0xFFFFFFFE, rounds=1) == A.FW_ERR_NO_DEVICE      # the last valid round
        assert call(not_a_scene, _lm(chunk_texels=3), _rp(), dilate=0, o=None, h=None) == A.FW_ERR_NO_DEVICE
        assert np.all(sums == 7.0) and np.all(irr == 7.0)


def test_python_entry_points_without_a_device_fail_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    scene, r = scenes.cornell_box()
    lm = R.lightmap("quad", 8, 8)
    for call in (lambda: _lib.lightmap_texels(lm), lambda: _lib.lightmap_rays(lm, 0, n=2),
                 lambda: _lib.lightmap_reduce(np.zeros((32, 4), np.float32), 1, 16, np.zeros((8, 8, 4), np.float32)),
                 lambda: _lib.lightmap_dilate(np.zeros((8, 8, 4), np.float32), 1), lambda: r.samples(2).bake_lightmap(scene, lm, 2)):
        with pytest.raises(_lib.FireworkError) as e:
            call()
        assert e.value.status == A.FW_ERR_NO_DEVICE


def test_cli_bake_lightmap_checks(capsys, tmp_path):
    from firework_amd.__main__ import main
    base = ["--scene-file", "s.yml", "-s", "4", "--bake-lightmap", "0,16,16", "-o", "l.npz"]
    for extra in (["--camera", "panorama"], ["--denoise"], ["--orbit", "3"], ["--adaptive", "0.05"], ["--progressive", "2"],
                  ["--checkpoint", "c.npz"], ["--temporal"], ["--orbit", "3", "--temporal"],
                  ["--bake-probes", "2,2,2", "--probe-min", "0,0,0", "--probe-max", "1,1,1"]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
        assert "--bake-lightmap cannot be combined" in capsys.readouterr().err, extra
    for bad, word in ((["--bake-lightmap", "0,16"], "OBJECT,W,H"), (["--bake-lightmap", "0,0,16"], "OBJECT,W,H"), (["--bake-lightmap", "a,b,c"], "OBJECT,W,H"),
                      (["--bake-lightmap", "-1,4,4"], "OBJECT,W,H"), (["--bake-lightmap", "0,4,16385"], "OBJECT,W,H"),
                      (["--lightmap-dirs", "0"], "--lightmap-dirs"), (["--lightmap-dirs", str((1 << 20) + 1)], "--lightmap-dirs"),
                      (["--lightmap-rounds", "0"], "--lightmap-rounds"), (["--lightmap-dilate", "65"], "--lightmap-dilate"),
                      (["--lightmap-dilate", "-1"], "--lightmap-dilate")):
        with pytest.raises(SystemExit) as e:
            main(base + bad)                                                              # (a repeated option: the last one counts)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad
    with pytest.raises(SystemExit) as e:
        main(base[:-2])
    assert e.value.code == 2 and "-o" in capsys.readouterr().err
    for alone in (["--lightmap-dirs", "64"], ["--lightmap-rounds", "2"], ["--lightmap-dilate", "1"]):
        with pytest.raises(SystemExit) as e:
            main(["--scene-file", "s.yml", "-s", "4", "-o", "x.png"] + alone)
        assert e.value.code == 2 and "need --bake-lightmap" in capsys.readouterr().err
    # an object that is not a mesh with uvs, or is not there: a message and exit status 2, no traceback, before any device is looked for
    scene_file = os.path.join(ROOT, "scenes", "three_lights.yml")
    for obj, word in (("0", "not a triangle mesh with uvs"), ("999", "does not exist")):
        assert main(["--scene-file", scene_file, "-s", "4", "--bake-lightmap", f"{obj},8,8", "-o", str(tmp_path / "l.npz")]) == 2
        err = capsys.readouterr().err
        assert word in err and "Traceback" not in err
    assert not (tmp_path / "l.npz").exists()


# ---- the numpy statements -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(8, 8), (17, 5), (64, 1)])
def test_texel_centres_invert_the_image_texture_lookup(w, h):
    """a texel centre pushed through ImageTexture's index arithmetic (i = floor(u w), j = floor((1 - v) h), in float32 as the tracer's,
    and in float64) returns its own (x, y)"""
    lm = R.lightmap("quad", w, h)
    u, v = lm.centres()
    y, x = np.divmod(np.arange(w * h), w)
    assert np.array_equal(np.floor(u * w).astype(np.int64), x) and np.array_equal(np.floor((1.0 - v) * h).astype(np.int64), y)
    u32, v32 = u.astype(np.float32), v.astype(np.float32)
    assert np.array_equal(np.floor(u32 * np.float32(w)).astype(np.int64), x)
    assert np.array_equal(np.floor((np.float32(1.0) - v32) * np.float32(h)).astype(np.int64), y)


@pytest.mark.parametrize("w,h", [(8, 8), (17, 5), (64, 1)])
def test_coverage_statement(w, h):
    e = R.edge_u(w)
    xe = w // 2                                                              # the column whose centres lie on the shared edge
    # texels whose centre lies exactly on a shared edge go to the lower triangle: the left quad's (0 or 1), never the right one's (2, 3)
    own = R.lightmap("shared_edge", w, h).texels()[1].reshape(h, w)
    assert np.all(own != NO)
    assert np.all(own[:, :xe + 1] <= 1) and np.all(own[:, xe + 1:] >= 2)
    u = (xe + 0.5) / w
    assert u == e
    if w == h:                                                               # the quad's own diagonal passes through the centres x + y = W - 1
        d = R.lightmap("diagonal", w, h).texels()[1].reshape(h, w)
        for y in range(h):
            assert d[y, w - 1 - y] == 0 and np.all(d[y, :w - 1 - y] == 1) and np.all(d[y, w - y:] == 0), y
    # overlapping triangles: the lower index wins wherever it covers
    ov = R.lightmap("overlap", w, h)
    both = ov.texels()[1]
    first = Lightmap(TriangleMesh(ov.mesh.verts, ov.mesh.indicies[:3], ov.mesh.normals, ov.mesh.uvs, 0), w, h).texels()[1]
    second = Lightmap(TriangleMesh(ov.mesh.verts, ov.mesh.indicies[3:], ov.mesh.normals, ov.mesh.uvs, 0), w, h).texels()[1]
    assert np.array_equal(both == 0, first == 0) and np.array_equal(both == 1, (second == 0) & (first == NO))
    assert np.any(both == 0) and np.any(both == 1)
    # a zero-area UV triangle covers nothing, although texel centres lie on it
    z = R.lightmap("zero_area", w, h).texels()[1]
    assert not np.any(z == 0) and np.any(z != NO)
    # uvs outside [0, 1] are clipped: what lies inside is covered as by the quad's own edge functions, nothing wraps round
    o = R.lightmap("outside", w, h)
    oo = o.texels()[1].reshape(h, w)
    cu, cv = (c.reshape(h, w) for c in o.centres())
    inside = (cu <= np.float64(np.float32(0.6))) & (cv <= np.float64(np.float32(0.7)))
    assert np.array_equal(oo != NO, inside) and not np.any(oo == 2)
    assert np.array_equal(o.covered(), np.nonzero(oo.reshape(-1) != NO)[0])


def test_records_statement():
    """positions interpolate the vertices and normals are unit, through a rotated placement and both flips"""
    lm = R.lightmap("quad", 8, 8, normals=False)
    rec, own = lm.texels()
    cov = own != NO
    assert cov.sum() == 25 and np.all(rec[~cov][:, [0, 1, 2, 4, 5, 6, 7]] == 0.0)
    assert np.array_equal(rec[:, 3].view(np.uint32), own) and np.all(rec[:, 7] == 0.0)
    u, v = lm.centres()
    want = np.stack([4.0 * u, 0.3 * u * v, 3.0 * v], axis=1)[cov]
    # (the sheet is bilinear, each triangle a plane through three of its points: equal on the edges, close inside)
    assert np.abs(rec[cov, 0] - want[:, 0]).max() <= 1e-6 and np.abs(rec[cov, 2] - want[:, 2]).max() <= 1e-6
    assert np.abs(rec[cov, 1] - want[:, 1]).max() <= 0.3 * 0.7 * 0.7 / 4 + 1e-6
    n = rec[cov, 4:7].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-7
    for place in ("rotated", "near_identity", "flip_normals", "flip", "both_flips"):
        for normals in (False, True):
            a = R.lightmap("quad", 8, 8, normals=normals).texels()[0]
            b = R.lightmap("quad", 8, 8, normals=normals, placement=place).texels()[0]
            rows = api.rotor_rows(R.lightmap("quad", 8, 8, placement=place).rotation).astype(np.float64)
            if place == "near_identity":
                rows = np.eye(3)
            sign = -1.0 if place in ("flip_normals", "flip") else 1.0
            nb = b[cov, 4:7].astype(np.float64)
            assert np.abs(nb - sign * a[cov, 4:7].astype(np.float64) @ rows.T).max() <= 3e-7, (place, normals)
            assert np.abs(np.linalg.norm(nb, axis=1) - 1.0).max() <= 2e-7
    # a triangle whose vertex normals cancel, or whose corners are collinear in space, loses its texels
    m = lm.mesh
    zero_n = Lightmap(TriangleMesh(m.verts, m.indicies, np.zeros_like(m.verts), m.uvs, 0), 8, 8).texels()[1]
    assert np.all(zero_n == NO)
    line = Lightmap(TriangleMesh(np.stack([m.uvs[:, 0], m.uvs[:, 0], m.uvs[:, 0]], axis=1), m.indicies, None, m.uvs, 0), 8, 8).texels()[1]
    assert np.all(line == NO)


@pytest.mark.parametrize("D", [1, 3, 16, 63, 64, 65, 200])
def test_rays_statement(D):
    lm = R.lightmap("quad", 8, 8, placement="rotated", directions=D).seed(7)
    rec, own = lm.texels()
    ids = lm.covered()
    n = ids.size
    rays = lm.rays(5)
    assert rays.shape == (n * D, 6) and rays.dtype == np.float32
    d = rays[:, 3:].astype(np.float64).reshape(n, D, 3)
    nrm = rec[ids, 4:7].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() <= 1e-7                         # unit
    cos = np.einsum("qjk,qk->qj", d, nrm)
    xi = lm.shifts(5, ids)
    c = np.sqrt(np.maximum(0.0, 1.0 - (np.arange(D)[None, :] + xi[:, 0:1]) / D))
    assert np.all(cos > 0.0) and np.abs(cos - c).max() <= 4e-7                           # d . n = c > 0
    if D > 1:
        assert np.all(np.diff(cos, axis=1) < 4e-7)                                       # c falls with j
    # origins: position + bias x normal; bias 0: the record's position bit for bit
    o = rays[:, :3].astype(np.float64).reshape(n, D, 3)
    assert np.abs(o - (rec[ids, None, 0:3].astype(np.float64) + float(np.float32(1e-3)) * nrm[:, None, :])).max() <= 2.0 ** -22
    zero = R.lightmap("quad", 8, 8, placement="rotated", directions=D).seed(7).bias(0.0).rays(5)
    assert np.array_equal(zero[:, :3].view(np.uint32), np.repeat(rec[ids, 0:3], D, axis=0).view(np.uint32))
    assert np.array_equal(zero[:, 3:], rays[:, 3:])
    # the shift is the texel id's: a part of the list, or a mesh that covers fewer texels, gives the same rays for the same texel
    assert np.array_equal(lm.rays(5, first=3, n=4), rays[3 * D:7 * D])
    assert np.array_equal(xi, api.pixel_jitter(7, 5, 64)[ids])
    half = Lightmap(TriangleMesh(lm.mesh.verts, lm.mesh.indicies[:3], lm.mesh.normals, lm.mesh.uvs, 0), 8, 8, D).placement(
        RenderObject.new(lm.mesh).rotate(lm.rotation).position_vec(lm._position)).seed(7)
    hid = half.covered()
    assert 0 < hid.size < n and np.all(half.texels()[1][hid] == own[hid])
    pick = np.searchsorted(ids, hid)
    assert np.array_equal(half.rays(5).reshape(-1, D, 6), rays.reshape(n, D, 6)[pick])
    # rounds and seeds change the shifts; jitter off: the shift (1/2, 1/2) in every round
    assert not np.array_equal(rays, lm.rays(6)) and not np.array_equal(rays, R.lightmap("quad", 8, 8, placement="rotated", directions=D).seed(8).rays(5))
    fixed = R.lightmap("quad", 8, 8, placement="rotated", directions=D).jitter(False)
    assert np.all(fixed.shifts(3, ids) == 0.5) and np.array_equal(fixed.rays(0), fixed.rays(9))
    s = fixed.to_abi()[0]
    assert (s.width, s.height, s.directions, s.jitter, s.seed, s.flip, s.chunk_texels) == (8, 8, D, 0, 0, 0, 0) and s.bias == np.float32(1e-3)


def test_dilation_statement_on_hand_made_masks():
    img = np.zeros((5, 5, 4), np.float32)
    img[2, 2] = (1.0, 2.0, 3.0, 1.0)
    one = api.lightmap_dilate(img, 1)
    ring = np.ones((5, 5), bool)
    ring[1:4, 1:4] = False
    assert np.all(one[1:4, 1:4, :3] == (1.0, 2.0, 3.0)) and np.all(one[ring] == 0.0)
    assert one[2, 2, 3] == 1.0 and np.all(np.delete(one[1:4, 1:4, 3].reshape(-1), 4) == 0.5)
    two = api.lightmap_dilate(img, 2)
    assert np.all(two[..., :3] == (1.0, 2.0, 3.0)) and np.all(two[ring, 3] == 0.5)
    assert np.array_equal(api.lightmap_dilate(one, 1), two) and np.array_equal(api.lightmap_dilate(img, 0), img)
    # two sources: the float32 sum in the neighbour order (-1,-1) ... (1,1), divided by float32(n); corners do not wrap round
    img = np.zeros((5, 5, 4), np.float32)
    img[0, 0] = (0.1, 0.2, 0.3, 1.0)
    img[0, 2] = (0.7, 0.5, 0.9, 1.0)
    img[2, 1] = (0.3, 0.3, 0.1, 1.0)
    out = api.lightmap_dilate(img, 1)
    f = np.float32
    want = ((f(0.1) + f(0.7)) + f(0.3)) / f(3.0)                                        # texel (1, 1): (-1,-1), (-1,1), (1,0)
    assert out[1, 1, 0] == want and out[1, 1, 3] == 0.5
    assert out[0, 1, 0] == (f(0.1) + f(0.7)) / f(2.0)                                   # texel (0, 1): (0,-1), (0,1); nothing above row 0
    assert np.all(out[4] == 0.0) and np.all(out[:, 4] == 0.0)                            # nothing arrives from the other side
    assert np.array_equal(out[0, 0], img[0, 0])                                          # a > 0 is copied
    # a filled texel (a = 0.5) is a source in the next pass and is itself left alone
    nxt = api.lightmap_dilate(out, 1)
    assert np.array_equal(nxt[1, 1], out[1, 1]) and nxt[3, 3, 3] == 0.5
    # an empty image stays empty
    assert np.all(api.lightmap_dilate(np.zeros((3, 4, 4), np.float32), 3) == 0.0)


def _one_texel(normal, D, seed):
    """a 1 x 1 lightmap whose only texel has the unit normal given (vertex normals), far enough from axis-aligned to be general"""
    mesh = TriangleMesh([[0, 0, 0], [1, 0, 0], [0, 0, 1]], [0, 1, 2], [list(normal)] * 3, [[0, 0], [2, 0], [0, 2]], 0)
    return Lightmap(mesh, 1, 1, D).seed(seed)


NORMALS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.6, 0.0, -0.8), (1 / 3, 2 / 3, -2 / 3), (-0.48, -0.6, 0.64)]


@pytest.mark.parametrize("D", [16, 64, 256, 4096])
def test_closed_forms_of_the_rays_statement(D):
    """(pi / D) sum_j L(d_j) on the statement's float32 rays, reduced by api.lightmap_reduce, against the closed forms: a constant L gives
    pi L up to rounding; the sky L(d) = h + 1/2 (d_y + 1)(z - h) gives pi (h + z) / 2 + (pi / 3)(z - h) n_y within C / D, C derived in
    tests/lightmap_ref.py: for the sky beta = 1/2 (z - h) e_y, so C = pi |z - h| / 2 (|n_y| + 2 sqrt(1 - n_y^2) / |sin(pi g)|), at most
    1.82 over these normals for the red channel's z - h = -0.5, and 0 for the blue one's z = h.
    Measured on the statement, largest |error| x D over normals, rounds, seeds and channels, beside the largest C of the same cases:
    D = 16: 0.47 vs 1.82; D = 64: 0.52 vs 1.82; D = 256: 0.42 vs 1.82; D = 4096: 0.49 vs 1.82 — recorded, not used."""
    hor, zen = np.array([1.0, 1.0, 1.0]), np.array([0.5, 0.7, 1.0])
    Lc = np.array([0.25, 1.5, 3.0])
    worst, worst_c = 0.0, 0.0
    for normal in NORMALS:
        for seed in (0, 11):
            lm = _one_texel(normal, D, seed)
            n = lm.texels()[0][0, 4:7].astype(np.float64)
            assert np.abs(n - np.asarray(normal)).max() <= 2.0 ** -24
            for rnd in range(3):
                rays = lm.rays(rnd)
                d = rays[:, 3:].astype(np.float64)
                for S in (1, 7):
                    acc = np.zeros((D, 4))
                    acc[:, :3] = Lc * S
                    got = api.lightmap_reduce(acc, S, D)[0]
                    assert np.all(np.abs(got - np.pi * Lc) <= (D + 16) * 2.0 ** -53 * np.pi * Lc)     # the weights sum to pi exactly
                    acc[:, :3] = R.sky(d, hor, zen) * S
                    got = api.lightmap_reduce(acc, S, D)[0]
                    want = R.sky_irradiance(hor, zen, n[None, :])[0]
                    for c in range(3):
                        alpha, beta = 0.5 * (hor[c] + zen[c]), np.array([0.0, 0.5 * (zen[c] - hor[c]), 0.0])
                        bound = R.closed_form_bound(alpha, beta, n, D)
                        assert abs(got[c] - want[c]) <= bound, (D, normal, seed, rnd, c, abs(got[c] - want[c]) * D, bound * D)
                        worst, worst_c = max(worst, abs(got[c] - want[c]) * D), max(worst_c, R.closed_form_C(beta, n))
    print(f"D {D}: largest error x D {worst:.3f}, largest C {worst_c:.3f}")
