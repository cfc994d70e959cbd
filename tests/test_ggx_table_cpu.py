"""CPU-side checks of the GGX albedo table (fw_check_ggx_quad, fw_ggx_terms, fw_ggx_table, fw_ggx_table_lookup, fw_probe_shade_split;
DESIGN.md §9y): the exports and their ctypes signatures against the header, fw_ggx_quad's layout against the C compiler's; every
argument error of the five calls in the header's order (they come before HIP is called), and the no-device error with the caller's
buffers untouched; GgxTable's validation and the CLI's refusals; and the properties of the numpy statement — the mirror at rho = 0,
the signs and the bound of the terms, §9m's 0.31, the 24 points against ggx_ref's independent half-vector quadrature, the lookup at
texel centres, outside [0, 1] and on an affine table, and the white furnace of the split shade."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, api
from firework_amd.api import GgxTable

import ggx_ref as G
import ggx_table_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
MUS, RHOS = (1.0 / 64, 0.1, 0.5, 0.99), (1.0 / 64, 0.05, 0.1, 0.3, 0.6, 1.0)


# ---- exports and layout ---------------------------------------------------------------------------------------------------------------
def _ctype_of(param):
    param = param.strip()
    if "*" in param:
        for name, t in (("fw_ggx_quad", A.fw_ggx_quad), ("fw_probe_grid", A.fw_probe_grid), ("fw_probe_radiance", A.fw_probe_radiance),
                        ("fw_probe_depth", A.fw_probe_depth), ("fw_probe_shade_params", A.fw_probe_shade_params)):
            if re.search(rf"\b{name}\b", param):
                return C.POINTER(t)
        return C.c_void_p
    if param.startswith("uint32_t"):
        return C.c_uint32
    if param.startswith("float "):
        return C.c_float
    assert param.startswith("int "), param
    return C.c_int


def test_exports_and_signatures_at_abi_8():
    lib = _lib.load()
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert sorted(A.GGX_TABLE_PROTOTYPES) == ["fw_check_ggx_quad", "fw_ggx_table", "fw_ggx_table_lookup", "fw_ggx_terms", "fw_probe_shade_split"]
    for name, argtypes in A.GGX_TABLE_PROTOTYPES.items():
        assert hasattr(lib, name), name
        found = re.findall(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert len(found) == 1, name
        want = [_ctype_of(p) for p in found[0].replace("\n", " ").split(",")]
        assert argtypes == want, (name, argtypes, want)
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == C.c_int
    assert re.search(r"#define FW_SPLIT_ENERGY 1u", text) and A.FW_SPLIT_ENERGY == 1


def test_struct_layout(tmp_path):
    """ctypes' fw_ggx_quad equals the C compiler's, size and every field offset"""
    names = ["m1", "m2"]
    assert [f for f, _ in A.fw_ggx_quad._fields_] == names
    src = ('#include "firework_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("' + "%zu " * (len(names) + 1) + '\\n",sizeof(fw_ggx_quad)' +
           "".join(f",offsetof(fw_ggx_quad,{f})" for f in names) + ");return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(A.fw_ggx_quad)] + [getattr(A.fw_ggx_quad, f).offset for f in names]
    q = GgxTable().to_abi()
    assert (q.m1, q.m2) == (128, 128)


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def _said(lib, st, word):
    msg = lib.fw_last_error().decode()
    assert st in (A.FW_ERR_BAD_ARG, A.FW_ERR_UNSUPPORTED), (st, msg)
    assert word in msg, (word, msg)
    return st


def _q(m1=16, m2=16):
    return A.fw_ggx_quad(m1, m2)


BAD_QUADS = [("m1", _q(m1=0)), ("m1", _q(m1=1025)), ("m1", _q(m1=0, m2=0)), ("m2", _q(m2=0)), ("m2", _q(m2=1025))]


def test_check_ggx_quad():
    lib = _lib.load()
    assert _said(lib, lib.fw_check_ggx_quad(None), "null") == A.FW_ERR_BAD_ARG
    for word, q in BAD_QUADS:
        assert _said(lib, lib.fw_check_ggx_quad(C.byref(q)), word) == A.FW_ERR_BAD_ARG
    for q in (_q(1, 1), _q(1024, 1024), _q(128, 128)):
        assert lib.fw_check_ggx_quad(C.byref(q)) == A.FW_OK
    with pytest.raises(_lib.FireworkError, match="m2"):
        _lib.check_ggx_quad((16, 2000))
    _lib.check_ggx_quad(GgxTable())


def test_ggx_terms_argument_checks():
    lib = _lib.load()
    mu, rho, out = np.full(4, 0.5, np.float32), np.full(4, 0.5, np.float32), np.full((4, 2), 7.0, np.float32)

    def call(q=None, n=4, device=0, on_device=0, null_q=False, m=mu.ctypes.data, r=rho.ctypes.data, o=out.ctypes.data):
        return lib.fw_ggx_terms(None if null_q else C.byref(q if q is not None else _q()), device, n, m, r, o, on_device, None)

    assert _said(lib, call(null_q=True), "null") == A.FW_ERR_BAD_ARG
    for kw in (dict(m=None), dict(r=None), dict(o=None)):
        assert _said(lib, call(_q(m1=0), **kw), "null") == A.FW_ERR_BAD_ARG                               # NULL before the quadrature
    for word, q in BAD_QUADS:
        assert _said(lib, call(q, n=0), word) == A.FW_ERR_BAD_ARG                                         # the quadrature before the size
    assert _said(lib, call(n=0, on_device=1, m=C.c_void_p(mu.ctypes.data + 2)), "n must") == A.FW_ERR_BAD_ARG
    for kw in (dict(m=C.c_void_p(mu.ctypes.data + 2)), dict(r=C.c_void_p(rho.ctypes.data + 2)), dict(o=C.c_void_p(out.ctypes.data + 4))):
        assert _said(lib, call(on_device=1, device=-1, **kw), "aligned") == A.FW_ERR_BAD_ARG              # alignment before the device
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(out == 7.0)
        with pytest.raises(_lib.FireworkError) as e:
            _lib.ggx_terms((16, 16), mu, rho)
        assert e.value.status == A.FW_ERR_NO_DEVICE
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG
        assert np.all(out == 7.0)


def test_ggx_table_argument_checks():
    lib = _lib.load()
    tab = np.full((4, 4, 2), 7.0, np.float32)

    def call(q=None, n_mu=4, n_rho=4, device=0, on_device=0, null_q=False, t=tab.ctypes.data):
        return lib.fw_ggx_table(None if null_q else C.byref(q if q is not None else _q()), device, n_mu, n_rho, t, on_device, None)

    assert _said(lib, call(null_q=True), "null") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_q(m1=0), t=None), "null") == A.FW_ERR_BAD_ARG
    for word, q in BAD_QUADS:
        assert _said(lib, call(q, n_mu=1), word) == A.FW_ERR_BAD_ARG
    for n_mu, n_rho in ((1, 4), (4, 1), (257, 4), (4, 257), (0, 0)):
        assert _said(lib, call(n_mu=n_mu, n_rho=n_rho, on_device=1, t=C.c_void_p(tab.ctypes.data + 4)), "n_mu and n_rho") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(on_device=1, device=-1, t=C.c_void_p(tab.ctypes.data + 4)), "aligned") == A.FW_ERR_BAD_ARG
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(n_mu=2, n_rho=2) == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(tab == 7.0)
        with pytest.raises(_lib.FireworkError) as e:
            _lib.ggx_table(GgxTable(4, 4, 16, 16))
        assert e.value.status == A.FW_ERR_NO_DEVICE
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG
        assert np.all(tab == 7.0)


def test_ggx_table_lookup_argument_checks():
    lib = _lib.load()
    tab, mu, rho, out = np.full((4, 4, 2), 7.0, np.float32), np.full(4, 0.5, np.float32), np.full(4, 0.5, np.float32), np.full((4, 2), 7.0, np.float32)

    def call(n_mu=4, n_rho=4, n=4, device=0, on_device=0, t=tab.ctypes.data, m=mu.ctypes.data, r=rho.ctypes.data, o=out.ctypes.data):
        return lib.fw_ggx_table_lookup(device, n_mu, n_rho, t, n, m, r, o, on_device, None)

    for kw in (dict(t=None), dict(m=None), dict(r=None), dict(o=None)):
        assert _said(lib, call(n_mu=1, **kw), "null") == A.FW_ERR_BAD_ARG
    for n_mu, n_rho in ((1, 4), (4, 1), (257, 4), (4, 257)):
        assert _said(lib, call(n_mu=n_mu, n_rho=n_rho, n=0), "n_mu and n_rho") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(n=0, on_device=1, t=C.c_void_p(tab.ctypes.data + 4)), "n must") == A.FW_ERR_BAD_ARG
    for kw in (dict(t=C.c_void_p(tab.ctypes.data + 4)), dict(m=C.c_void_p(mu.ctypes.data + 2)), dict(r=C.c_void_p(rho.ctypes.data + 2)),
               dict(o=C.c_void_p(out.ctypes.data + 4))):
        assert _said(lib, call(on_device=1, device=-1, **kw), "aligned") == A.FW_ERR_BAD_ARG
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(device=5) == A.FW_ERR_NO_DEVICE
        assert np.all(out == 7.0)
        with pytest.raises(_lib.FireworkError) as e:
            _lib.ggx_table_lookup(tab, mu, rho)
        assert e.value.status == A.FW_ERR_NO_DEVICE
    else:
        assert _said(lib, call(device=_lib.device_count()), "device") == A.FW_ERR_BAD_ARG and call(device=-1) == A.FW_ERR_BAD_ARG
        assert np.all(out == 7.0)


def _grid(lo=(0.0, 0.0, 0.0), hi=(1.0, 2.0, 3.0), counts=(2, 3, 2), flags=1):
    g = A.fw_probe_grid()
    for k in range(3):
        g.lo[k], g.hi[k], g.counts[k] = lo[k], hi[k], counts[k]
    g.flags = flags
    return g


def _rad(resolution=8, sharpness_log2=2, levels=2, roughness=(0.1, 1.0, 0.0, 0.0)):
    d = A.fw_probe_radiance()
    d.resolution, d.sharpness_log2, d.levels = resolution, sharpness_log2, levels
    for i, v in enumerate(roughness):
        d.roughness[i] = v
    return d


def _depth(resolution=8, sharpness_log2=6, max_distance=10.0):
    d = A.fw_probe_depth()
    d.resolution, d.sharpness_log2, d.max_distance = resolution, sharpness_log2, max_distance
    return d


def test_probe_shade_split_argument_checks():
    """fw_probe_shade_glossy's errors in its order, the table among the NULLs, its sizes and the flags straight after them"""
    lib = _lib.load()
    buf = dict(sh=np.full((12, 9, 3), 7.0, np.float32), maps=np.full((12, 80, 4), 7.0, np.float32), mom=np.full((12, 8, 8, 2), 7.0, np.float32),
               pl=np.full((12, 4), 7.0, np.float32), aov=np.full((6, 12), 7.0, np.float32), spec=np.full((6, 4), 7.0, np.float32),
               view=np.full((6, 3), 7.0, np.float32), tab=np.full((4, 4, 2), 7.0, np.float32), lin=np.full((6, 3), 7.0, np.float32),
               gam=np.full((6, 3), 7.0, np.float32), rgb8=np.full((6, 3), 7, np.uint8))
    good = {k: v.ctypes.data for k, v in buf.items()}

    def params(**kw):
        p = A.fw_probe_shade_params()
        p.width, p.height, p.gamma = 3, 2, 2.2
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(g=None, pr=None, pd=None, bias=0.0, p=None, vstride=3, n_mu=4, n_rho=4, flags=0, null=None, **ptrs):
        a = dict(good, **ptrs)
        gp = None if null == "grid" else C.byref(g if g is not None else _grid())
        rp = None if null == "pr" else C.byref(pr if pr is not None else _rad())
        dp = None if null == "pd" else C.byref(pd if pd is not None else _depth())
        pp = None if null == "p" else C.byref(p if p is not None else params())
        return lib.fw_probe_shade_split(gp, a["sh"], rp, a["maps"], dp, a["mom"], bias, a["pl"], pp, a["aov"], a["spec"], a["view"], vstride,
                                        a["tab"], n_mu, n_rho, flags, a["lin"], a["gam"], a["rgb8"])

    for null in ("grid", "pr", "pd", "p"):
        assert _said(lib, call(null=null, n_mu=1), "null") == A.FW_ERR_BAD_ARG, null
    for name in ("sh", "maps", "mom", "aov", "spec", "view", "tab"):
        assert _said(lib, call(n_mu=1, **{name: None}), "null") == A.FW_ERR_BAD_ARG, name
    for n_mu, n_rho in ((1, 4), (4, 1), (257, 4), (4, 257)):
        assert _said(lib, call(n_mu=n_mu, n_rho=n_rho, flags=2, lin=None, gam=None, rgb8=None), "n_mu and n_rho") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(flags=2, lin=None, gam=None, rgb8=None), "flags") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(pr=_rad(resolution=5), lin=None, gam=None, rgb8=None), "output") == A.FW_ERR_BAD_ARG     # then the counterpart's
    assert _said(lib, call(pr=_rad(resolution=5), pd=_depth(resolution=5)), "resolution") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_grid(flags=2), bias=-0.5), "normal_bias") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(_grid(counts=(2, 0, 2)), p=params(width=0)), "count") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(p=params(width=0, gamma=0.0)), "width") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(p=params(gamma=NAN, device=-1), vstride=2), "gamma") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(p=params(device=-1), vstride=2), "view_stride") == A.FW_ERR_BAD_ARG
    assert _said(lib, call(p=params(device=-1)), "device") == A.FW_ERR_BAD_ARG
    for name, off in (("aov", 8), ("spec", 4), ("maps", 8), ("tab", 4), ("sh", 2), ("view", 2), ("lin", 2), ("gam", 2), ("mom", 2), ("pl", 2)):
        assert _said(lib, call(p=params(on_device=1), **{name: C.c_void_p(good[name] + off)}), "aligned") == A.FW_ERR_BAD_ARG, name
    assert _said(lib, call(_grid(counts=(1 << 11, 1 << 10, 1 << 10))), "nx x ny x nz") == A.FW_ERR_UNSUPPORTED
    assert _said(lib, call(p=params(width=0x10000, height=0x10000)), "image too large") == A.FW_ERR_UNSUPPORTED
    if _lib.device_count() == 0:
        assert call() == A.FW_ERR_NO_DEVICE and call(null="pd", mom=None, pl=None, flags=1) == A.FW_ERR_NO_DEVICE
        assert all(np.all(v == 7) for v in buf.values())
        grid = api.ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1))
        pr = api.ProbeRadiance(8)
        with pytest.raises(_lib.FireworkError) as e:
            _lib.probe_shade_split(grid, np.zeros((2, 9, 3), np.float32), pr, np.ones((2, pr.texels, 4), np.float32), np.zeros((1, 12), np.float32),
                                   np.zeros((1, 4), np.float32), np.ones((1, 3), np.float32), np.ones((4, 4, 2), np.float32), 1, 1)
        assert e.value.status == A.FW_ERR_NO_DEVICE
    else:
        assert call(p=params(device=_lib.device_count())) == A.FW_ERR_BAD_ARG


def test_ggx_table_validation():
    t = GgxTable()
    assert (t.n_mu, t.n_rho, t.m1, t.m2, t.energy, t.flags) == (64, 64, 128, 128, False, 0)
    assert GgxTable(energy=True).flags == A.FW_SPLIT_ENERGY and GgxTable(2, 256, 1, 1024).check() is not None
    for kw, word in ((dict(n_mu=1), "n_mu"), (dict(n_rho=257), "n_mu and n_rho"), (dict(m1=0), "m1"), (dict(m2=1025), "m1 and m2")):
        with pytest.raises(ValueError, match=word):
            GgxTable(**kw)
    t.m1 = 5000
    with pytest.raises(ValueError, match="m1"):
        t.check()
    r = api.Renderer.default()
    with pytest.raises(ValueError, match="ggx_table needs radiance"):
        r.render_probe_lit(None, api.ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1)), np.zeros((2, 9, 3), np.float32), ggx_table=GgxTable())


@pytest.mark.parametrize("args, word", [
    (["--probe-energy"], "--probe-split-sum"),
    (["--probe-lit", "none.npz", "-o", "x.png", "--probe-energy"], "--probe-split-sum"),
    (["--probe-split-sum"], "--probe-lit"),
    (["--probe-split-sum", "32,32"], "--probe-lit"),
    (["--probe-lit", "none.npz", "-o", "x.png", "--probe-split-sum", "--probe-no-radiance"], "--probe-no-radiance"),
    (["--probe-lit", "none.npz", "-o", "x.png", "--probe-split-sum", "1,32"], "N_MU,N_RHO"),
    (["--probe-lit", "none.npz", "-o", "x.png", "--probe-split-sum", "32,257"], "N_MU,N_RHO"),
    (["--probe-lit", "none.npz", "-o", "x.png", "--probe-split-sum", "32"], "N_MU,N_RHO"),
    (["--probe-lit", "none.npz", "-o", "x.png", "--probe-split-sum", "a,b"], "N_MU,N_RHO"),
])
def test_cli_refusals_come_before_the_scene_is_read(args, word, capsys):
    """argparse's exit 2 with a message naming the flag; the scene file does not exist, so nothing was loaded, let alone a device asked"""
    from firework_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--scene-file", "none.yml", "-s", "1"] + args)
    assert e.value.code == 2 and word in capsys.readouterr().err, args


def test_cli_refuses_a_file_without_radiance_maps(tmp_path, capsys):
    """the file is looked at before the scene and the device are: one without radiance maps is a message and exit status 2"""
    from firework_amd.__main__ import main
    path = tmp_path / "probes.npz"
    np.savez(path, sh=np.zeros((2, 9, 3), np.float32), grid_lo=np.zeros(3), grid_hi=np.ones(3), grid_counts=np.array([2, 1, 1]))
    assert main(["--scene-file", "none.yml", "-s", "1", "--probe-lit", str(path), "-o", str(tmp_path / "x.png"), "--probe-split-sum"]) == 2
    assert "holds none" in capsys.readouterr().err


# ---- properties of the statement ------------------------------------------------------------------------------------------------------
def test_rho_zero_is_a_mirror():
    mu = np.array([2.0 ** -6, 0.1, 0.3, 0.5, 0.9, 0.99, 1.0], np.float32)
    m64 = mu.astype(np.float64)
    for m1, m2 in ((1, 1), (3, 2), (16, 16), (40, 25), (128, 128)):
        _, T = api.ggx_terms(mu, np.zeros_like(mu), m1, m2, terms=True)
        assert np.allclose(T["AB"][:, 1], (1.0 - m64) ** 5, rtol=1e-13, atol=1e-15), (m1, m2)
        assert np.allclose(T["AB"][:, 0], 1.0 - (1.0 - m64) ** 5, rtol=1e-13, atol=1e-15), (m1, m2)


def test_terms_are_non_negative_and_bounded():
    rng = np.random.default_rng(5)
    mu = np.concatenate([rng.random(400).astype(np.float32), np.float32([1.0, 2.0 ** -6, 1e-30, 1.0, 1.0])])
    rho = np.concatenate([rng.random(400).astype(np.float32), np.float32([1.0, 1.0, 0.5, 0.0, 2.0 ** -6])])
    for m1, m2 in ((1, 1), (9, 7), (32, 32)):
        _, T = api.ggx_terms(mu, rho, m1, m2, terms=True)
        AB = T["AB"]
        assert np.all(np.isfinite(AB)) and np.all(AB >= 0.0) and np.all(AB[:, 0] + AB[:, 1] <= 1.0 + 2.0 ** -40), (m1, m2)
    out = api.ggx_terms(np.float32([0.0, -0.5, 1.5, 0.5, 0.5, NAN, 0.5, INF]), np.float32([0.5, 0.5, 0.5, -0.1, 1.1, 0.5, NAN, 0.5]), 8, 8)
    assert np.all(out == 0.0)


def test_section_9m_albedo_at_roughness_one():
    _, T = api.ggx_terms([0.99], [1.0], 128, 128, terms=True)
    assert abs(T["AB"][0].sum() - 0.3088) <= 2e-3


def test_24_points_against_the_half_vector_quadrature():
    """both terms at 128 x 128 within 2e-3 of ggx_ref.albedo's independent rule: 8.8e-4 between this rule at 128^2 and at 2048^2, plus
    2e-5 between the two rules, with a factor of two over the sum.  The largest seen is 8.7e-4 (mu = 0.99, rho = 0.3)."""
    mu = np.float32([m for m in MUS for _ in RHOS])
    rho = np.float32([r for _ in MUS for r in RHOS])
    _, T = api.ggx_terms(mu, rho, 128, 128, terms=True)
    worst = 0.0
    for i in range(mu.size):
        e1, e0 = G.albedo(float(mu[i]), float(rho[i]), 1.0, 512, 1024), G.albedo(float(mu[i]), float(rho[i]), 0.0, 512, 1024)
        worst = max(worst, abs(T["AB"][i, 0] - (e1 - e0)), abs(T["AB"][i, 1] - e0))
        assert abs(T["AB"][i, 0] + T["AB"][i, 1] - e1) <= 2e-3 and abs(T["AB"][i, 1] - e0) <= 2e-3, (mu[i], rho[i])
        assert abs(T["AB"][i, 0] - (e1 - e0)) <= 2e-3, (mu[i], rho[i])
    print(f"largest |term - half-vector quadrature| at the 24 points: {worst:.3e}")


def test_sampler_is_section_9m_s():
    """the statement's (wi, h) of a sample equal ggx_ref.sample_local's — the renderer's sampler — up to the frame's sign convention:
    T1 = (0, 1, 0) here is ggx_ref's (-Vh.y, Vh.x, 0) / |.| for a wo in the xz plane"""
    for mu, rho in ((0.3, 0.7), (0.9, 0.2), (2.0 ** -6, 1.0)):
        alpha = float(G.alpha_of(rho))
        wo = G.wo_of(float(np.float32(mu)))
        xi1, xi2 = np.meshgrid((np.arange(8) + 0.5) / 8, (np.arange(4) + 0.5) / 4, indexing="ij")
        wi, h = G.sample_local(wo, alpha, xi1, xi2)
        alive = wi[..., 2] > 0
        lo, li = G.lam(wo, alpha), G.lam(np.where(alive[..., None], wi, [0.0, 0.0, 1.0]), alpha)
        m = 1.0 - np.sum(h * wo, -1)
        k = np.where(alive, (1 + lo) / (1 + lo + li), 0.0)
        want = np.array([np.mean(k * (1 - m ** 5)), np.mean(k * m ** 5)])
        _, T = api.ggx_terms([mu], [rho], 8, 4, terms=True)
        assert np.allclose(T["AB"][0], want, rtol=1e-12, atol=1e-15), (mu, rho)


def test_table_is_terms_at_the_centres():
    t = api.ggx_table(3, 5, 9, 7)
    mu, rho = api.ggx_table_centres(3, 5)
    assert t.shape == (5, 3, 2) and t.dtype == np.float32
    assert mu[2, 1] == np.float32(1.5 / 3.0) and rho[2, 1] == np.float32(2.5 / 5.0)
    assert np.array_equal(t, api.ggx_terms(mu.reshape(-1), rho.reshape(-1), 9, 7).reshape(5, 3, 2))


def _wild_table(n_mu, n_rho, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n_rho, n_mu, 2)) * 10.0 ** rng.integers(-20, 20, size=(n_rho, n_mu, 2))).astype(np.float32)


def test_lookup_at_centres_and_outside():
    """a centre of a power-of-two size is x = i exactly, so the lookup returns that texel's bits whatever the neighbours hold (at other
    sizes float32((i + 0.5) / n) n - 0.5 misses i by a rounding of mu times n, and a share of the neighbour that small comes in)"""
    for n_mu, n_rho in ((2, 2), (16, 16), (256, 8), (3, 5), (100, 7)):
        t = _wild_table(n_mu, n_rho)
        mu, rho = api.ggx_table_centres(n_mu, n_rho)
        if n_mu & (n_mu - 1) == 0 and n_rho & (n_rho - 1) == 0:
            got = api.ggx_table_lookup(t, mu.reshape(-1), rho.reshape(-1)).reshape(n_rho, n_mu, 2)
            assert np.array_equal(got.view(np.uint32), t.view(np.uint32)), (n_mu, n_rho)
        out = api.ggx_table_lookup(t, np.float32([-3.0, 0.0, 1.0, 7.0, -INF, 1e30]), np.float32([-1.0, 0.0, 1.0, 2.0, 0.5, -1e30]))
        assert np.array_equal(out[0], t[0, 0]) and np.array_equal(out[1], t[0, 0]) and np.array_equal(out[2], t[-1, -1]) and np.array_equal(out[3], t[-1, -1])
        assert np.all(out[4] == 0.0) and np.array_equal(out[5], t[0, -1])
        assert np.all(api.ggx_table_lookup(t, np.float32([NAN, 0.5, INF]), np.float32([0.5, NAN, 0.5])) == 0.0)


def test_lookup_of_an_affine_table_is_affine():
    n_mu, n_rho = 16, 12
    mu_c, rho_c = api.ggx_table_centres(n_mu, n_rho)
    f = lambda m, r: np.stack([0.25 + 0.5 * m - 0.125 * r, 1.0 - 0.75 * m + 0.5 * r], -1)           # noqa: E731
    t = f(mu_c.astype(np.float64), rho_c.astype(np.float64)).astype(np.float32)
    rng = np.random.default_rng(11)
    mu = (0.5 / n_mu + (1.0 - 1.0 / n_mu) * rng.random(500)).astype(np.float32)                        # between the outermost centres
    rho = (0.5 / n_rho + (1.0 - 1.0 / n_rho) * rng.random(500)).astype(np.float32)
    got = api.ggx_table_lookup(t, mu, rho)
    want = f(mu.astype(np.float64), rho.astype(np.float64))
    assert np.all(np.abs(got - want) <= 4.0 * np.spacing(np.abs(want).astype(np.float32)))


def test_white_furnace_of_the_split_shade():
    """F0 = 1 with the energy flag under Ls = c gives c within 4 float32 ulps at every texel centre of a 16 x 16 table; without the flag
    it gives float32 E1 c"""
    n = 16
    table = api.ggx_table(n, n, 32, 32)
    mu, rho = (v.reshape(-1) for v in api.ggx_table_centres(n, n))
    N = mu.size
    c = np.float32([0.75, 1.5, 3.0])
    aov = np.zeros((N, 12), np.float32)
    aov[:, 0:3], aov[:, 3], aov[:, 5], aov[:, 8:11] = 0.5, 1.0, 1.0, 0.25                             # albedo, coverage, normal +y, position
    sx = np.sqrt(1.0 - mu.astype(np.float64) ** 2)
    view = np.stack([sx, -mu.astype(np.float64), np.zeros(N)], 1).astype(np.float32)                   # towards the floor: -(n . u) = mu
    spec = np.concatenate([np.ones((N, 3), np.float32), rho[:, None]], 1)
    Ls = np.broadcast_to(c, (N, 3)).copy()
    mu_f = api.probe_split_mu(aov, view)
    assert np.all(np.abs(mu_f - mu) <= np.spacing(mu))
    terms = api.ggx_table_lookup(table, mu_f, rho)
    on = api.probe_split_ref(aov, spec, view, np.zeros((N, 3), np.float32), Ls, terms=terms, flags=A.FW_SPLIT_ENERGY)
    assert np.all(np.abs(on - c) <= 4.0 * np.spacing(c)), float(np.max(np.abs(on - c) / np.spacing(c)))
    off = api.probe_split_ref(aov, spec, view, np.zeros((N, 3), np.float32), Ls, terms=terms)
    e1 = (np.float32(1.0) * terms[:, 0] + terms[:, 1]).astype(np.float32)
    assert np.array_equal(off, (np.float32(1.0) * (e1[:, None] * Ls)).astype(np.float32))
    assert np.array_equal(api.probe_split_ref(aov, spec, view, np.zeros((N, 3), np.float32), Ls, table=table), off)   # its own lookup
    spec[:, 3] = 0.0                                                                                   # diffuse: the placed shade's output
    d = np.full((N, 3), 0.125, np.float32)
    assert np.array_equal(api.probe_split_ref(aov, spec, view, d, Ls, terms=terms, flags=1), d)


def test_bound_module_restates_the_statement():
    """tests/ggx_table_ref.py carries error bounds along the statement: its values are api.ggx_terms' bit for bit, its K stays below
    2^-30 on the GPU test's own inputs, and those inputs need no replacement"""
    for (m1, m2) in R.QUADS:
        for n in R.COUNTS:
            mu, rho, replaced = R.pairs(n, 100 + n, m1, m2)
            assert replaced <= R.MAX_REPLACED * n and replaced == 0
            AB, bound, info = R.terms_bound(mu, rho, m1, m2)
            _, T = api.ggx_terms(mu, rho, m1, m2, terms=True)
            assert np.array_equal(AB, T["AB"]) and np.all(info["fit"])
            assert np.all(info["K"] * 2.0 ** -53 < R.K_LIMIT) and np.all(info["min_wz"] >= R.WZ_MARGIN)
            if n >= 12:
                assert np.any(rho == 0) and np.any(rho == 1) and np.any(mu == 1) and np.any(mu == np.float32(2.0 ** -6))
                assert np.any(np.isnan(mu)) and np.any(np.isnan(rho)) and np.any(mu > 1) and np.any(rho < 0)
