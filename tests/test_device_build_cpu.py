"""CPU checks of fw_selftest_bvh_trees (the device tree builders' diagnostic) and of the BUILD option: device = -1 runs the host builders and
must give what fw_selftest_bvh_build hashes; without a GPU, device >= 0 is FW_ERR_NO_DEVICE.  The device builds themselves are compared
with the host's in tests/test_gpu_device_build.py."""
import ctypes as C

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib


def _boxes(n, seed, flat=False):              # as tests/test_host_build_cpu.py
    r = np.random.default_rng(seed)
    c = r.uniform(-10, 10, (n, 3)).astype(np.float32)
    if flat:
        c[:, 1] = np.float32(0.25)
        c[: n // 3, 0] = np.float32(1.5)
    e = r.uniform(0.001, 0.3, (n, 3)).astype(np.float32)
    return np.concatenate([c - e, c + e], axis=1)


def _fnv(a):
    h = 1469598103934665603
    for byte in np.ascontiguousarray(a, np.float32).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_export_exists():
    lib = _lib.load()
    assert hasattr(lib, "fw_selftest_bvh_trees")
    assert lib.fw_abi_version() == 8


@pytest.mark.parametrize("n,flat", [(1, False), (2, False), (3, False), (5000, False), (7001, True)])
def test_host_trees_match_the_host_build_hashes(n, flat):
    b = _boxes(n, 7 * n + flat, flat)
    ref, sah, st = _lib.selftest_bvh_trees(b, -1)
    h_ref, h_sah, st_build = _lib.selftest_bvh_build(b, 1)
    assert (_fnv(ref), _fnv(sah)) == (h_ref, h_sah)
    assert [int(x) for x in st] == [st_build["median_nodes"], st_build["median_depth"], st_build["sah_nodes"], st_build["sah_depth"]]
    assert ref.shape == (st_build["median_nodes"], 8) and sah.shape == (st_build["sah_nodes"], 8)


def test_host_trees_nan_centre():
    b = _boxes(100, 1)
    b[17, 0] = np.nan; b[17, 3] = np.nan
    with pytest.raises(_lib.FireworkError) as e:
        _lib.selftest_bvh_trees(b, -1)
    assert e.value.status == A.FW_ERR_NAN_BBOX


def test_device_without_gpu_is_no_device():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.FireworkError) as e:
        _lib.selftest_bvh_trees(_boxes(10, 1), 0)
    assert e.value.status == A.FW_ERR_NO_DEVICE


def test_argument_errors():
    lib = _lib.load()
    b = np.ascontiguousarray(_boxes(10, 1), np.float32)
    out = np.zeros(19 * 8, np.float32)
    st = (C.c_uint32 * 4)()
    p, o = b.ctypes.data, out.ctypes.data
    assert lib.fw_selftest_bvh_trees(-1, p, 0, o, o, st) == A.FW_ERR_BAD_ARG
    assert lib.fw_selftest_bvh_trees(-1, None, 10, o, o, st) == A.FW_ERR_BAD_ARG
    assert lib.fw_selftest_bvh_trees(-1, p, 10, None, o, st) == A.FW_ERR_BAD_ARG
    assert lib.fw_selftest_bvh_trees(-1, p, 10, o, None, st) == A.FW_ERR_BAD_ARG
    assert lib.fw_selftest_bvh_trees(-1, p, 10, o, o, None) == A.FW_ERR_BAD_ARG
    assert lib.fw_selftest_bvh_trees(-2, p, 10, o, o, st) == A.FW_ERR_BAD_ARG


def test_build_option_values():
    for v in ("host", "device", None):
        _lib.set_option("BUILD", v)
    _lib.set_option("BUILD", None)
    for bad in ("gpu", "1", ""):
        with pytest.raises(_lib.FireworkError) as e:
            _lib.set_option("BUILD", bad)
        assert e.value.status == A.FW_ERR_BAD_ARG
    _lib.set_option("BUILD", None)
