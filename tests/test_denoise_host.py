"""CPU checks of the denoise entry points (lio_sor_filter, lio_radius_first_seed, lio_denoise_slam_map):
exported, in the ABI struct-size guard, and failing loudly (LIO_ERR_NODEV) without a device — there is no
CPU path behind them."""
import ctypes as C

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import filters as FL

NEW = ("lio_sor_filter", "lio_radius_first_seed", "lio_denoise_slam_map")


def test_new_symbols_are_exported():
    L = _capi.lib()
    for name in NEW:
        assert name in _capi.EXPORTS
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes, name  # declared with a signature


def test_abi_struct_sizes_include_denoise_params():
    L = _capi.lib()
    assert _capi._ABI_STRUCTS[-1] == "DenoiseParams"
    n = L.lio_abi_struct_sizes(None, 0)
    assert n == len(_capi._ABI_STRUCTS)
    sizes = (C.c_int64 * n)()
    L.lio_abi_struct_sizes(sizes, n)
    assert sizes[n - 1] == C.sizeof(_capi.DenoiseParams) == 24
    p = _capi.DenoiseParams(2800.0, 0.1, 0.5, 2700.0, 200, 0.2)
    assert (p.seed_thres, p.mean_k) == (2800.0, 200) and p.stddev_mul == np.float32(0.2)


def test_python_mirrors_exist():
    assert callable(FL.radius_first_seed) and callable(FL.denoise_slam_map)
    assert issubclass(FL.StatisticalOutlierRemoval, FL._Handle)
    for m in ("setMeanK", "setStddevMulThresh", "setNegative", "filter"):
        assert hasattr(FL.StatisticalOutlierRemoval, m)


def test_entry_points_fail_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    h = C.c_void_p()
    assert L.lio_filter_create(0, C.byref(h)) == _capi.LIO_ERR_NODEV and not h.value
    pts = np.zeros((8, 4), np.float32)
    out = np.zeros_like(pts)
    m = C.c_int64(0)
    fp = C.POINTER(C.c_float)
    rc = L.lio_sor_filter(None, pts.ctypes.data_as(fp), 8, 4, 5, 1.0, 0, out.ctypes.data_as(fp), C.byref(m), None, None)
    assert rc == _capi.LIO_ERR_NODEV
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    seed = np.zeros(8, np.int32)
    rc = L.lio_radius_first_seed(None, pts.ctypes.data_as(fp), 8, 4, pts.ctypes.data_as(fp), 2, 0.5,
                                 seed.ctypes.data_as(C.POINTER(C.c_int32)), None)
    assert rc == _capi.LIO_ERR_NODEV
    p = _capi.DenoiseParams(2800.0, 0.1, 0.5, 2700.0, 200, 0.2)
    rc = L.lio_denoise_slam_map(None, pts.ctypes.data_as(fp), 8, C.byref(p), out.ctypes.data_as(fp), C.byref(m), None)
    assert rc == _capi.LIO_ERR_NODEV
    # the Python mirrors raise the same error
    for call in (lambda: FL.StatisticalOutlierRemoval(5), lambda: FL.denoise_slam_map(pts),
                 lambda: FL.radius_first_seed(pts, pts[:2, :3], 0.5)):
        with pytest.raises(_capi.LioError) as e:
            call()
        assert e.value.code == _capi.LIO_ERR_NODEV
