"""CPU checks of the GPS alignment interface (lio_gps_align, lio_similarity2d_fit, lio_georeference_xy): declared
in the header with the contract in words, exported by the library, listed in the binding, failing loudly
(LIO_ERR_NODEV) without a device — there is no CPU path behind them — and mirrored in Python and C++."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"lio_gps_align": 10, "lio_similarity2d_fit": 5, "lio_georeference_xy": 10}
dp = C.POINTER(C.c_double)


def _decl(src, name):
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert decl, f"{name} is not declared"
    comment = " ".join(src[:decl.start()].rsplit("/*", 1)[1].replace("*", " ").split())
    return " ".join(decl.group(1).split()), comment


def test_header_declares_the_entries_and_the_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    args, comment = _decl(src, "lio_gps_align")
    assert len(args.split(",")) == 10
    for piece in ("lio_filter* f", "const double* gps_xy", "int64_t m", "const double* slam_xy", "int64_t n",
                  "int max_iterations", "double tolerance", "double* aligned_xy_out", "int32_t* nn_out_opt", "double* out"):
        assert piece in args, piece
    # the tie rule, the summation order and the reference-return quirk, in words
    assert re.search(r"an equal d2 goes to the lowest index", comment, flags=re.I)
    assert "not on the rooted distance" in comment
    assert re.search(r"TREE\(v\)", comment) and re.search(r"ascending block order", comment, flags=re.I) and "+0.0" in comment
    assert re.search(r"reference's return triple", comment, flags=re.I) and "quirk" in comment
    assert re.search(r"last iteration only", comment, flags=re.I)
    assert comment.count("this library's contract") >= 2
    assert "LIO_ERR_STATE" in comment and "zero variance" in comment
    for macro in ("LIO_GPSALIGN_LEN", "LIO_GPSALIGN_ITERATIONS", "LIO_GPSALIGN_CONVERGED", "LIO_GPSALIGN_MEAN_ERROR",
                  "LIO_GPSALIGN_REF_SCALE", "LIO_GPSALIGN_TOTAL_SCALE", "LIO_GPSALIGN_TOTAL_T", "LIO_SIM2D_LEN"):
        assert re.search(r"#define\s+" + macro + r"\b", src), macro
    args, comment = _decl(src, "lio_similarity2d_fit")
    assert len(args.split(",")) == 5 and "align_trajectories_horn" in comment and "TREE" in comment
    args, comment = _decl(src, "lio_georeference_xy")
    assert len(args.split(",")) == 10 and "const double* origin2_opt" in args and "double* xy_out_opt" in args
    assert "((x r00) + (y r01)) scale + tx - ox" in comment and "6 cm" in comment and "bit-copied" in comment


def test_header_offsets_match_the_binding():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    for name in dir(_capi):
        if name.startswith("GPSALIGN_"):
            m = re.search(r"#define\s+LIO_" + name + r"\s+(\d+)", src)
            assert m and int(m.group(1)) == getattr(_capi, name), name
    assert int(re.search(r"#define\s+LIO_GPSALIGN_LEN\s+(\d+)", src).group(1)) == _capi.LIO_GPSALIGN_LEN
    assert int(re.search(r"#define\s+LIO_SIM2D_LEN\s+(\d+)", src).group(1)) == _capi.LIO_SIM2D_LEN
    # plain arrays, no new public struct: the ABI guard lists the same 15 structs as before
    assert _capi.lib().lio_abi_struct_sizes(None, 0) == 15 == len(_capi._ABI_STRUCTS)


def test_symbols_are_exported_and_bound():
    L = _capi.lib()
    for name, nargs in NAMES.items():
        assert name in _capi.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes and len(fn.argtypes) == nargs and fn.restype is C.c_int


def test_python_mirrors_exist_with_the_reference_defaults():
    from lio_gpu import georef as G
    from lio_gpu.filters import _Handle

    assert issubclass(G.GpsAligner, _Handle) and hasattr(G.GpsAligner, "align")
    sig = inspect.signature(G.GpsAligner.__init__)
    assert sig.parameters["max_iterations"].default == 50 and sig.parameters["tolerance"].default == 1e-4
    assert sig.parameters["device"].default == 0
    sig = inspect.signature(G.georeference)
    assert sig.parameters["origin"].default == (0.0, 0.0) and sig.parameters["return_f64"].default is False
    assert list(inspect.signature(G.fit_pairs).parameters)[:2] == ["src", "dst"]
    assert list(inspect.signature(G.georeference_pcd).parameters)[:3] == ["in_path", "params_path", "out_path"]
    for field in ("aligned", "nn", "iterations", "converged", "mean_error", "total", "reference_return"):
        assert field in G.GpsAlignResult.__dataclass_fields__, field
    assert "cannot parse" in G.write_georef_params.__doc__


def test_params_file_round_trip_in_the_readers_format(tmp_path):
    from lio_gpu import georef as G

    p = str(tmp_path / "georef_params.txt")
    scale, R, t = 1.0200000000000002, np.array([[0.8253356149096783, -0.5646424733950354], [0.5646424733950354, 0.8253356149096783]]), \
        np.array([836000.1234567891, 818000.9876543219])
    G.write_georef_params(p, scale, R, t)
    s2, R2, t2 = G.read_georef_params(p)
    assert s2 == scale and np.array_equal(R2, R) and np.array_equal(t2, t)
    # the layout georeference_pcd.py:6-26 parses: comment lines, then scale / r11 r12 / r21 r22 / t1 t2
    lines = [ln.strip() for ln in open(p) if not ln.startswith("#")]
    assert len(lines) == 4 and float(lines[0]) == scale and [len(ln.split()) for ln in lines] == [1, 2, 2, 2]
    open(p, "w").write("# only\n1.0\n1 0\n")
    with pytest.raises(ValueError):
        G.read_georef_params(p)


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    body = src[src.index("class GpsAligner"):]
    body = body[:body.index("\n};")]
    for m in ("setMaxIterations", "setTolerance", "align(", "iterations()", "converged()", "meanError()", "nearest()",
              "total()", "referenceReturn()", "lio_gps_align("):
        assert m in body, m
    assert "lio_similarity2d_fit(" in src and "lio_georeference_xy(" in src and "struct Similarity2D" in src
    mk = open(os.path.join(ROOT, "fast-lio-sam_gps_amd", "Makefile")).read()
    assert "gps_align_api" in mk and "csrc/lio_gpsalign.hip" in mk


def test_entries_fail_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    from lio_gpu import georef as G

    xy = np.zeros((8, 2))
    out = np.zeros(_capi.LIO_GPSALIGN_LEN)
    rc = L.lio_gps_align(None, xy.ctypes.data_as(dp), 8, xy.ctypes.data_as(dp), 8, 50, 1e-4, xy.ctypes.data_as(dp), None,
                         out.ctypes.data_as(dp))
    assert rc == _capi.LIO_ERR_NODEV
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    assert L.lio_similarity2d_fit(None, xy.ctypes.data_as(dp), xy.ctypes.data_as(dp), 8, out.ctypes.data_as(dp)) == _capi.LIO_ERR_NODEV
    pts = np.zeros((8, 4), np.float32)
    R = np.eye(2).ravel()
    rc = L.lio_georeference_xy(None, pts.ctypes.data_as(_capi.fp), 8, 4, 1.0, R.ctypes.data_as(dp), R.ctypes.data_as(dp), None,
                               pts.ctypes.data_as(_capi.fp), None)
    assert rc == _capi.LIO_ERR_NODEV
    with pytest.raises(_capi.LioError) as e:
        G.GpsAligner()
    assert e.value.code == _capi.LIO_ERR_NODEV
    with pytest.raises(_capi.LioError) as e:
        G.fit_pairs(xy, xy)
    assert e.value.code == _capi.LIO_ERR_NODEV
