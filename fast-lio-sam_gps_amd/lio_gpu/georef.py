"""GPS-to-SLAM trajectory alignment and map georeferencing: the reference's offline GPS leg over the C-ABI.

* :class:`GpsAligner` — ``icp_alignment`` (post_process/align_slam_gps_icp.py:81-156): a 2-D similarity, with
  scale, between the SLAM trajectory and the projected GPS track by point-to-point ICP (``lio_gps_align``)
* :func:`fit_pairs` — ``align_trajectories_horn`` (georef_mapmatch.py:115-135) on timestamp-matched pairs
  (``lio_similarity2d_fit``)
* :func:`georeference`, :func:`georeference_pcd` — the map transform of post_process/georeference_pcd.py:236-244
  (``lio_georeference_xy``)
* :func:`read_georef_params`, :func:`write_georef_params` — the four-line parameter file of
  georeference_pcd.py:6-26

Coordinates are already projected (WGS84 to a national grid or UTM is pyproj's job).  Every result follows the
contract of include/lio_gpu.h bit for bit: IEEE double operations in a written order, sums by TREE.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import check, lib
from .filters import _Handle, _fp, _rows

_dp = C.POINTER(C.c_double)


def _xy(a, what):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{what}: an (n, 2) array of projected coordinates is expected")
    return a


def _rot(c, s):
    return np.array([[c, -s], [s, c]], np.float64)


@dataclass
class Similarity2D:
    """``dst = scale * R @ src + t``"""
    scale: float
    R: np.ndarray
    t: np.ndarray

    def apply(self, xy):
        return self.scale * (np.asarray(xy, np.float64) @ self.R.T) + self.t


@dataclass
class GpsAlignResult:
    """``aligned``: the SLAM points in the GPS frame; ``nn``: per SLAM point the index of its GPS point in the last
    iteration; ``total``: the similarity that maps the input ``slam_xy`` to ``aligned`` — the one to georeference
    with; ``reference_return``: what the reference's ``icp_alignment`` returns, which chains only the LAST
    iteration's increment with the initial scale (a quirk of the script, kept under that name for comparison);
    ``out``: the raw ``LIO_GPSALIGN_*`` array."""
    aligned: np.ndarray
    nn: np.ndarray
    iterations: int
    converged: bool
    mean_error: float
    total: Similarity2D
    reference_return: Similarity2D
    out: np.ndarray


class GpsAligner(_Handle):
    """``icp_alignment(gps_coords_2d, slam_coords_2d, max_iterations=50, tolerance=1e-4)`` by the contract of
    ``lio_gps_align``: nearest neighbours by squared distance with the lowest index on a tie, the rotation in
    closed form, the reference's norm-ratio scale, convergence on the change of the mean distance."""

    def __init__(self, max_iterations: int = 50, tolerance: float = 1e-4, device: int = 0):
        super().__init__(device)
        self.max_iterations = int(max_iterations)
        self.tolerance = float(tolerance)

    def align(self, gps_xy, slam_xy) -> GpsAlignResult:
        gps, slam = _xy(gps_xy, "gps_xy"), _xy(slam_xy, "slam_xy")
        n = len(slam)
        aligned = np.zeros((n, 2), np.float64)
        nn = np.zeros(n, np.int32)
        out = np.zeros(_capi.LIO_GPSALIGN_LEN, np.float64)
        check(lib().lio_gps_align(self._h, gps.ctypes.data_as(_dp), len(gps), slam.ctypes.data_as(_dp), n,
                                  self.max_iterations, self.tolerance, aligned.ctypes.data_as(_dp),
                                  nn.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(_dp)))
        G = _capi
        return GpsAlignResult(
            aligned=aligned + out[G.GPSALIGN_CB:G.GPSALIGN_CB + 2], nn=nn, iterations=int(out[G.GPSALIGN_ITERATIONS]),
            converged=bool(out[G.GPSALIGN_CONVERGED]), mean_error=float(out[G.GPSALIGN_MEAN_ERROR]),
            total=Similarity2D(float(out[G.GPSALIGN_TOTAL_SCALE]), _rot(out[G.GPSALIGN_TOTAL_C], out[G.GPSALIGN_TOTAL_S]),
                               out[G.GPSALIGN_TOTAL_T:G.GPSALIGN_TOTAL_T + 2].copy()),
            reference_return=Similarity2D(float(out[G.GPSALIGN_REF_SCALE]), _rot(out[G.GPSALIGN_REF_C], out[G.GPSALIGN_REF_S]),
                                          out[G.GPSALIGN_REF_T:G.GPSALIGN_REF_T + 2].copy()),
            out=out)


def fit_pairs(src, dst, handle: _Handle | None = None) -> Similarity2D:
    """``align_trajectories_horn``: the similarity ``dst ~ scale * R @ src + t`` of n pairs matched one to one
    (by timestamp, in the reference), with the norm-ratio scale of ``lio_gps_align``'s iteration."""
    h = handle or _Handle()
    s, d = _xy(src, "src"), _xy(dst, "dst")
    if len(s) != len(d):
        raise ValueError("fit_pairs: src and dst must have the same length")
    out = np.zeros(_capi.LIO_SIM2D_LEN, np.float64)
    check(lib().lio_similarity2d_fit(h._h, s.ctypes.data_as(_dp), d.ctypes.data_as(_dp), len(s), out.ctypes.data_as(_dp)))
    return Similarity2D(float(out[0]), _rot(out[1], out[2]), out[3:5].copy())


def georeference(pts, scale, R, t, origin=(0.0, 0.0), return_f64: bool = False, handle: _Handle | None = None):
    """Point records (n x stride float32, x, y, z first) with x, y moved by ``(x, y) @ R.T * scale + t - origin``,
    computed in double from the float32 x, y; every other field is copied bit for bit.  ``origin = (0, 0)`` is the
    reference's behaviour: at national-grid magnitudes (HK1980: about 8e5 m) float32 x, y then quantise to 6 cm.
    A non-zero ``origin`` near the map keeps the float32 records fine-grained.  ``return_f64``: also the n x 2
    georeferenced coordinates at full precision."""
    h = handle or _Handle()
    p = _rows(pts)
    n = len(p)
    R4 = np.ascontiguousarray(np.asarray(R, np.float64).reshape(4))
    t2 = np.ascontiguousarray(np.asarray(t, np.float64).reshape(2))
    o2 = np.ascontiguousarray(np.asarray(origin, np.float64).reshape(2))
    out = np.empty_like(p)
    xy = np.zeros((n, 2), np.float64) if return_f64 else None
    check(lib().lio_georeference_xy(h._h, _fp(p), n, p.shape[1], float(scale), R4.ctypes.data_as(_dp), t2.ctypes.data_as(_dp),
                                    o2.ctypes.data_as(_dp), _fp(out), xy.ctypes.data_as(_dp) if return_f64 else None))
    return (out, xy) if return_f64 else out


def read_georef_params(path: str):
    """(scale, R 2x2, t 2) from the four-line file georeference_pcd.py:6-26 reads: lines starting with ``#`` are
    skipped, then ``scale``, ``r11 r12``, ``r21 r22``, ``t1 t2``."""
    with open(path) as f:
        lines = [ln.strip() for ln in f if not ln.startswith("#")]
    if len(lines) < 4:
        raise ValueError(f"{path}: four data lines expected (scale, two rotation rows, translation)")
    try:
        scale = float(lines[0])
        R = np.array([[float(v) for v in lines[1].split()], [float(v) for v in lines[2].split()]], np.float64)
        t = np.array([float(v) for v in lines[3].split()], np.float64)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    if R.shape != (2, 2) or t.shape != (2,):
        raise ValueError(f"{path}: two numbers per rotation row and per translation expected")
    return scale, R, t


def write_georef_params(path: str, scale, R, t):
    """The file :func:`read_georef_params` and georeference_pcd.py:6-26 read, numbers with 17 significant digits
    (a double survives the round trip).  The reference's own writer (align_slam_gps_icp.py:269-281) emits a
    labelled layout that its reader cannot parse; this one writes what the reader expects."""
    R = np.asarray(R, np.float64).reshape(2, 2)
    t = np.asarray(t, np.float64).reshape(2)
    with open(path, "w") as f:
        f.write("# scale / rotation row 1 / rotation row 2 / translation\n")
        f.write(f"{float(scale):.17g}\n{R[0, 0]:.17g} {R[0, 1]:.17g}\n{R[1, 0]:.17g} {R[1, 1]:.17g}\n{t[0]:.17g} {t[1]:.17g}\n")


def georeference_pcd(in_path: str, params_path: str, out_path: str, origin=(0.0, 0.0),
                     fields=("x", "y", "z", "intensity")) -> int:
    """``georeference_pcd.py <in> <params> <out>``: reads the float columns ``fields`` of a PCD file, moves x, y by
    the similarity of ``params_path`` and writes a binary PCD.  Returns the point count."""
    from . import formats

    scale, R, t = read_georef_params(params_path)
    codec = formats.CloudCodec()
    try:
        rec = codec.read_pcd(in_path, want=fields)
        out = georeference(rec, scale, R, t, origin=origin, handle=codec) if len(rec) else rec
        formats.write_pcd_binary(out_path, out, names=fields)
    finally:
        codec.close()
    return len(rec)
