"""Point-cloud filters around the hot path, over the C-ABI.

* :class:`VoxelGrid` — ``pcl::VoxelGrid<PointT>`` (PCL 1.10 ``applyFilter``):
  FAST-LIO's ``downSizeFilterSurf`` and the loop closure's ``voxelizePcd``
  (/root/reference/fast_lio_sam/include/utilities.hpp:161-183)
* :func:`voxelize_submap` — one side of ``LoopClosure::setSrcAndDstCloud``
  (loop_closure.cpp:42-67): ``transformPcd`` (utilities.hpp:132-143) per
  keyframe, concatenation, ``voxelizePcd``
* :class:`ScanPreprocessor` — FAST-LIO ``Preprocess`` selection +
  ``ImuProcess::UndistortPcl`` + ``downSizeFilterSurf`` for one raw scan
* :class:`StatisticalOutlierRemoval`, :func:`radius_first_seed`, :func:`denoise_slam_map` — the back
  end's intensity denoise (fast_lio_sam.cpp:941-1008, 575-646, 332-365) and its parts
* :class:`EuclideanClusterExtraction` — ``pcl::EuclideanClusterExtraction`` with one axis-aligned bounding
  box per cluster (fast_lio_sam.cpp:343-363, post_process/clustering.py:39-75)
* :class:`DBSCAN` — the offline pipeline's other clustering method (post_process/clustering.py:30-36), with
  core flags and one box per cluster
* :class:`KMeans`, :func:`cluster_palette` — the projection tool's ``cv::kmeans`` call and its cluster colours
  (post_process/lidar_projection/src/lidar_projection.cpp:82-92, 36-52)
* :class:`NormalEstimation`, :func:`with_normals` — ``pcl::NormalEstimation`` / Open3D ``estimate_normals``: the
  normal and curvature fields of the map's PointXYZINormal records, which the reference saves empty

Point records are float rows ``[x, y, z, attr...]`` (3..8 floats); PCL's
PointXYZI is ``stride = 4``, FAST-LIO's PointXYZINormal-with-time is
``[x, y, z, intensity, time_ms]`` (time = the reference's ``curvature``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class _Handle:
    """A handle of the C-ABI: a ``lio_filter``, or what a subclass names in ``_create`` / ``_destroy`` (``args``: what
    its create takes between ``device`` and ``out``)."""
    _create, _destroy = "lio_filter_create", "lio_filter_destroy"

    def __init__(self, device: int = 0, *args):
        self._h = C.c_void_p()
        check(getattr(lib(), self._create)(device, *args, C.byref(self._h)))

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def _timing(self, fn: str, names) -> dict:
        """``names`` -> the device ms of the last call's stages, from the handle's ``get_timing``"""
        ms = np.zeros(len(names), np.float64)
        check(getattr(lib(), fn)(self._h, ms.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(zip(names, (float(v) for v in ms)))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VoxelGrid(_Handle):
    """``pcl::VoxelGrid``: every field averaged per voxel, output in voxel-index order."""

    def __init__(self, leaf=0.5, device: int = 0):
        super().__init__(device)
        self.setLeafSize(*(np.broadcast_to(np.asarray(leaf, np.float32), 3)))

    def setLeafSize(self, lx, ly, lz):
        self.leaf = np.array([lx, ly, lz], np.float32)

    def filter(self, pts: np.ndarray) -> np.ndarray:
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        pts2 = pts.reshape(len(pts), -1)
        stride = pts2.shape[1]
        out = np.empty_like(pts2)
        m = C.c_int64(0)
        check(lib().lio_voxel_grid(self._h, _fp(pts2), len(pts2), stride, _fp(self.leaf), _fp(out), C.byref(m)))
        return out[: m.value].copy()


def _rows(pts):
    """float32 records as a contiguous (n, stride) array (an empty cloud keeps its stride)"""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    if pts.size == 0:
        return pts.reshape(0, pts.shape[-1] if pts.ndim > 1 and pts.shape[-1] else 3)
    return pts.reshape(len(pts), -1)


class StatisticalOutlierRemoval(_Handle):
    """``pcl::StatisticalOutlierRemoval``: the mean distance to the ``mean_k`` nearest neighbours per point,
    points farther than ``mean + stddev_mul * stddev`` removed (``negative``: the others), order kept.
    After :meth:`filter`: ``distances`` (per input point, 0 where not counted) and ``stats`` = mean, stddev,
    threshold, counted points."""

    def __init__(self, mean_k: int = 50, stddev_mul: float = 1.0, negative: bool = False, device: int = 0):
        super().__init__(device)
        self.setMeanK(mean_k)
        self.setStddevMulThresh(stddev_mul)
        self.setNegative(negative)
        self.distances = np.zeros(0, np.float32)
        self.stats = np.full(4, np.nan)

    def setMeanK(self, k):
        self.mean_k = int(k)

    def setStddevMulThresh(self, m):
        self.stddev_mul = float(m)

    def setNegative(self, negative):
        self.negative = bool(negative)

    def filter(self, pts: np.ndarray) -> np.ndarray:
        pts2 = _rows(pts)
        out = np.empty_like(pts2)
        self.distances = np.zeros(len(pts2), np.float32)
        self.stats = np.zeros(4, np.float64)
        m = C.c_int64(0)
        check(lib().lio_sor_filter(self._h, _fp(pts2), len(pts2), pts2.shape[1], self.mean_k, self.stddev_mul,
                                   int(self.negative), _fp(out), C.byref(m), _fp(self.distances),
                                   self.stats.ctypes.data_as(C.POINTER(C.c_double))))
        return out[: m.value].copy()


def radius_first_seed(pts, seeds_xyz, radius: float, handle: _Handle | None = None):
    """Per cloud point the lowest seed index within ``radius`` (strict, float squared distances; -1: none)
    and that squared distance: ``KdTreeFLANN::radiusSearch`` per seed, turned round."""
    h = handle or _Handle()
    pts2 = _rows(pts)
    seeds = np.ascontiguousarray(np.asarray(seeds_xyz, np.float32).reshape(-1, 3))
    seed = np.full(len(pts2), -1, np.int32)
    d2 = np.zeros(len(pts2), np.float32)
    check(lib().lio_radius_first_seed(h._h, _fp(pts2), len(pts2), pts2.shape[1], _fp(seeds),
                                      len(seeds), float(radius), seed.ctypes.data_as(C.POINTER(C.c_int32)), _fp(d2)))
    return seed, d2


def denoise_slam_map(pts, seed_thres=2800.0, cluster_seed_radius=1.0, denoise_radius=0.5, noise_thres=2700.0,
                     mean_k=50, stddev_mul=1.0, handle: _Handle | None = None):
    """``FastLioSam::denoise_slam_map`` (fast_lio_sam.cpp:941-1008) on ``[x, y, z, intensity]`` rows; the
    defaults are the reference's (fast_lio_sam.cpp:89-96; its config.yaml sets 0.1, 200 and 0.2).
    Returns the denoised map (denoised segment, then the remained points) and ``counts`` = seeds, segmented,
    after SOR, denoised, remained."""
    h = handle or _Handle()
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
    out = np.empty_like(pts)
    counts = np.zeros(5, np.int64)
    m = C.c_int64(0)
    p = _capi.DenoiseParams(seed_thres, cluster_seed_radius, denoise_radius, noise_thres, int(mean_k), stddev_mul)
    check(lib().lio_denoise_slam_map(h._h, _fp(pts), len(pts), C.byref(p), _fp(out), C.byref(m),
                                     counts.ctypes.data_as(C.POINTER(C.c_int64))))
    return out[: m.value].copy(), counts


def _cluster_call(entry, handle, pts, params, cap_clusters, with_core):
    """Allocates the outputs of ``lio_euclidean_clusters`` / ``lio_dbscan`` (``entry``; ``params`` are its arguments
    between the stride and ``labels_out``), calls it and slices the result: the cluster count, labels, core flags
    (``None`` without ``with_core``), offsets, indices, boxes, stats and the list of index arrays."""
    pts2 = _rows(pts)
    n = len(pts2)
    cap = n if cap_clusters is None else int(cap_clusters)
    labels = np.full(n, -1, np.int32)
    core = np.zeros(n, np.uint8) if with_core else None
    offsets = np.zeros(max(cap, 0) + 1, np.int64)
    indices = np.zeros(n, np.int32)
    aabb = np.zeros((max(cap, 0), 6), np.float32)
    stats = np.zeros(4, np.int64)
    m = C.c_int64(0)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    core_arg = (core.ctypes.data_as(C.POINTER(C.c_uint8)),) if with_core else ()
    check(entry(handle, _fp(pts2), n, pts2.shape[1], *params, labels.ctypes.data_as(i32p), *core_arg, C.byref(m), cap,
                offsets.ctypes.data_as(i64p), indices.ctypes.data_as(i32p), _fp(aabb), stats.ctypes.data_as(i64p)))
    k = min(m.value, cap)
    offsets, indices = offsets[: k + 1].copy(), indices[: stats[3]].copy()
    return (m.value, labels, core, offsets, indices, aabb[:k].copy(), stats,
            [indices[offsets[t]:offsets[t + 1]] for t in range(k)])


class EuclideanClusterExtraction(_Handle):
    """``pcl::EuclideanClusterExtraction``: the connected components of the graph that joins two finite points
    closer than ``tolerance`` (strict, float squared distances), those with ``min_size <= size <= max_size``
    kept, ordered by size descending, then by lowest member index; indices ascend inside a cluster.  The
    defaults are PCL's (tolerance 0 — an argument error until set —, min 1, max ``INT_MAX``); the reference's
    commented block uses 0.5, 10, 25000 (fast_lio_sam.cpp:343-363).
    After :meth:`extract`: ``labels`` (per input point the cluster rank, -1: none), ``offsets`` / ``indices``
    (cluster k is ``indices[offsets[k]:offsets[k + 1]]``), ``aabb`` (per cluster min x, y, z, max x, y, z:
    post_process/clustering.py:72-75) and ``stats`` = finite points, components, accepted clusters, points in
    them."""

    def __init__(self, tolerance: float = 0.0, min_size: int = 1, max_size: int = 2**31 - 1, device: int = 0):
        super().__init__(device)
        self.setClusterTolerance(tolerance)
        self.setMinClusterSize(min_size)
        self.setMaxClusterSize(max_size)
        self.n_clusters = 0  # accepted clusters of the last extract(), whatever its cap_clusters
        self.labels = np.zeros(0, np.int32)
        self.offsets = np.zeros(1, np.int64)
        self.indices = np.zeros(0, np.int32)
        self.aabb = np.zeros((0, 6), np.float32)
        self.stats = np.zeros(4, np.int64)

    def setClusterTolerance(self, tolerance):
        self.tolerance = float(tolerance)

    def setMinClusterSize(self, min_size):
        self.min_size = int(min_size)

    def setMaxClusterSize(self, max_size):
        self.max_size = int(max_size)

    def extract(self, pts: np.ndarray, cap_clusters: int | None = None) -> list:
        """The list of index arrays.  ``cap_clusters`` (default: as many as there can be) bounds the clusters
        that ``offsets`` / ``aabb`` and the returned list describe; ``labels``, ``indices`` and ``stats`` are
        always complete."""
        (self.n_clusters, self.labels, _, self.offsets, self.indices, self.aabb, self.stats, clusters) = _cluster_call(
            lib().lio_euclidean_clusters, self._h, pts, (self.tolerance, self.min_size, self.max_size), cap_clusters, False)
        return clusters


class DBSCAN(_Handle):
    """DBSCAN as the offline pipeline's ``cluster_with_dbscan`` calls it (post_process/clustering.py:30-36), by
    the contract of ``lio_dbscan``: finite points are neighbours when their float squared distance is
    ``<= eps * eps`` (inclusive, itself counted), a point with ``min_samples`` neighbours is core, a cluster is a
    connected component of the core points, numbered by its lowest core index; a border point takes the
    lowest-numbered cluster among its core neighbours'; everything else is noise (-1).  The defaults are
    scikit-learn's (0.5, 5); the reference's call uses 0.5, 10.
    After :meth:`fit`: ``labels_``, ``core_sample_indices_`` (scikit-learn's names), ``n_clusters``, ``offsets`` /
    ``indices`` (cluster k is ``indices[offsets[k]:offsets[k + 1]]``), ``aabb`` (per cluster min x, y, z, max x, y,
    z over all members) and ``stats`` = finite points, core points, clusters, clustered points."""

    def __init__(self, eps: float = 0.5, min_samples: int = 5, device: int = 0):
        super().__init__(device)
        self.eps = float(eps)
        self.min_samples = int(min_samples)
        self.n_clusters = 0  # clusters of the last fit(), whatever its cap_clusters
        self.labels_ = np.zeros(0, np.int32)
        self.core_sample_indices_ = np.zeros(0, np.int64)
        self.offsets = np.zeros(1, np.int64)
        self.indices = np.zeros(0, np.int32)
        self.aabb = np.zeros((0, 6), np.float32)
        self.stats = np.zeros(4, np.int64)

    def fit(self, pts: np.ndarray, cap_clusters: int | None = None) -> list:
        """The list of index arrays.  ``cap_clusters`` (default: as many as there can be) bounds the clusters
        that ``offsets`` / ``aabb`` and the returned list describe; ``labels_``, ``core_sample_indices_``,
        ``indices`` and ``stats`` are always complete."""
        (self.n_clusters, self.labels_, core, self.offsets, self.indices, self.aabb, self.stats, clusters) = _cluster_call(
            lib().lio_dbscan, self._h, pts, (self.eps, self.min_samples), cap_clusters, True)
        self.core_sample_indices_ = np.flatnonzero(core).astype(np.int64)
        return clusters


def sample_triples(seed: int, n: int, num_iterations: int) -> np.ndarray:
    """The built-in sampler of :class:`PlaneSegmentation` (``lio_plane_sample_triples``; host only):
    ``num_iterations`` triples of distinct indices in ``[0, n)``; none for ``n < 3``."""
    k = int(num_iterations) if n >= 3 else 0
    out = np.zeros((k, 3), np.int32)
    check(lib().lio_plane_sample_triples(int(seed) & (2**64 - 1), int(n), int(num_iterations),
                                         out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


class PlaneSegmentation(_Handle):
    """Open3D's ``PointCloud.segment_plane`` as the offline pipeline calls it for ground removal
    (post_process/clustering.py:21-28), as the contract of ``lio_segment_plane``: every one of the
    ``num_iterations`` three-point hypotheses is scored against every point (strict float distance below
    ``distance_threshold``), and the winner minimises (-inliers, fixed-point squared error, hypothesis index).
    The triples come from ``triples`` (``K x 3``) or from the built-in sampler with ``seed``.
    After :meth:`segment_plane`: ``best_iteration`` (-1: no plane), ``counts`` / ``sq`` / ``degenerate`` (per
    hypothesis), ``mask`` (per input point) and ``refit`` (the least-squares plane through the inliers, 4
    doubles)."""

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.best_iteration = -1
        self.counts = np.zeros(0, np.int64)
        self.sq = np.zeros(0, np.uint64)
        self.degenerate = np.zeros(0, np.uint8)
        self.mask = np.zeros(0, np.uint8)
        self.refit = np.zeros(4, np.float64)

    def segment_plane(self, pts: np.ndarray, distance_threshold: float = 0.2, ransac_n: int = 3,
                      num_iterations: int = 1000, seed: int = 0, triples=None):
        """``(plane4, inliers)``: float32 (a, b, c, d) and the inliers' indices ascending."""
        pts2 = _rows(pts)
        n, k = len(pts2), max(int(num_iterations), 0)
        plane = np.zeros(4, np.float32)
        inliers = np.zeros(n, np.int32)
        counts, sq = np.zeros(k, np.int64), np.zeros(k, np.uint64)
        degenerate, mask = np.zeros(k, np.uint8), np.zeros(n, np.uint8)
        refit = np.zeros(4, np.float64)
        best, m = C.c_int64(-1), C.c_int64(0)
        tri = None
        if triples is not None:
            tri = np.ascontiguousarray(triples, dtype=np.int32)
            if tri.shape != (int(num_iterations), 3):
                raise ValueError("triples must be num_iterations x 3")
        i32p, i64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
        check(lib().lio_segment_plane(self._h, _fp(pts2), n, pts2.shape[1], float(distance_threshold), int(ransac_n),
                                      int(num_iterations), int(seed) & (2**64 - 1),
                                      tri.ctypes.data_as(i32p) if tri is not None else None, _fp(plane), C.byref(best),
                                      inliers.ctypes.data_as(i32p), C.byref(m), mask.ctypes.data_as(u8p),
                                      counts.ctypes.data_as(i64p), sq.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      degenerate.ctypes.data_as(u8p), refit.ctypes.data_as(C.POINTER(C.c_double))))
        self.best_iteration = best.value
        self.counts, self.sq, self.degenerate, self.mask, self.refit = counts, sq, degenerate, mask, refit
        return plane, inliers[: m.value].copy()


class KMeans(_Handle):
    """``cv::kmeans`` as the reference's projection tool calls it (post_process/lidar_projection/src/
    lidar_projection.cpp:82-92: 5 clusters, ``TermCriteria(EPS + MAX_ITER, 100, 0.1)``, 3 attempts, k-means++
    centres), by the contract of ``lio_kmeans``: k-means++ seeding with three trials per centre from a
    counter-based sampler, Lloyd iterations on fixed-point sums (so no result depends on the device's schedule),
    empty clusters repaired from the largest one, the attempt with the smallest compactness kept.  It follows
    OpenCV's procedure; it is not bit parity with it.  Centres are float32: subtract an origin from map coordinates
    first (:func:`lio_gpu.georef.georeference_xy` offers one).
    After :meth:`fit`: ``labels_`` (-1 for a non-finite point), ``cluster_centers_``, ``inertia_`` (the
    compactness; scikit-learn's names), ``n_iter_``, ``best_attempt``, ``counts``, ``aabb`` (per cluster min x, y,
    z, max x, y, z), ``seeds`` (attempts x K point indices, -1 with ``init_centers``), ``attempt_q`` /
    ``attempt_iters`` (per attempt) and ``stats`` = finite points, best attempt, its iterations, repairs, ec, ed."""

    def __init__(self, n_clusters: int = 5, max_iter: int = 100, eps: float = 0.1, attempts: int = 3, seed: int = 0,
                 device: int = 0):
        super().__init__(device)
        self.n_clusters = int(n_clusters)
        self.max_iter = int(max_iter)
        self.eps = float(eps)
        self.attempts = int(attempts)
        self.seed = int(seed)
        self.labels_ = np.zeros(0, np.int32)
        self.cluster_centers_ = np.zeros((0, 3), np.float32)
        self.inertia_ = 0.0
        self.n_iter_ = 0
        self.best_attempt = 0
        self.counts = np.zeros(0, np.int64)
        self.aabb = np.zeros((0, 6), np.float32)
        self.seeds = np.zeros((0, 0), np.int32)
        self.attempt_q = np.zeros(0, np.uint64)
        self.attempt_iters = np.zeros(0, np.int32)
        self.stats = np.zeros(6, np.int64)

    def fit(self, pts: np.ndarray, init_centers=None) -> np.ndarray:
        """The labels.  ``init_centers`` (attempts x K x 3) replaces the seeding of every attempt."""
        pts2 = _rows(pts)
        n, k, a = len(pts2), max(self.n_clusters, 0), max(self.attempts, 0)
        init = None
        if init_centers is not None:
            init = np.ascontiguousarray(init_centers, dtype=np.float32)
            if init.shape != (a, k, 3):
                raise ValueError("init_centers must be attempts x n_clusters x 3")
        labels = np.full(n, -1, np.int32)
        centers = np.zeros((k, 3), np.float32)
        counts, aabb = np.zeros(k, np.int64), np.zeros((k, 6), np.float32)
        seeds = np.full((a, k), -1, np.int32)
        attempt_q, attempt_iters = np.zeros(a, np.uint64), np.zeros(a, np.int32)
        stats = np.zeros(6, np.int64)
        compactness = C.c_double(0.0)
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        check(lib().lio_kmeans(self._h, _fp(pts2), n, pts2.shape[1], self.n_clusters, self.max_iter, self.eps,
                               self.attempts, self.seed & (2**64 - 1), _fp(init) if init is not None else None,
                               labels.ctypes.data_as(i32p), _fp(centers), C.byref(compactness),
                               counts.ctypes.data_as(i64p), _fp(aabb), seeds.ctypes.data_as(i32p),
                               attempt_q.ctypes.data_as(C.POINTER(C.c_uint64)), attempt_iters.ctypes.data_as(i32p),
                               stats.ctypes.data_as(i64p)))
        self.labels_, self.cluster_centers_, self.inertia_ = labels, centers, compactness.value
        self.counts, self.aabb, self.seeds = counts, aabb, seeds
        self.attempt_q, self.attempt_iters, self.stats = attempt_q, attempt_iters, stats
        self.best_attempt, self.n_iter_ = int(stats[1]), int(stats[2])
        return labels


class NormalEstimation(_Handle):
    """``pcl::NormalEstimation`` (``k``: ``setKSearch``; ``radius``: ``setRadiusSearch``) and, with both set,
    Open3D's hybrid search of ``estimate_normals``, by the contract of ``lio_estimate_normals``: the neighbours are
    the ``k`` nearest under (float squared distance, index) and / or the points strictly within ``radius``, the
    covariance comes from integer moments, the normal is the eigenvector of its smallest eigenvalue (cyclic Jacobi
    in double) and the curvature that eigenvalue over the trace.  It follows PCL's procedure; it is not bit parity
    with it.  The default is Open3D's and PCL's customary 20 neighbours.
    After :meth:`compute`: ``curvature`` (n float32), ``counts`` (n: the neighbours used, the point itself
    included) and ``stats`` = finite points, points with a normal, finite points with fewer than 3 neighbours,
    degenerate points, the largest neighbourhood, the sum of all.  A point without a normal has NaN."""

    def __init__(self, k: int = 20, radius: float = 0.0, device: int = 0):
        super().__init__(device)
        self.k = int(k)
        self.radius = float(radius)
        self.curvature = np.zeros(0, np.float32)
        self.counts = np.zeros(0, np.int32)
        self.stats = np.zeros(6, np.int64)

    def compute(self, pts: np.ndarray, viewpoint=None) -> np.ndarray:
        """The normals (n x 3 float32).  ``viewpoint``: ``(3,)`` turns every normal towards that point, ``(n, 3)``
        each towards its own (the pose that saw the point); ``None``: the sign that makes ``n_z`` (then ``n_y``,
        then ``n_x``) positive."""
        pts2 = _rows(pts)
        n = len(pts2)
        vp, vp_stride = None, 0
        if viewpoint is not None:
            vp = np.ascontiguousarray(viewpoint, dtype=np.float32)
            if vp.shape == (n, 3) and vp.ndim == 2:
                vp_stride = 3
            elif vp.shape != (3,):
                raise ValueError("viewpoint must be (3,) or (n, 3)")
        normals = np.full((n, 3), np.nan, np.float32)
        curvature = np.full(n, np.nan, np.float32)
        counts = np.zeros(n, np.int32)
        stats = np.zeros(6, np.int64)
        check(lib().lio_estimate_normals(self._h, _fp(pts2), n, pts2.shape[1], self.radius, self.k,
                                         _fp(vp) if vp is not None else None, vp_stride, _fp(normals), _fp(curvature),
                                         counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                         stats.ctypes.data_as(C.POINTER(C.c_int64))))
        self.curvature, self.counts, self.stats = curvature, counts, stats
        return normals


# the float fields of FAST-LIO's PointXYZINormal, the rows of :func:`with_normals`
POINT_XYZI_NORMAL_FIELDS = ("x", "y", "z", "intensity", "normal_x", "normal_y", "normal_z", "curvature")


def with_normals(pts, normals, curvature) -> np.ndarray:
    """n x 8 float32 rows ``x y z intensity normal_x normal_y normal_z curvature`` — FAST-LIO's PointXYZINormal,
    which ``lio_gpu.formats.write_pcd_binary(path, rows, POINT_XYZI_NORMAL_FIELDS)`` (``lio_pcd_write_binary``)
    saves under those names — from ``pts`` (n x 3: intensity 0; n x 4 or wider: column 3), the normals (n x 3) and
    the curvature (n).  Host only."""
    pts2 = _rows(pts)
    n = len(pts2)
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)
    cur = np.asarray(curvature, np.float32).reshape(-1)
    if len(nrm) != n or len(cur) != n:
        raise ValueError("with_normals: one normal and one curvature per point")
    out = np.zeros((n, 8), np.float32)
    out[:, :3] = pts2[:, :3]
    if pts2.shape[1] > 3:
        out[:, 3] = pts2[:, 3]
    out[:, 4:7] = nrm
    out[:, 7] = cur
    return out


# the ten B, G, R colours of the projection tool's overlay (lidar_projection.cpp:38-49)
CLUSTER_PALETTE_BGR = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255),
                                (128, 0, 0), (0, 128, 0), (0, 0, 128), (128, 128, 0)], np.uint8)


def cluster_palette(labels) -> np.ndarray:
    """n x 3 uint8 B, G, R: the projection tool's colour of each point's cluster (``label % 10``), black for -1.
    Host only.  :func:`lio_gpu.camera.draw_points` draws with it (``colors=``), and
    :func:`lio_gpu.camera.lidar_projection_overlay` is the tool from its k-means to the finished image."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    out = CLUSTER_PALETTE_BGR[np.mod(lab, 10)]
    out[lab < 0] = 0
    return out


def cluster_objects(pts, nb_neighbors=20, std_ratio=2.0, distance_threshold=0.2, num_iterations=1000, seed=0,
                    tolerance=0.5, min_size=10, max_size=10000, method="euclidean", min_samples=10):
    """The main block of post_process/clustering.py (:77-118) on one handle's worth of device work: statistical
    outlier removal, ground-plane segmentation, the plane's inliers dropped, Euclidean clustering, one bounding
    box per cluster.  Every stage is this library's (the outlier removal with PCL's semantics, the plane by the
    contract of ``lio_segment_plane``, the clusters as PCL's).  Returns a dict: ``clusters`` (index arrays into the rows of ``pts``), ``aabb`` (per
    cluster min x, y, z, max x, y, z), ``plane`` (a, b, c, d), ``ground`` (rows of ``pts`` on the plane) and
    ``kept`` (rows of ``pts`` that passed the outlier removal).
    ``method="dbscan"`` (the script's other ``clustering_method``, :95-107) runs ``DBSCAN(tolerance, min_samples)``
    in place of the Euclidean stage — ``min_size`` / ``max_size`` are not used then — and adds ``noise``: the rows
    of ``pts`` that reached the clustering and were left in no cluster."""
    if method not in ("euclidean", "dbscan"):
        raise ValueError("cluster_objects: method must be 'euclidean' or 'dbscan'")
    pts2 = _rows(pts)
    sor = StatisticalOutlierRemoval(nb_neighbors, std_ratio)
    filtered = sor.filter(pts2)
    # removed when the distance is > the threshold: the kept rows, in input order
    kept = np.flatnonzero(~(sor.distances.astype(np.float64) > sor.stats[2])).astype(np.int64)
    if len(kept) != len(filtered):
        raise RuntimeError("cluster_objects: the outlier removal kept another number of rows than its distances say")
    sor.close()
    seg = PlaneSegmentation()
    plane, inl = seg.segment_plane(filtered, distance_threshold, 3, num_iterations, seed)
    seg.close()
    rest = np.flatnonzero(seg.mask == 0) if len(filtered) else np.zeros(0, np.int64)
    if method == "dbscan":
        db = DBSCAN(tolerance, min_samples)
        found = db.fit(filtered[rest])
        db.close()
        rows = kept[rest]
        return dict(clusters=[rows[c] for c in found], aabb=db.aabb, plane=plane, ground=kept[inl], kept=kept,
                    noise=rows[db.labels_ < 0])
    ec = EuclideanClusterExtraction(tolerance, min_size, max_size)
    found = ec.extract(filtered[rest])
    ec.close()
    rows = kept[rest]
    return dict(clusters=[rows[c] for c in found], aabb=ec.aabb, plane=plane, ground=kept[inl], kept=kept)


def voxelize_submap(clouds, poses, voxel_res: float, handle: VoxelGrid | None = None) -> np.ndarray:
    """``voxelizePcd(sum_k transformPcd(clouds[k], poses[k]), voxel_res)``; poses are 4x4 double."""
    h = handle or VoxelGrid(voxel_res)
    clouds = [np.ascontiguousarray(c, dtype=np.float32) for c in clouds]
    stride = clouds[0].shape[1] if clouds else 4
    seg = np.zeros(len(clouds) + 1, np.int64)
    for k, c in enumerate(clouds):
        seg[k + 1] = seg[k] + len(c)
    pts = np.ascontiguousarray(np.concatenate(clouds) if clouds else np.zeros((0, stride), np.float32))
    T = np.ascontiguousarray(np.stack([np.asarray(p, np.float64).reshape(4, 4) for p in poses])
                             if poses else np.zeros((0, 4, 4)), dtype=np.float64)
    out = np.empty((max(len(pts), 1), stride), np.float32)
    m = C.c_int64(0)
    check(lib().lio_submap_voxelize(h._h, _fp(pts), seg.ctypes.data_as(C.POINTER(C.c_int64)), len(clouds), stride,
                                    T.ctypes.data_as(C.POINTER(C.c_double)), float(voxel_res), _fp(out), C.byref(m)))
    return out[: m.value].copy()


def imu_poses_to_c(poses):
    """poses: list of dicts offset_time, acc, gyr, vel, pos, rot (3x3)  ->  ctypes array (lio_imu_pose is 22
    doubles in this order; filled through numpy, not element by element)."""
    n = len(poses)
    P = np.zeros((max(n, 1), 22), np.float64)
    for i, p in enumerate(poses):  # row slices assigned directly (no per-field temporaries)
        r = P[i]
        r[0] = p["offset_time"]
        r[1:4] = p["acc"]
        r[4:7] = p["gyr"]
        r[7:10] = p["vel"]
        r[10:13] = p["pos"]
        r[13:22] = np.ravel(p["rot"])
    assert C.sizeof(_capi.ImuPose) == 22 * 8
    return (_capi.ImuPose * max(n, 1)).from_buffer(P)


class ScanPreprocessor(_Handle):
    """Preprocess (point_filter_num, blind) + UndistortPcl + downSizeFilterSurf, to host memory."""

    def __init__(self, point_filter_num=4, blind=2.0, filter_size_surf=0.5, time_field=4, device: int = 0):
        super().__init__(device)
        self.params = _capi.ScanPrepParams(point_filter_num, blind, filter_size_surf, time_field)

    def process(self, raw: np.ndarray, imu_poses, end_pose) -> np.ndarray:
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        stride = raw.shape[1]
        out = np.empty_like(raw)
        m = C.c_int64(0)
        arr = imu_poses_to_c(imu_poses)
        check(lib().lio_preprocess(self._h, _fp(raw), len(raw), stride, C.byref(self.params), arr, len(imu_poses),
                                   C.byref(end_pose), _fp(out), C.byref(m)))
        return out[: m.value].copy()
