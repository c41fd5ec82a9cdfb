"""The contract of lio_gaussian_weights, lio_exposure_recover and lio_exposure_gaussian_blur (include/lio_gpu.h)
restated in numpy: the weights in Python floats (doubles) in the written order, everything else in int64.  The HSV
conversions are exposure_ref's.  No OpenCV.  CPU only; tests/test_overexposure_ref.py holds it against independent
formulations.  Also the images of the overexposure tests."""
import math

import numpy as np

import exposure_ref as ER

FIXED = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
         7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
PINNED_15 = [1, 3, 6, 12, 20, 30, 36, 40, 36, 30, 20, 12, 6, 3, 1]  # (15, 0), pinned by the contract
KSIZES = list(range(1, 32, 2))
SIGMAS = [0.0, 0.5, 2.6, 10.0]


def gaussian_weights(k, sigma=0.0):
    """k int64 weights with 8 fractional bits whose sum is 256"""
    assert k % 2 == 1 and 1 <= k <= 31 and math.isfinite(sigma)
    if sigma <= 0 and k <= 7:
        g = list(FIXED[k])
    else:
        s = sigma if sigma > 0 else ((k - 1) * 0.5 - 1.0) * 0.3 + 0.8
        scale2 = -0.5 / (s * s)
        t = []
        for i in range(k):
            x = i - (k - 1) * 0.5
            t.append(math.exp(scale2 * x * x))
        total = 0.0
        for v in t:  # from i = 0 up, one addition at a time
            total += v
        inv = 1.0 / total
        g = [v * inv for v in t]
    w = [0] * k
    err, left = 0.0, 0
    for i in range(k // 2):
        a = g[i] * 256.0 + err
        wi = round(a)  # Python's round: ties to even, as rint
        w[i] = w[k - 1 - i] = wi
        err = a - wi
        left += wi
    w[k // 2] = 256 - 2 * left
    return np.array(w, np.int64)


def refl(p, n):
    """REFLECT_101 applied until the index is in range; p an int array"""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    m = 2 * (n - 1)
    q = np.mod(p, m)  # non-negative
    return np.where(q < n, q, m - q)


def blur_plane(plane, w):
    """int plane (H x W, values 0..255) -> int64 plane: the row pass, then the column pass with the rounding"""
    plane = np.asarray(plane, np.int64)
    H, W = plane.shape
    k = len(w)
    r = k // 2
    hrow = np.zeros((H, W), np.int64)
    for j in range(k):
        hrow += int(w[j]) * plane[:, refl(np.arange(W) + j - r, W)]
    assert hrow.max() <= 65280
    acc = np.zeros((H, W), np.int64)
    for j in range(k):
        acc += int(w[j]) * hrow[refl(np.arange(H) + j - r, H), :]
    return (acc + 32768) >> 16


def dilate(mask, d):
    """the OR of a bool plane over |dx|, |dy| <= (d - 1) / 2, inside the image only"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    rd = (d - 1) // 2
    ext = np.zeros((H + 2 * rd, W + 2 * rd), bool)
    ext[rd:rd + H, rd:rd + W] = mask
    out = np.zeros((H, W), bool)
    for dy in range(2 * rd + 1):
        for dx in range(2 * rd + 1):
            out |= ext[dy:dy + H, dx:dx + W]
    return out


def recover_plane(v, threshold, d, w):
    v = np.asarray(v, np.int64)
    return np.where(dilate(v > threshold, d), blur_plane(v, w), v)


def recover(img, threshold=200, dilate=5, ksize=15, sigma=0.0, order=0):
    """lio_exposure_recover"""
    a = np.asarray(img)
    w = gaussian_weights(ksize, sigma)
    if a.ndim == 2:
        return recover_plane(a, threshold, dilate, w).astype(np.uint8)
    h, s, v = ER.bgr2hsv(*ER.split(a, order))
    return ER.merge(*ER.hsv2bgr(h, s, recover_plane(v, threshold, dilate, w)), order)


def gaussian_blur(img, ksize, sigma=0.0):
    """lio_exposure_gaussian_blur"""
    a = np.asarray(img)
    w = gaussian_weights(ksize, sigma)
    if a.ndim == 2:
        return blur_plane(a, w).astype(np.uint8)
    return np.stack([blur_plane(a[..., c], w) for c in range(a.shape[2])], -1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ images
def _shape(width, height, channels):
    return (height, width) if channels == 1 else (height, width, channels)


def stripes(width, height, channels):
    """values 199..202 in vertical stripes of one column (V of a 3-channel pixel is its largest byte)"""
    v = (199 + np.arange(width) % 4).astype(np.uint8)[None, :] + np.zeros((height, 1), np.uint8)
    if channels == 1:
        return v
    return np.stack([v, v // 2, np.full_like(v, 30)], -1)


def bright_points(width, height, channels):
    """a dark ground (40) with one pixel of 255 in each corner and in the centre"""
    img = np.full(_shape(width, height, channels), 40, np.uint8)
    for y, x in ((0, 0), (0, width - 1), (height - 1, 0), (height - 1, width - 1), (height // 2, width // 2)):
        img[y, x] = 255
    return img


def step(width, height, channels, at, vertical):
    """201 before column (vertical: row) `at`, 50 from it on"""
    img = np.full(_shape(width, height, channels), 50, np.uint8)
    if vertical:
        img[:at] = 201
    else:
        img[:, :at] = 201
    return img


def images(width, height, channels):
    """exposure_ref's images and the ones above that fit the shape"""
    out = dict(ER.images(width, height, channels))
    out["stripes"] = stripes(width, height, channels)
    out["points"] = bright_points(width, height, channels)
    return out
