"""CPU checks of the exposure contract's numpy restatement (tests/exposure_ref.py) against itself and of the host
table helpers of lio_gpu.exposure against numpy: the properties the contract states, on the sizes where they can
break."""
import numpy as np
import pytest

import exposure_ref as ER
from lio_gpu import exposure as EX

ROUND_TRIP_MAX = 5  # the largest channel error of BGR -> HSV -> BGR over all 2^24 colours, as this test found it


def test_hsv_over_all_colours():
    """h in 0..179, s in 0..255, v the maximum; greys come back as themselves; swapping the order is swapping the
    bytes; the largest error of the round trip"""
    worst, count_worst = 0, 0
    for r0 in range(0, 256, 16):
        b, g, r = np.meshgrid(np.arange(256), np.arange(256), np.arange(r0, r0 + 16), indexing="ij")
        h, s, v = ER.bgr2hsv(b, g, r)
        assert h.min() >= 0 and h.max() <= 179 and s.min() >= 0 and s.max() <= 255
        assert (v == np.maximum(b, np.maximum(g, r))).all()
        b2, g2, r2 = ER.hsv2bgr(h, s, v)
        grey = (b == g) & (g == r)
        assert (s[grey] == 0).all() and (b2[grey] == b[grey]).all() and (g2[grey] == g[grey]).all() and (r2[grey] == r[grey]).all()
        err = np.maximum(abs(b2 - b), np.maximum(abs(g2 - g), abs(r2 - r)))
        if err.max() > worst:
            worst, count_worst = int(err.max()), 0
        count_worst += int((err == worst).sum())
        # order 1 on the swapped bytes is order 0
        img = ER.merge(b, g, r, 0)
        for x, y in zip(ER.split(img[..., ::-1], 1), (b, g, r)):
            assert (x == y).all()
        ident = np.arange(256, dtype=np.uint8)
        if r0 == 96:
            np.testing.assert_array_equal(ER.remap(img[:, :, 3, ::-1], ident, None, 1), ER.remap(img[:, :, 3], ident, None, 0)[..., ::-1])
    print("largest round-trip channel error", worst, "in", count_worst, "colours")
    assert worst == ROUND_TRIP_MAX


def test_division_tables():
    assert ER.SDIV[0] == 0 and ER.HDIV[0] == 0 and ER.SDIV[255] == 4096 and ER.SDIV[1] == 255 << 12 and ER.HDIV[1] == 122880
    for i in range(1, 256):  # the integer rounding (ties to even) of the exact quotient
        for tab, num, den in ((ER.SDIV, 255 << 12, i), (ER.HDIV, 180 << 12, 6 * i)):
            q, r = divmod(num, den)
            q += 1 if (2 * r > den or (2 * r == den and q % 2)) else 0
            assert tab[i] == q


def test_float_constants():
    assert ER.HS == np.float32(1.0 / 30.0) and ER.K == np.float32(1.0 / 255.0)
    assert float(ER.HS).hex() == "0x1.1111120000000p-5" and float(ER.K).hex() == "0x1.0101020000000p-8"


def test_closed_form_residual_equals_the_loop():
    rng = np.random.default_rng(5)
    for res in range(256):
        for batch in (0, 3):
            clip = 40
            hist = rng.integers(0, clip + 1, 256).astype(np.int64)
            hist[7] = clip + res + 256 * batch  # the excess is exactly res + 256 batch
            a, b = ER.redistribute_closed(hist, clip), ER.redistribute_loop(hist, clip)
            np.testing.assert_array_equal(a, b, err_msg=f"res {res} batch {batch}")
            assert a.sum() == hist.sum()


def test_padding_quirk():
    t = ER.Tiling(64, 38, 2.0, 8, 8)
    assert (t.ext_w, t.ext_h, t.tw, t.th) == (72, 40, 9, 5)  # 64 divides evenly and is padded by a whole tiles_x
    t = ER.Tiling(64, 48, 2.0, 8, 8)
    assert (t.ext_w, t.ext_h, t.pad_w, t.pad_h) == (64, 48, 0, 0)
    t = ER.Tiling(67, 38, 2.0, 8, 8)
    assert (t.ext_w, t.ext_h) == (72, 40)
    t = ER.Tiling(9, 7, 2.0, 8, 6)
    assert (t.ext_w, t.ext_h, t.tw, t.th) == (16, 12, 2, 2)
    assert ER.Tiling(5, 7, 2.0, 4, 1).pad_w == 3 and ER.Tiling(3, 7, 2.0, 2, 1).pad_w == 1  # pads of at most width - 1
    with pytest.raises(ValueError):
        ER.Tiling(2, 7, 2.0, 4, 1)  # a pad of 2 columns on a width of 2
    with pytest.raises(ValueError):
        ER.Tiling(8, 3, 2.0, 8, 8)  # 8 % 8 == 0 but the rows do not divide: the width is padded by 8 > 7
    # the reflected border is REFLECT_101
    plane = np.arange(9 * 7).reshape(7, 9) % 256
    t = ER.Tiling(9, 7, 0.0, 8, 6)
    ext = np.pad(plane, ((0, t.pad_h), (0, t.pad_w)), mode="reflect")
    for x in range(9, 16):
        np.testing.assert_array_equal(ext[:7, x], plane[:, 2 * 8 - x])
    for y in range(7, 12):
        np.testing.assert_array_equal(ext[y, :9], plane[2 * 6 - y])


def test_clip_values():
    assert ER.Tiling(64, 48, 0.0, 8, 8).clip == 0 and ER.Tiling(64, 48, -3.0, 8, 8).clip == 0
    assert ER.Tiling(64, 48, 0.001, 8, 8).clip == 1  # a tiny positive limit
    assert ER.Tiling(64, 48, 2.0, 8, 8).clip == 1 and ER.Tiling(64, 48, 40.0, 8, 8).clip == 7
    assert ER.Tiling(4096, 2464, 2.0, 8, 8).clip == 2 * 512 * 308 // 256
    with pytest.raises(ValueError):
        ER.Tiling(64, 48, float("nan"), 8, 8)
    with pytest.raises(ValueError):
        ER.Tiling(64, 48, 1e12, 8, 8)
    # clip_limit <= 0 is plain AHE: the tables are the scaled cumulative histograms
    plane = ER.random_image(64, 48, 1, seed=2).astype(np.int64)
    t = ER.Tiling(64, 48, 0.0, 8, 8)
    L = ER.clahe_luts(plane, t)
    tile = plane[6:12, 8:16]
    want = ER.sat_rint(np.cumsum(np.bincount(tile.ravel(), minlength=256)).astype(np.float32) * (np.float32(255) / np.float32(48)))
    np.testing.assert_array_equal(L[1, 1], want)


@pytest.mark.parametrize("value", [0, 1, 128, 255])
@pytest.mark.parametrize("clip", [0.0, 2.0, 1e6])
def test_constant_plane_maps_to_one_value(value, clip):
    for (w, h, tx, ty) in ((64, 48, 8, 8), (67, 38, 8, 8), (5, 7, 1, 1)):
        out = ER.clahe(np.full((h, w), value, np.uint8), clip, (tx, ty))
        assert len(np.unique(out)) == 1, (w, h, out.min(), out.max())


def test_script_normalisation_is_the_identity():
    v = np.arange(256, dtype=np.uint8)
    back = (np.clip(v.astype(np.float32) / 255.0, 0, 1) * 255).astype(np.uint8)
    np.testing.assert_array_equal(back, v)


# ------------------------------------------------------------------------------------------- the host helpers
def test_stretch_percentiles_equal_numpy():
    rng = np.random.default_rng(9)
    planes = [rng.integers(0, 256, (37, 53), dtype=np.uint8), rng.integers(0, 256, (48, 64), dtype=np.uint8),
              rng.integers(100, 104, (31, 17), dtype=np.uint8), rng.choice(np.array([3, 200], np.uint8), (20, 21)),
              rng.choice(np.array([0, 17, 255], np.uint8), (19, 7)), np.array([[5, 9]], np.uint8), np.array([[77]], np.uint8),
              (rng.integers(0, 40, (101, 1)) ** 1.5).astype(np.uint8)]
    for k, p in enumerate(planes):
        hist = np.bincount(p.ravel(), minlength=256)
        for q in (5, 95, 0, 100, 50, 33.3):
            assert EX.hist_percentile(hist, q) == float(np.percentile(p, q)), (k, q)
        lo, hi = np.percentile(p, 5), np.percentile(p, 95)
        if hi == lo:
            with pytest.raises(ValueError):
                EX.stretch_lut(hist)
            continue
        with np.errstate(all="ignore"):
            want = np.clip((p - lo) / (hi - lo) * 255, 0, 255).astype(np.uint8)  # the script's line
        np.testing.assert_array_equal(EX.stretch_lut(hist, 5, 95)[p], want, err_msg=str(k))


def test_equalize_lut():
    one = np.zeros(256, np.int64)
    one[93] = 1234
    np.testing.assert_array_equal(EX.equalize_lut(one), np.full(256, 93, np.uint8))  # a one-value histogram
    two = one.copy()
    two[200] = 10
    lut = EX.equalize_lut(two)
    assert (lut[:200] == 0).all() and (lut[200:] == 255).all()
    rng = np.random.default_rng(3)
    hist = rng.integers(0, 5000, 256)
    hist[:9] = 0
    lut = EX.equalize_lut(hist)
    scale = np.float32(255.0) / np.float32(hist.sum() - hist[9])
    acc = 0
    for i in range(256):
        if i <= 9:
            assert lut[i] == 0
        else:
            acc += int(hist[i])
            assert lut[i] == min(max(int(np.rint(np.float32(acc) * scale)), 0), 255)
    assert lut[255] == 255 and (np.diff(lut.astype(int)) >= 0).all()
    with pytest.raises(ValueError):
        EX.equalize_lut(np.zeros(256))


def test_gamma_lut_and_detect():
    x = np.arange(256)
    for g in (0.8, 1.2, 1.0):
        np.testing.assert_array_equal(EX.gamma_lut(g), np.clip(((x / 255.0) ** g) * 255.0, 0, 255).astype(np.uint8))
    assert EX.gamma_lut(0.8)[0] == 0 and EX.gamma_lut(0.8)[255] == 255 and EX.gamma_lut(1.0)[128] in (127, 128)
    h = np.zeros(256, np.int64)
    h[100] = 70
    h[200] = 30
    assert EX.detect_exposure(h) == "well-exposed"  # 0.3 is not more than 0.3
    h[255] = 1
    assert EX.detect_exposure(h) == "overexposed"
    h[:] = 0
    h[49], h[50] = 31, 69
    assert EX.detect_exposure(h) == "underexposed"
    h[49], h[50] = 30, 70
    assert EX.detect_exposure(h) == "well-exposed"
    h[199], h[10] = 100, 100  # both dark and bright: the bright test comes first, and 199 is not bright
    assert EX.detect_exposure(h) == "underexposed"


def test_images_cover_their_cases():
    im = ER.images(64, 48, 3)
    assert set(im) == {"random", "ramp", "zeros", "full", "sky", "few"}
    assert (im["sky"][:24] == 255).all() and len(np.unique(im["few"].reshape(-1, 3), axis=0)) <= 4
    vd = ER.vd_image()
    h, s, v = ER.bgr2hsv(*ER.split(vd))
    d = v - np.minimum(vd[..., 0], np.minimum(vd[..., 1], vd[..., 2])).astype(np.int64)
    pairs = set(zip(v.ravel().tolist(), d.ravel().tolist()))
    assert len(pairs) == 256 * 257 // 2  # every v with every d <= v
