"""The numpy restatement of the embedding inputs (tests/embed_inputs_ref.py) pinned without a device: its patches against what
numpy's ``pad`` and Pillow's ``resize`` returned (tests/golden/g23_reid_crops.npz, byte for byte), its RoIAlign by properties with
derived float32 bounds, the level mapper at its boundaries -- and every ``ValueError`` of ``mpntrackseg_amd.embed_inputs``, which
its host code raises before a device is needed."""
import numpy as np
import pytest
import torch

import embed_inputs_ref as R
from mpntrackseg_amd import embed_inputs as E

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
GROUPS = (("small_128x64", "small_frames", (128, 64)), ("small_16x8", "small_frames", (16, 8)), ("small_5x3", "small_frames", (5, 3)),
          ("big_128x64", "big_frames", (128, 64)))


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("g23_reid_crops.npz")


# ------------------------------------------------------------------------------------------------ patches
@pytest.mark.parametrize("group,frames,size", GROUPS)
def test_restated_crops_equal_pad_and_pillow_byte_for_byte(fixture, group, frames, size):
    u8, _ = R.reid_crops(fixture[frames], fixture[group + "_boxes"], fixture[group + "_frame"], size)
    assert u8.dtype == np.uint8 and u8.shape == fixture[group + "_crops"].shape
    assert np.array_equal(u8, fixture[group + "_crops"])


def test_the_fixture_holds_the_cases_it_is_for(fixture):
    H, W = fixture["small_frames"].shape[1:3]
    geo = {str(n): R.crop_geometry(b, H, W) for n, b in zip(fixture["small_names"], fixture["small_16x8_boxes"])}
    sides = {n: (g[4] + g[1] - g[0] + g[5], g[6] + g[3] - g[2] + g[7]) for n, g in geo.items()}
    assert sides["inside 9 x 5, upscaled"] == (9, 5) and sides["1 x 1"] == (1, 1) and sides["whole frame"] == (37, 53)
    # the whole frame to (5, 3): both downscales are over 7, and the taps grow with them -- 15 down the rows, 35 along them
    assert 37 / 5 > 7 and len(R.resample_coeffs(37, 5)[2][1]) == 15 and max(len(c) for _, c in R.resample_coeffs(53, 3)) == 35
    assert sides["width 8 = ow"][1] == 8 and sides["height 16 = oh"][0] == 16 and sides["width 3 = ow"][1] == 3 and sides["height 5 = oh"][0] == 5
    assert sides["padded width 64 = ow"][1] == 64 and sides["padded height 128 = oh"][0] == 128
    only = lambda g, i: g[4 + i] > 0 and sum(g[4:]) == g[4 + i]
    assert only(geo["over the top edge"], 0) and only(geo["over the bottom edge"], 1) and only(geo["over the left edge"], 2) and only(geo["over the right edge"], 3)
    assert all(v > 0 for v in geo["over all four edges"][4:])
    g = geo["pad larger than the crop"]
    assert g[6] > g[3] - g[2]
    assert sum(geo["top = -0.5: no pad"][4:]) == 0 and sum(geo["bottom = H + 0.6: no pad"][4:]) == 0
    assert np.array_equal(np.unique(fixture["small_16x8_frame"]), [0, 1])


def test_restated_pad_is_numpy_pad(fixture):
    crop = fixture["small_frames"][0, 3:12, 20:27]
    for pads in ((2, 0, 0, 0), (0, 3, 0, 0), (0, 0, 4, 0), (0, 0, 0, 5), (3, 1, 2, 6), (20, 0, 0, 31)):
        want = np.pad(crop, ((pads[0], pads[1]), (pads[2], pads[3]), (0, 0)), mode="mean")
        assert np.array_equal(R.pad_mean(crop, *pads), want), pads


def test_normalised_output_is_the_float32_formula(fixture):
    u8, got = R.reid_crops(fixture["small_frames"], fixture["small_16x8_boxes"], fixture["small_16x8_frame"], (16, 8))
    assert got.dtype == F32 and got.shape == (u8.shape[0], 3, 16, 8)
    for c in range(3):
        table = np.asarray([(F32(v) / F32(255) - F32(R.MEAN[c])) / F32(R.STD[c]) for v in range(256)])
        assert table.dtype == F32
        assert np.array_equal(got[:, c], table[u8[..., c]])


# ------------------------------------------------------------------------------------------------ RoIAlign
def test_roi_align_of_a_constant_map_is_the_constant():
    """A sample's four weights are (hy + ly)(hx + lx) with h = float32(1 - l): 2 roundings; in float32 four products of weights,
    four by the constant and three sums follow: 13 roundings per sample; then four sums of samples and a division: 18 in all.
    The bound is 20 x 2^-24 |c| for float32 and 4 x 2^-24 |c| for float64 (the roundings of h alone, twice over)."""
    for acc, factor in ((F32, 20), (F64, 4)):
        for c, box, scale in ((3.7, (10.3, 20.9, 90.2, 77.7), 0.25), (-0.013, (0, 0, 159.9, 127.9), 0.125), (251.0, (33.3, 8.1, 35.0, 60.0), 0.5)):
            out = R.roi_align(np.full((2, 64, 80), c, F32), box, scale, 14, 2, acc)
            assert out.dtype == acc and np.abs(out.astype(F64) - F64(F32(c))).max() <= factor * EPS * abs(c), (acc, c)


def test_roi_align_of_a_ramp_is_the_ramp_at_the_bin_centres():
    """On a y + b x bilinear interpolation is exact and the samples of a bin lie symmetrically about its centre, so the result is
    the ramp at start + (p + .5) bin.  Roundings, each at most 2^-24 of M = |a| h + |b| w: roi_start, extent, bin and the four
    operations of a sample position (7, scaled by the slope: at most M), the map's own float32 values (1), h (1), a sample's four
    weight products, four value products and three sums (11), four sums of samples of up to 4 M before the division by 4 (4) and
    the division (1): 25.  The bound is 32 x 2^-24 M."""
    h, w = 64, 80
    y, x = np.mgrid[0:h, 0:w].astype(F64)
    for a, b, box, scale, S in ((0.7, -1.3, (40.3, 30.9, 250.2, 200.7), 0.25, 14), (2.5, 0.4, (16.0, 8.0, 400.0, 330.0), 0.125, 7),
                                (-0.3, 0.9, (5.5, 7.25, 100.0, 90.0), 0.5, 3)):
        feat = (a * y + b * x).astype(F32)[None]
        out = R.roi_align(feat, box, scale, S, 2, F32)[0].astype(F64)
        sx, sy = box[0] * scale, box[1] * scale
        bx, by = max(box[2] * scale - sx, 1.0) / S, max(box[3] * scale - sy, 1.0) / S
        assert sx >= 0 and sy >= 0 and sx + S * bx <= w - 1 and sy + S * by <= h - 1      # inside the map: nothing clamps
        p = np.arange(S) + 0.5
        want = a * (sy + p * by)[:, None] + b * (sx + p * bx)[None, :]
        M = abs(a) * h + abs(b) * w
        assert np.abs(out - want).max() <= 32 * EPS * M, (a, b)


def test_float32_roi_align_stays_within_16_roundings_of_float64():
    rng = np.random.default_rng(5)
    feat = rng.normal(size=(6, 32, 40)).astype(F32)
    for box, scale, S in (((10.3, 20.9, 290.2, 177.7), 0.125, 14), ((-30.0, -20.0, 100.0, 90.0), 0.125, 7), ((250.0, 200.0, 400.0, 300.0), 0.125, 3),
                          ((33.0, 44.0, 35.0, 250.0), 0.125, 14)):
        lo, hi = R.roi_align(feat, box, scale, S, 2, F32), R.roi_align(feat, box, scale, S, 2, F64)
        terms = R.roi_align(np.abs(feat), box, scale, S, 2, F64)       # the sum of |weight x value| over the count
        assert lo.dtype == F32 and hi.dtype == F64
        assert (np.abs(lo.astype(F64) - hi) <= 16 * EPS * terms).all(), box


def test_level_mapper_at_the_canonical_sizes():
    square = lambda s, x=20.0, y=30.0: (x, y, x + s, y + s)
    boxes = np.asarray([square(112), square(224), square(448), square(10), square(2000), (5, 5, 5, 90), (5, 5, 90, 5)], F32)
    want = [1, 2, 3, 0, 3, 0, 0]
    assert R.box_levels(boxes).tolist() == want
    assert E.box_levels(boxes).tolist() == want
    assert E.level_scales([(128, 160), (64, 80), (32, 40), (16, 20)], (500, 640)) == [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    assert R.level_scales([(200, 336), (100, 168), (50, 84), (25, 42)], (800, 1333)) == [1 / 4, 1 / 8, 1 / 16, 1 / 32]


def test_host_mapping_equals_the_restatement():
    rng = np.random.default_rng(0)
    boxes = rng.uniform(0, 300, (300, 4))
    boxes[:, 2:] = boxes[:, :2] + rng.uniform(2, 500, (300, 2))
    shapes = [(128, 160), (64, 80), (32, 40), (16, 20)]
    b, scales, levels = E.map_boxes(boxes, shapes, (500, 640), (375, 480))
    want = R.resize_boxes(boxes, (375, 480), (500, 640))
    assert b.dtype == torch.float32 and np.array_equal(b.numpy(), want) and scales == R.level_scales(shapes, (500, 640))
    near = np.abs(np.log2(np.sqrt((want[:, 2] - want[:, 0]).astype(F64) * (want[:, 3] - want[:, 1])) / 224) % 1 - 0.5) > 0.499
    assert np.array_equal(levels.numpy()[~near], R.box_levels(want)[~near]) and set(levels.tolist()) == {0, 1, 2, 3}
    for k, g in enumerate(E.crop_geometry(boxes, 375, 480)):
        assert tuple(g) == R.crop_geometry(boxes[k], 375, 480)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_value_error_is_raised_on_the_host():
    frames = torch.zeros((2, 37, 53, 3), dtype=torch.uint8)      # (not on a device: the boxes are looked at first)
    ok = np.asarray([[5.0, 5.0, 20.0, 30.0]])
    for boxes, text in (([[60.0, 0, 70, 5]], "empty crop"), ([[5.0, 40, 20, 50]], "empty crop"), ([[5.0, 5, 5.5, 30]], "empty crop"),
                        ([[0.0, -3, 10, -1]], "empty crop"), ([[0.0, 0, np.nan, 4]], "not finite"), ([[0.0, -np.inf, 10, 4]], "not finite"),
                        ([[0.0, 0, 1e9, 5]], "MPNHIP_CROP_MAX_SIDE"), ([[-8200.0, 0, 5, 5]], "MPNHIP_CROP_MAX_SIDE")):
        with pytest.raises(ValueError, match=text):
            E.reid_crops(frames, np.asarray(boxes), [0])
    assert E.crop_geometry(np.asarray([[-8100.0, 0, 5, 5]]), 37, 53, pad=False)[0, 4:].tolist() == [0, 0, 0, 0]
    for box_frame in ([2], [-1], [0.0], [0, 1]):
        with pytest.raises(ValueError, match="box_frame|one frame index per box"):
            E.reid_crops(frames, ok, box_frame)
    feats = [torch.zeros((2, 5, h, w)) for h, w in ((128, 160), (64, 80), (32, 40), (16, 20))]
    for boxes, text in (([[0.0, 0, np.inf, 4]], "not finite"), ([[10.0, 0, 9, 4]], "x2 < x1"), ([[0.0, 8, 9, 4]], "y2 < y1")):
        with pytest.raises(ValueError, match=text):
            E.fpn_roi_align(feats, np.asarray(boxes), [0], (500, 640))
    with pytest.raises(ValueError, match="box_frame"):
        E.fpn_roi_align(feats, ok, [2], (500, 640))
    with pytest.raises(ValueError, match="2\\^24"):
        E.fpn_roi_align(feats, ok, [0], (500, 640), detection_id=[1 << 24])
    with pytest.raises(ValueError, match="no one scale"):
        E.fpn_roi_align([feats[0], feats[1], feats[2], torch.zeros((2, 5, 16, 40))], ok, [0], (500, 640))
    with pytest.raises(ValueError, match="at most 1024"):
        E.fpn_roi_align(feats, ok, [0], (500, 640), output_size=600)
    # and with nothing wrong, the missing device is what is reported: there is no CPU fallback
    with pytest.raises(E.MpnhipError, match="no CPU fallback"):
        E.reid_crops(frames, ok, [0])
    with pytest.raises(E.MpnhipError, match="no CPU fallback"):
        E.fpn_roi_align(feats, ok, [0], (500, 640))


def test_entry_points_check_their_arguments_without_a_device():
    import ctypes
    from mpntrackseg_amd import capi
    l = capi.load()
    p = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    ms = (ctypes.c_float * 6)(*(R.MEAN + R.STD))
    need = l.mpnhip_reid_crops_workspace_bytes(50, 300, 120, 128, 64)
    assert need > 0 and l.mpnhip_reid_crops_workspace_bytes(100, 300, 120, 128, 64) > need
    assert l.mpnhip_reid_crops_workspace_bytes(50, 8193, 120, 128, 64) == 0 and l.mpnhip_reid_crops_workspace_bytes(50, 300, 120, 0, 64) == 0
    crops = lambda n=50, ph=300, pw=120, oh=128, ow=64, ws=p, nbytes=1 << 40, frames=p, norm=ms: \
        l.mpnhip_reid_crops(frames, 2, 1080, 1920, p, p, n, ph, pw, oh, ow, norm, p, None, ws, nbytes, None)
    assert crops(n=0) == 0                                    # no boxes: a successful no-op
    assert crops(ph=8193) == -1 and crops(ow=0) == -1 and crops(n=-1) == -1 and crops(frames=None) == -1 and crops(norm=None) == -1
    assert b"reid_crops" in l.mpnhip_last_error()
    assert crops(norm=(ctypes.c_float * 6)(0, 0, 0, 1, 0, 1)) == -1 and b"std" in l.mpnhip_last_error()
    assert crops(ws=None) == -3 and crops(nbytes=need - 1) == -3 and b"reid_crops: workspace" in l.mpnhip_last_error()
    assert crops(ph=8192, oh=8, ow=8192) == -4 and b"LDS" in l.mpnhip_last_error()     # MPNHIP_ERR_UNSUPPORTED
    lv = capi.FpnLevels()
    for i, (h, w) in enumerate(((200, 336), (100, 168), (50, 84), (25, 42))):
        lv.data[i], lv.h[i], lv.w[i], lv.scale[i] = p.value, h, w, 0.25 / 2 ** i
    roi = lambda n=3, S=14, g=2, levels=lv, boxes=p: l.mpnhip_fpn_roi_align(ctypes.byref(levels) if levels else None, 2, 256, boxes, p, p, n, S, g,
                                                                            None, p, None)
    assert roi(n=0) == 0
    assert roi(levels=None) == -1 and roi(S=0) == -1 and roi(g=0) == -1 and roi(S=600) == -1 and roi(boxes=None) == -1 and roi(n=-1) == -1
    assert b"fpn_roi_align" in l.mpnhip_last_error()
    bad = capi.FpnLevels.from_buffer_copy(lv)
    bad.scale[2] = 0.0
    assert roi(levels=bad) == -1 and b"level 2" in l.mpnhip_last_error()
    bad = capi.FpnLevels.from_buffer_copy(lv)
    bad.data[1] = None
    assert roi(levels=bad) == -1 and b"level 1" in l.mpnhip_last_error() and roi(levels=bad, n=0) == 0
