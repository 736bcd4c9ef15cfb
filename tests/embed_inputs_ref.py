"""numpy restatement of ``mpntrackseg_amd.embed_inputs`` (``csrc/embed_inputs.hip``), without torchvision and without PIL:

ReID patches      ``BoundingBoxDataset.__getitem__`` (``utils/rgb.py:40-69``): the crop, ``np.pad(mode='mean')`` in integer
                  arithmetic, Pillow's ``ImagingResample`` for 8-bit images (bilinear, fixed point with 22 bits), ``ToTensor``
                  and ``Normalize`` in float32;
FPN RoIAlign      ``resize_boxes``, the level mapper and ``roi_align`` of ``MultiScaleRoIAlign`` (torchvision 0.6.0, CPU) in the
                  operator's order, with the interpolation in ``acc`` = float32 (the device's bits) or float64.

``tests/golden/g23_reid_crops.npz`` (``tools/make_golden_embed_inputs.py``) holds what numpy's ``pad`` and Pillow's ``resize``
themselves return; ``test_embed_inputs_cpu.py`` pins this file against it."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
PRECISION_BITS = 22
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------------ ReID patches
def crop_geometry(box, H, W, pad=True):
    """``(y0, y1, x0, x1, pt, pb, pl, pr)`` of one box (left, top, right, bottom) in an ``H x W`` frame: the reference's
    expressions (``rgb.py:51-58``), the slice clipped as numpy clips it."""
    left, top, right, bot = (float(v) for v in box)
    y0, y1 = min(int(max(0, top)), H), min(int(max(0, bot)), H)
    x0, x1 = min(int(max(0, left)), W), min(int(max(0, right)), W)
    if not pad:
        return y0, y1, x0, x1, 0, 0, 0, 0
    return (y0, y1, x0, x1, int(abs(top - max(top, 0))), int(abs(bot - min(bot, H))), int(abs(left - max(left, 0))),
            int(abs(right - min(right, W))))


def mean_u8(total, count):
    """``round(total / count)`` half to even in integer arithmetic: numpy's ``mean`` of uint8 followed by ``round``"""
    total = np.asarray(total, np.int64)
    q, r = total // count, total % count
    return q + ((2 * r > count) | ((2 * r == count) & (q % 2 == 1)))


def pad_mean(crop, pt, pb, pl, pr):
    """``np.pad(crop, ((pt, pb), (pl, pr), (0, 0)), mode='mean')`` for uint8 ``crop`` [h, w, 3]: axis 0 first (the mean of every
    column over the crop's rows), then axis 1 (every row of the result, the new ones included, by its mean over the crop's
    columns)"""
    ch, cw, _ = crop.shape
    rows = crop.astype(np.int64)
    if pt or pb:
        col = mean_u8(rows.sum(axis=0), ch)
        rows = np.concatenate([np.broadcast_to(col, (pt, cw, 3)), rows, np.broadcast_to(col, (pb, cw, 3))], axis=0)
    if pl or pr:
        rm = mean_u8(rows.sum(axis=1), cw)[:, None, :]
        rows = np.concatenate([np.broadcast_to(rm, (rows.shape[0], pl, 3)), rows, np.broadcast_to(rm, (rows.shape[0], pr, 3))], axis=1)
    return rows.astype(np.uint8)


def resample_coeffs(in_size, out_size):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the bilinear filter: per output index ``(xmin, [coef])``"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(xmax - xmin) + xmin - center + 0.5) * ss))
        ww = 0.0
        for v in w:
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        out.append((xmin, np.asarray([int(v * (1 << PRECISION_BITS) + 0.5) for v in w], np.int64)))
    return out


def resample_axis(img, out_size, axis):
    """one pass of ``ImagingResample`` over ``axis`` of uint8 ``img`` [h, w, 3]; skipped when the size does not change"""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    res = np.empty((out_size,) + src.shape[1:], np.int64)
    for xx, (xmin, coef) in enumerate(resample_coeffs(in_size, out_size)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coef, src[xmin:xmin + coef.size], axes=(0, 0))
        assert acc.max() < 2 ** 31
        res[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(res, 0, axis).astype(np.uint8)


def resize_bilinear(img, oh, ow):
    """``Image.fromarray(img).resize((ow, oh), Image.BILINEAR)``: the horizontal pass, then the vertical one"""
    return resample_axis(resample_axis(img, ow, 1), oh, 0)


def normalise(u8, mean=MEAN, std=STD):
    """``ToTensor`` and ``Normalize`` of uint8 [..., h, w, 3] -> float32 [..., 3, h, w], one rounded operation at a time"""
    v = np.moveaxis(np.asarray(u8), -1, -3).astype(F32) / F32(255)
    m, s = np.asarray(mean, F32).reshape(3, 1, 1), np.asarray(std, F32).reshape(3, 1, 1)
    out = (v - m) / s
    assert out.dtype == F32
    return out


def reid_crops(frames, boxes, box_frame, output_size=(128, 64), pad=True, mean=MEAN, std=STD):
    """``(uint8 [n, oh, ow, 3], float32 [n, 3, oh, ow])`` of ``embed_inputs.reid_crops``"""
    frames = np.asarray(frames)
    oh, ow = output_size
    _, H, W, _ = frames.shape
    u8 = np.zeros((len(boxes), oh, ow, 3), np.uint8)
    for k, box in enumerate(boxes):
        y0, y1, x0, x1, pt, pb, pl, pr = crop_geometry(box, H, W, pad)
        u8[k] = resize_bilinear(pad_mean(frames[box_frame[k], y0:y1, x0:x1], pt, pb, pl, pr), oh, ow)
    return u8, normalise(u8, mean, std)


# ------------------------------------------------------------------------------------------------ FPN RoIAlign
def resize_boxes(boxes, original_size, image_size):
    """torchvision's ``resize_boxes`` in float32: boxes [n, 4] (left, top, right, bottom) of the frame -> of the network's image"""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    rh, rw = F32(image_size[0]) / F32(original_size[0]), F32(image_size[1]) / F32(original_size[1])
    out = np.stack([b[:, 0] * rw, b[:, 1] * rh, b[:, 2] * rw, b[:, 3] * rh], axis=1)
    assert out.dtype == F32
    return out


def level_scales(level_shapes, image_size):
    """``MultiScaleRoIAlign.infer_scale`` per level: ``2 ** round(log2(size / image size))``, from heights and from widths"""
    scales = []
    for h, w in level_shapes:
        sh, sw = (2.0 ** round(math.log2(float(s) / float(i))) for s, i in zip((h, w), image_size))
        if sh != sw:
            raise ValueError("a level of %d x %d has no one scale in an image of %d x %d" % (h, w, image_size[0], image_size[1]))
        scales.append(sh)
    return scales


def box_levels(boxes, k_min=2, k_max=5):
    """torchvision 0.6.0's ``LevelMapper`` (canonical scale 224 at level 4, eps = 1e-6 outside the logarithm) in float32"""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    with np.errstate(divide="ignore"):
        s = np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
        k = np.floor((F32(4) + np.log2(s / F32(224))) + F32(1e-6))
    assert k.dtype == F32
    return (np.clip(k, k_min, k_max).astype(np.int64) - k_min)


def roi_axis(v1, v2, scale, S, grid, size, acc):
    """One axis of ``roi_align`` (``aligned=False``) for float tensors: the geometry in float32, one rounded operation at a time;
    the interpolation weights as ``acc``.  Returns ``(low, high, l, h, inside)`` [S, grid]."""
    start = F32(v1) * F32(scale)
    extent = max(F32(F32(v2) * F32(scale) - start), F32(1))
    bin_ = F32(extent / F32(S))
    p, i = np.arange(S, dtype=F32)[:, None], np.arange(grid, dtype=F32)[None, :]
    pos = (start + p * bin_) + ((i + F32(.5)) * bin_) / F32(grid)
    assert pos.dtype == F32
    inside = ~((pos < -1) | (pos > size))
    v = np.where(inside & (pos > 0), pos, F32(0))
    low = v.astype(np.int64)
    edge = low >= size - 1
    low = np.where(edge, size - 1, low)
    high = np.where(edge, size - 1, low + 1)
    v = np.where(edge, low.astype(F32), v)
    l = v - low.astype(F32)
    assert l.dtype == F32
    h = (1.0 - l.astype(F64)).astype(F32)      # (T hy = 1. - ly: a double's subtraction, stored as float)
    return low, high, l.astype(acc), h.astype(acc), inside


def roi_align(feat, box, scale, S=14, grid=2, acc=F32):
    """``roi_align(feat[None], [[0, *box]], S, scale, grid)[0]`` for ``feat`` [C, h, w] and ``box`` (left, top, right, bottom)
    in image coordinates: [C, S, S] in ``acc``.  The four taps of a sample are added in the operator's order, the samples in
    (iy, ix) order, and the sum is divided by their count."""
    feat = np.asarray(feat)
    C, h, w = feat.shape
    t = feat.astype(acc)
    ylo, yhi, ly, hy, yin = roi_axis(box[1], box[3], scale, S, grid, h, acc)
    xlo, xhi, lx, hx, xin = roi_axis(box[0], box[2], scale, S, grid, w, acc)
    out = np.zeros((C, S, S), acc)
    for iy in range(grid):
        for ix in range(grid):
            r0, r1, c0, c1 = ylo[:, iy, None], yhi[:, iy, None], xlo[None, :, ix], xhi[None, :, ix]
            wy0, wy1, wx0, wx1 = hy[:, iy, None], ly[:, iy, None], hx[None, :, ix], lx[None, :, ix]
            s = (((wy0 * wx0) * t[:, r0, c0] + (wy0 * wx1) * t[:, r0, c1]) + (wy1 * wx0) * t[:, r1, c0]) + (wy1 * wx1) * t[:, r1, c1]
            out = out + np.where(yin[:, iy, None] & xin[None, :, ix], s, acc(0))
    out = out / acc(grid * grid)
    assert out.dtype == acc
    return out


def fpn_roi_align(features, boxes, box_frame, image_size, original_size=None, output_size=14, sampling_ratio=2, detection_id=None,
                  acc=F32):
    """``embed_inputs.fpn_roi_align`` over numpy ``features`` (four arrays [B, C, h_l, w_l]): ``(out [n, C (+ 1), S, S], levels)``"""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    if original_size is not None:
        b = resize_boxes(b, original_size, image_size)
    scales = level_scales([f.shape[2:] for f in features], image_size)
    k_min, k_max = int(-math.log2(scales[0])), int(-math.log2(scales[-1]))
    levels = box_levels(b, k_min, k_max)
    C, S = features[0].shape[1], output_size
    extra = 0 if detection_id is None else 1
    out = np.zeros((b.shape[0], C + extra, S, S), acc)
    for k in range(b.shape[0]):
        lv = int(levels[k])
        out[k, extra:] = roi_align(features[lv][box_frame[k]], b[k], scales[lv], S, sampling_ratio, acc)
        if extra:
            out[k, 0] = acc(F32(detection_id[k]))
    return out, levels
