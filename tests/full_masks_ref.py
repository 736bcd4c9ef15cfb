"""Numpy restatement of the path from RoI masks to MOTS run-length strings (test infrastructure only): torchvision's
``paste_masks_in_image(padding=1)`` with the float32 operation order of ``csrc/full_masks.hip``, ``ensure_unique_masks``, the
threshold, and COCO's run-length code after ``maskApi.c``.  It is the project's definition of the result:
tests/test_full_masks_cpu.py pins it to the literal pipeline (``literal_*``: the resize done by ``torch.nn.functional.interpolate``
on the CPU) and to the reference's own ``ensure_unique_masks`` (tests/golden/g20_full_masks.npz, tools/make_golden.py gen_g20);
tests/test_gpu_full_masks.py compares the device results with it bit for bit."""
import numpy as np

F32 = np.float32
COORD_MAX = 2.0 ** 29   # csrc/full_masks.hip clamps the expanded coordinates here


def np_expand_boxes(boxes, mw):
    """``expand_boxes`` + ``.to(torch.int64)`` of roi_heads.py: int64 [n, 6] = x0, y0, x1, y1 (inclusive corners) and the size
    (w, h) of the resize.  float64, one operation at a time; a box that is not finite is the empty box (0, 0, -1, -1, 1, 1)."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    scale = float(mw + 2) / mw
    with np.errstate(invalid="ignore", over="ignore"):
        w_half = (b[:, 2] - b[:, 0]) * 0.5
        h_half = (b[:, 3] - b[:, 1]) * 0.5
        xc = (b[:, 2] + b[:, 0]) * 0.5
        yc = (b[:, 3] + b[:, 1]) * 0.5
        w_half = w_half * scale
        h_half = h_half * scale
        e = np.stack((xc - w_half, yc - h_half, xc + w_half, yc + h_half), axis=1)
    ok = np.isfinite(e).all(axis=1)
    c = np.trunc(np.clip(np.where(ok[:, None], e, 0.0), -COORD_MAX, COORD_MAX)).astype(np.int64)
    out = np.empty((b.shape[0], 6), np.int64)
    out[:, :4] = c
    out[:, 4] = np.maximum(c[:, 2] - c[:, 0] + 1, 1)
    out[:, 5] = np.maximum(c[:, 3] - c[:, 1] + 1, 1)
    out[~ok] = (0, 0, -1, -1, 1, 1)
    return out


def _axis(out_size, in_size):
    """Source indices and weights of one axis of ``F.interpolate(mode='bilinear', align_corners=False)``, in float32."""
    scale = F32(in_size) / F32(out_size)
    j = np.arange(out_size, dtype=np.int64).astype(F32)
    src = np.maximum(scale * (j + F32(0.5)) - F32(0.5), F32(0))
    i0 = src.astype(np.int64)
    i1 = np.minimum(i0 + 1, in_size - 1)
    l1 = src - i0.astype(F32)
    l0 = F32(1) - l1
    return i0, i1, l0, l1


def np_resize(mask, h, w, rows=None, cols=None):
    """The zero-padded ``mask`` [mh, mw] resized to (h, w), or its rows / columns ``rows`` / ``cols`` only: float32,
    ``l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)`` with every product and sum rounded."""
    m = np.pad(np.asarray(mask, F32), 1)
    y0, y1, ly0, ly1 = _axis(h, m.shape[0])
    x0, x1, lx0, lx1 = _axis(w, m.shape[1])
    if rows is not None:
        y0, y1, ly0, ly1 = y0[rows], y1[rows], ly0[rows], ly1[rows]
    if cols is not None:
        x0, x1, lx0, lx1 = x0[cols], x1[cols], lx0[cols], lx1[cols]
    with np.errstate(invalid="ignore", over="ignore"):
        top = lx0[None, :] * m[y0][:, x0] + lx1[None, :] * m[y0][:, x1]
        bot = lx0[None, :] * m[y1][:, x0] + lx1[None, :] * m[y1][:, x1]
        out = ly0[:, None] * top + ly1[:, None] * bot
    assert out.dtype == F32
    return out


def _paste(masks, boxes, H, W, resize):
    """[n, H, W] float32: every mask in an image of its own; ``resize(mask, h, w, rows, cols)`` gives the needed part."""
    masks = np.asarray(masks, F32)
    masks = masks.reshape(masks.shape[0], masks.shape[-2], masks.shape[-1])
    bx = np_expand_boxes(boxes, masks.shape[2])
    out = np.zeros((masks.shape[0], H, W), F32)
    for i, (x0, y0, x1, y1, w, h) in enumerate(bx.tolist()):
        xa, xb, ya, yb = max(x0, 0), min(x1 + 1, W), max(y0, 0), min(y1 + 1, H)
        if xa >= xb or ya >= yb:
            continue   # an empty slice pastes nothing
        out[i, ya:yb, xa:xb] = resize(masks[i], h, w, slice(ya - y0, yb - y0), slice(xa - x0, xb - x0))
    return out


def np_paste(masks, boxes, H, W):
    return _paste(masks, boxes, H, W, np_resize)


def literal_resize(mask, h, w, rows=None, cols=None):
    import torch
    m = torch.nn.functional.pad(torch.from_numpy(np.asarray(mask, F32)), (1, 1, 1, 1))
    r = torch.nn.functional.interpolate(m[None, None], size=(int(h), int(w)), mode='bilinear', align_corners=False)[0, 0].numpy()
    return r[rows if rows is not None else slice(None)][:, cols if cols is not None else slice(None)]


def literal_paste(masks, boxes, H, W):
    """``paste_masks_in_image`` with torch's own CPU resize."""
    return _paste(masks, boxes, H, W, literal_resize)


def np_unique(images):
    """``ensure_unique_masks`` (utils/mots.py:5-25) as ``(winner [H, W], value [H, W])``: np.argmax takes the first maximum and
    counts a NaN as the maximum (the first NaN).  No image at all: winner -1, value 0."""
    images = np.asarray(images, F32)
    if images.shape[0] == 0:
        return np.full(images.shape[1:], -1, np.int64), np.zeros(images.shape[1:], F32)
    i = np.argmax(images, axis=0)
    return i, np.take_along_axis(images, i[None], axis=0)[0]


def np_labels(winner, value, threshold):
    """int32 [H, W]: the winner where its value reaches the threshold (NaN compares false), else -1."""
    with np.errstate(invalid="ignore"):
        return np.where(value >= F32(threshold), winner, -1).astype(np.int32)


def np_frame(masks, boxes, H, W, threshold, paste=np_paste):
    """One frame: ``(labels [H, W] int32, values [H, W] float32)`` for its masks in order."""
    winner, value = np_unique(paste(masks, boxes, H, W))
    return np_labels(winner, value, threshold), value


def binary_masks(labels, n):
    """[n, H, W] uint8, what the reference encodes: mask i = (labels == i)."""
    return (labels[None] == np.arange(n).reshape(-1, 1, 1)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ COCO run-length code
def np_events(labels, n):
    """``(positions, counts)``: for every mask i < n the ascending column-major positions where ``labels == i`` flips (the
    value before position 0 is "unset"), concatenated over i, and their number per mask."""
    flat = np.asarray(labels).T.reshape(-1)
    pos, counts = [], []
    for i in range(n):
        m = np.concatenate(([False], flat == i))
        p = np.flatnonzero(m[1:] != m[:-1])
        pos.append(p)
        counts.append(p.size)
    return (np.concatenate(pos) if pos else np.zeros(0, np.int64)).astype(np.int64), np.array(counts, np.int64)


def np_rle_counts(mask):
    """``rleEncode`` of maskApi.c on one (H, W) mask, read column by column."""
    flat = np.asarray(mask).T.reshape(-1)
    counts, run, prev = [], 0, 0
    for v in flat.tolist():
        if v != prev:
            counts.append(run)
            run, prev = 0, v
        run += 1
    counts.append(run)
    return counts


def np_rle_string(counts):
    """``rleToString`` of maskApi.c, statement by statement."""
    s = []
    for i, x in enumerate(int(c) for c in counts):
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            s.append(chr(c + 48))
    return "".join(s)


def np_rle_from_string(string):
    """``rleFrString`` of maskApi.c, statement by statement."""
    counts, p = [], 0
    while p < len(string):
        x, k, more = 0, 0, True
        while more:
            c = ord(string[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def np_strings(labels, n):
    """The COCO strings of the n masks of one label image."""
    return [np_rle_string(np_rle_counts(labels == i)) for i in range(n)]


# ------------------------------------------------------------------------------------------------ inputs
def blob_masks(rng, n, mh=56, mw=56, noise=0.05):
    """n sigmoid blobs (an ellipse of random centre and radii per mask) plus uniform noise of +-``noise``, float32 in about (0, 1)."""
    yy, xx = np.mgrid[0:mh, 0:mw]
    out = np.empty((n, mh, mw), F32)
    for i in range(n):
        cy, cx = rng.uniform(0.3, 0.7) * mh, rng.uniform(0.3, 0.7) * mw
        ry, rx = rng.uniform(0.2, 0.5) * mh, rng.uniform(0.2, 0.5) * mw
        d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        out[i] = 1.0 / (1.0 + np.exp(6.0 * (d - 1.0))) + rng.uniform(-noise, noise, (mh, mw))
    return out


def random_boxes(rng, n, H, W, lo=3.0, hi=90.0):
    """n boxes (left, top, right, bottom) float64 with sides in [lo, hi], centred anywhere from 10 % outside the image on."""
    w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    cx, cy = rng.uniform(-0.1 * W, 1.1 * W, n), rng.uniform(-0.1 * H, 1.1 * H, n)
    return np.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), axis=1)
