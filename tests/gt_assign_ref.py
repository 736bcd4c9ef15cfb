"""Numpy restatement of ``mpntrackseg_amd/gt_assign.py`` and ``csrc/gt_assign.hip``: the project's definition of what the
reference's ``_assign_gt`` and ``_store_gt_masks`` compute (``lapsolver``, ``pycocotools`` and ``torchvision`` are not installed
where the tests run), pinned by the independent checks of ``tests/test_gt_assign_cpu.py``; and the small scenes the GPU tests
share."""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment as scipy_lsa

from mpntrackseg_amd import masks as M

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ IoU
def box_iou(a, b):
    """[na, nb] float64 of two box lists [n, 4] (top, left, bottom, right): extents with + 1, inter / (A + B - inter)"""
    a, b = np.asarray(a, F64).reshape(-1, 4), np.asarray(b, F64).reshape(-1, 4)
    lo = np.maximum(a[:, None, :2], b[None, :, :2])
    hi = np.minimum(a[:, None, 2:], b[None, :, 2:])
    inter = np.maximum((hi[..., 0] - lo[..., 0]) + 1.0, 0) * np.maximum((hi[..., 1] - lo[..., 1]) + 1.0, 0)
    area = lambda v: ((v[:, 2] - v[:, 0]) + 1.0) * ((v[:, 3] - v[:, 1]) + 1.0)
    return inter / ((area(a)[:, None] + area(b)[None, :]) - inter)


def mask_iou(a_masks, b_masks):
    """[na, nb] float64 of two lists of dense masks: pixels of the intersection over pixels of the union, 0 for an empty union"""
    out = np.zeros((len(a_masks), len(b_masks)), F64)
    union_ok = np.zeros(out.shape, bool)
    for i, a in enumerate(a_masks):
        for j, b in enumerate(b_masks):
            inter = int((a.astype(bool) & b.astype(bool)).sum())
            uni = int(a.astype(bool).sum()) + int(b.astype(bool).sum()) - inter
            union_ok[i, j] = uni > 0
            out[i, j] = float(inter) / float(uni) if uni > 0 else 0.0
    return out, union_ok


# ------------------------------------------------------------------------------------------------ the assignment contract
def ref_assign(iou, min_iou, union_ok=None):
    """``(match [na], allowed [na, nb])``: scipy on ``allowed ? 1 - iou : min(na, nb) + 1``, the pairs on forbidden cells dropped"""
    iou = np.asarray(iou, F64)
    na, nb = iou.shape
    allowed = ~(iou < min_iou) if union_ok is None else (union_ok & ~(iou < min_iou))
    match = np.full(na, -1, np.int64)
    if na and nb:
        rows, cols = scipy_lsa(np.where(allowed, 1.0 - iou, min(na, nb) + 1.0))
        keep = allowed[rows, cols]
        match[rows[keep]] = cols[keep]
    return match, allowed


def all_matchings(allowed):
    """every matching (a tuple of the column of each row, or -1) that uses only allowed pairs"""
    na, nb = allowed.shape

    def rec(i, used):
        if i == na:
            yield ()
            return
        for rest in rec(i + 1, used):
            yield (-1,) + rest
        for j in range(nb):
            if allowed[i, j] and j not in used:
                for rest in rec(i + 1, used | {j}):
                    yield (j,) + rest
    return rec(0, frozenset())


def brute_force(iou, allowed):
    """The contract by exhaustion: ``(match, count, total, gap)`` -- the matching with the most pairs and, among those, the
    smallest total ``1 - iou``; ``gap``: how far the second best total among the matchings of that many pairs lies above it
    (inf when there is none)."""
    na = allowed.shape[0]
    scored = []
    for m in all_matchings(allowed):
        pairs = [(i, j) for i, j in enumerate(m) if j >= 0]
        scored.append((-len(pairs), sum(1.0 - iou[i, j] for i, j in pairs), m))
    scored.sort(key=lambda s: (s[0], s[1]))
    best = scored[0]
    others = [s[1] for s in scored[1:] if s[0] == best[0]]
    return np.asarray(best[2], np.int64).reshape(na), -best[0], best[1], (min(others) - best[1] if others else np.inf)


# ------------------------------------------------------------------------------------------------ RoIAlign
def roi_axis(v1, v2, p, size, acc):
    """One axis of torchvision 0.6.0's CPU ``roi_align`` (``sampling_ratio=-1``, ``aligned=False``) for float tensors.  The
    geometry is float32, one rounded operation at a time -- the reference's boxes and images are ``.float()`` -- and the
    interpolation weights are ``acc``: float64, or float32 in the operator's order.  Returns ``(low, high, l, h, inside)``
    [p, grid] and ``grid``."""
    v1, v2 = F32(v1), F32(v2)
    extent = max(F32(v2 - v1), F32(1))
    bin_ = F32(extent / F32(p))
    grid = int(np.ceil(F32(extent / F32(p))))
    px, i = np.arange(p, dtype=F32)[:, None], np.arange(grid, dtype=F32)[None, :]
    pos = (v1 + px * bin_) + ((i + F32(.5)) * bin_) / F32(grid)
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
    h = 1.0 - l.astype(F64)
    return low, high, l.astype(acc), h.astype(acc), inside, grid


def roi_align(img, box, size=(56, 56), acc=F64):
    """``roi_align(img[None, None], [[0, *box]], size, 1.0)[0, 0]`` for ``img`` [H, W] (0 / 1) and ``box`` (left, top, right,
    bottom): ``(out [size] acc, (grid_h, grid_w))``.  Samples are added in (iy, ix) order; the sum is divided by the count."""
    img = np.asarray(img)
    H, W = img.shape
    t = img.astype(acc)
    ylo, yhi, ly, hy, yin, gh = roi_axis(box[1], box[3], size[0], H, acc)
    xlo, xhi, lx, hx, xin, gw = roi_axis(box[0], box[2], size[1], W, acc)
    out = np.zeros(size, acc)
    for iy in range(gh):
        for ix in range(gw):
            r0, r1, c0, c1 = ylo[:, iy, None], yhi[:, iy, None], xlo[None, :, ix], xhi[None, :, ix]
            wy0, wy1, wx0, wx1 = hy[:, iy, None], ly[:, iy, None], hx[None, :, ix], lx[None, :, ix]
            s = (((wy0 * wx0) * t[r0, c0] + (wy0 * wx1) * t[r0, c1]) + (wy1 * wx0) * t[r1, c0]) + (wy1 * wx1) * t[r1, c1]
            out = out + np.where(yin[:, iy, None] & xin[None, :, ix], s, acc(0))
    out = out / acc(max(gh * gw, 1))
    assert out.dtype == acc
    return out, (gh, gw)


def gt_roi_masks(det, gt, det_gt_entry, size=(56, 56), ignore_ids=(-1, 10000), acc=F64):
    """``gt_assign.gt_roi_masks`` from dense masks: ``(masks [n, 1, *size], valid [n] uint8, grids [n, 2])``"""
    n = len(det["frame"])
    masks, valid, grids = np.zeros((n, 1) + tuple(size), acc), np.zeros(n, np.uint8), np.ones((n, 2), np.int64)
    for k in range(n):
        e = int(det_gt_entry[k])
        if e < 0 or int(gt["id"][e]) in ignore_ids or gt["frame"][e] != det["frame"][k]:
            continue
        valid[k] = 1
        img = M.rle_to_mask(gt["rle"][e], int(gt["img_height"][e]), int(gt["img_width"][e]))
        box = [det[c][k] for c in ("bb_left", "bb_top", "bb_right", "bb_bot")]
        masks[k, 0], grids[k] = roi_align(img, box, size, acc)
    return masks, valid, grids


# ------------------------------------------------------------------------------------------------ scenes
H, W = 97, 131


def rle_of(mask):
    """COCO's compressed string of a dense [h, w] mask"""
    flat = np.asarray(mask, np.uint8).T.reshape(-1)
    events = np.flatnonzero(np.diff(np.concatenate(([0], flat))) != 0)
    return M.rle_string(M.rle_counts_from_events(events, flat.size))


def _table(rows, columns):
    out = {c: np.asarray([r[c] for r in rows], dtype=object if c == "rle" else None) for c in columns}
    for c in ("frame", "id", "img_height", "img_width", "detection_id"):
        if c in out:
            out[c] = out[c].astype(np.int64).reshape(-1)
    for c in ("bb_top", "bb_left", "bb_bot", "bb_right"):
        if c in out:
            out[c] = out[c].astype(F64).reshape(-1)
    return out


BOX_COLUMNS = ("frame", "bb_top", "bb_left", "bb_bot", "bb_right")


def box_scene(seed=3):
    """``(det, gt, named)``: six frames of boxes with real-valued noise on every coordinate (no two totals tie).  Frame 1: more
    detections than ground truth, and far below them two pairs where greedy by IoU is not optimal; 2: fewer; 3: no detection
    (ground truth only); 4: no ground truth; 5: every pair below 0.5; 6: the cardinality case.  ``named``: {"greedy" |
    "cardinality": (rows of det, rows of gt)} of those two.  The rows of both files are shuffled: nothing relies on a file
    sorted by frame."""
    rng = np.random.default_rng(seed)
    noise = lambda: rng.uniform(-.4, .4)
    det, gt = [], []

    def box(frame, top, left, h, w, **kw):
        return dict(frame=frame, bb_top=top + noise(), bb_left=left + noise(), bb_bot=top + h + noise(), bb_right=left + w + noise(), **kw)
    next_id = itertools.count(1)
    for frame, n_gt, n_extra, n_drop in ((1, 4, 2, 0), (2, 5, 0, 2)):
        for g in range(n_gt):
            top, left, h, w = 40 + 180 * g + rng.uniform(0, 20), 60 + rng.uniform(0, 300), rng.uniform(60, 160), rng.uniform(30, 80)
            gt.append(box(frame, top, left, h, w, id=next(next_id)))
            if g >= n_drop:
                det.append(box(frame, top + rng.uniform(-.12, .12) * h, left + rng.uniform(-.12, .12) * w, h * rng.uniform(.9, 1.1), w * rng.uniform(.9, 1.1)))
        for e in range(n_extra):   # next to a ground-truth box, too far to be allowed
            det.append(box(frame, 40 + 180 * e, 500 + rng.uniform(0, 50), 100, 50))
    gt += [box(3, 50, 50, 100, 40, id=next(next_id)), box(3, 250, 80, 100, 40, id=next(next_id))]
    det += [box(4, 50, 50, 100, 40), box(4, 250, 80, 100, 40), box(4, 20, 300, 80, 30)]
    for k in range(3):       # shifted by 60 % of the width: IoU about 0.25
        gt.append(box(5, 30 + 150 * k, 100, 120, 50, id=next(next_id)))
        det.append(box(5, 30 + 150 * k, 130, 120, 50))
    named = {}
    for name, frame, top, wide, d_shift, g_shift in (("greedy", 1, 2000, 200, (10, -13), (0, 22)), ("cardinality", 6, 100, 95, (5, -25), (0, 25))):
        named[name] = (list(range(len(det), len(det) + 2)), list(range(len(gt), len(gt) + 2)))
        for s in g_shift:
            gt.append(box(frame, top, 300 + s, 180, wide, id=next(next_id)))
        for s in d_shift:
            det.append(box(frame, top, 300 + s, 180, wide))
    # shuffle the rows of both files and carry the named rows along
    pd_, pg = rng.permutation(len(det)), rng.permutation(len(gt))
    inv_d, inv_g = np.argsort(pd_), np.argsort(pg)
    named = {f: ([int(inv_d[r]) for r in dr], [int(inv_g[r]) for r in gr]) for f, (dr, gr) in named.items()}
    return _table([det[i] for i in pd_], BOX_COLUMNS), _table([gt[i] for i in pg], BOX_COLUMNS + ("id",)), named


MASK_COLUMNS = ("frame", "img_height", "img_width", "rle", "bb_left", "bb_top", "bb_right", "bb_bot")


def strips(cuts, y_ranges, gap=0):
    """disjoint rectangles: object k covers the columns [cuts[k] + gap, cuts[k + 1]) and the rows y_ranges[k]"""
    out = []
    for k, (y0, y1) in enumerate(y_ranges):
        m = np.zeros((H, W), np.uint8)
        m[y0:y1, cuts[k] + gap:cuts[k + 1]] = 1
        out.append(m)
    return out


def mask_scene(seed=4):
    """``(det, gt, dense)``: six frames of ``H x W = 97 x 131`` masks, disjoint within a side: vertical strips whose cuts differ
    between the sides, so that a detection overlaps several ground-truth masks.  Frame 1: more detections than ground truth;
    2: fewer; 3: ground truth only; 4: detections only; 5: no pair reaches 0.2; 6: the cardinality case at ``min_iou = 0.2``
    (g0, g1 = columns [0, 40), [40, 80); d0 = [10, 60), d1 = [0, 10): d0-g0 0.5, d0-g1 0.29, d1-g0 0.25, d1-g1 0).  One ground
    truth of frame 1 has the id 10000.  ``dense``: {("det" | "gt", row): mask}.  Boxes are the masks' extents."""
    rng = np.random.default_rng(seed)
    det, gt, dense = [], [], {}
    next_id = itertools.count(1)

    def add(rows, side, frame, masks, **kw):
        for m in masks:
            ys, xs = np.nonzero(m)
            dense[(side, len(rows))] = m
            rows.append(dict(frame=frame, img_height=H, img_width=W, rle=rle_of(m), bb_left=float(xs.min()), bb_top=float(ys.min()),
                             bb_right=float(xs.max() + 1), bb_bot=float(ys.max() + 1), **({"id": next(next_id)} if side == "gt" else {}), **kw))
    ys = lambda n, lo=0, hi=H: [tuple(sorted((int(rng.integers(lo, lo + 20)), int(rng.integers(hi - 25, hi))))) for _ in range(n)]
    add(gt, "gt", 1, strips([3, 37, 70, 101, 131], ys(4)[:3]))
    gt[1]["id"] = 10000
    add(det, "det", 1, strips([0, 22, 41, 66, 99, 128], ys(5), gap=1))
    add(gt, "gt", 2, strips([0, 25, 52, 80, 104, 131], ys(5)))
    add(det, "det", 2, strips([5, 49, 87, 131], ys(3), gap=2))
    add(gt, "gt", 3, strips([10, 60, 120], ys(2)))
    add(det, "det", 4, strips([10, 60, 120], ys(2)))
    add(gt, "gt", 5, strips([0, 60, 131], [(50, 90), (55, 97)]))
    add(det, "det", 5, strips([0, 50, 131], [(0, 14), (3, 17)]))
    add(gt, "gt", 6, strips([0, 40, 80], [(20, 30), (20, 30)]))
    add(det, "det", 6, [strips([10, 60], [(20, 30)])[0], strips([0, 10], [(20, 30)])[0]])
    return _table(det, MASK_COLUMNS), _table(gt, MASK_COLUMNS + ("id",)), dense


def assign_scene(det, gt, min_iou, dense=None):
    """The restatement of ``gt_assign.assign_gt`` frame by frame: ``(det_id, det_gt_entry, frames)`` with ``frames`` = {frame:
    (rows of det, rows of gt, iou, allowed, match)} in file order."""
    n = len(det["frame"])
    det_id, entry, frames = np.full(n, -1, np.int64), np.full(n, -1, np.int32), {}
    for f in np.unique(det["frame"]):
        dr, gr = np.flatnonzero(det["frame"] == f), np.flatnonzero(gt["frame"] == f)
        if dense is None:
            cols = ("bb_top", "bb_left", "bb_bot", "bb_right")
            iou = box_iou(np.stack([det[c][dr] for c in cols], 1), np.stack([gt[c][gr] for c in cols], 1))
            union_ok = None
        else:
            iou, union_ok = mask_iou([dense[("det", r)] for r in dr], [dense[("gt", r)] for r in gr])
        match, allowed = ref_assign(iou, min_iou, union_ok)
        hit = match >= 0
        entry[dr[hit]] = gr[match[hit]]
        det_id[dr[hit]] = gt["id"][gr[match[hit]]]
        frames[int(f)] = (dr, gr, iou, allowed, match)
    return det_id, entry, frames


ROI_COLUMNS = ("frame", "detection_id", "bb_left", "bb_top", "bb_right", "bb_bot")


def roi_scene():
    """``(det, det_gt_entry, what)`` over the ground truth of ``mask_scene`` (rows 0-2: frame 1, row 1 with the id 10000; 3-7:
    frame 2; 8-9: frame 3): boxes smaller than the output grid, about 130 px wide (grid 2 x 3), partly outside the frame on
    either side, with fractional corners, narrower than a pixel across a mask's border; a detection without a match, one matched
    to the id 10000, one in a frame without ground truth and one whose entry lies in another frame."""
    rows = [(1, (8.3, 30.2, 38.6, 50.9), 0, "small"), (1, (40.0, 10.0, 70.0, 90.0), 1, "ignored id"), (1, (20.0, 10.0, 90.0, 80.0), -1, "unmatched"),
            (1, (0.2, 0.3, 130.7, 96.6), 2, "wide"), (2, (-20.5, -10.25, 60.3, 40.9), 3, "negative side"),
            (2, (70.1, 50.2, 150.0, 110.0), 7, "beyond W and H"), (2, (51.6, 20.0, 51.9, 70.0), 4, "narrower than a pixel"),
            (2, (12.37, 5.81, 97.42, 88.13), 5, "fractional"), (3, (5.5, 6.5, 35.8, 27.2), 8, "small, ground truth only"),
            (4, (10.0, 10.0, 60.0, 60.0), -1, "frame without ground truth"), (6, (8.3, 30.2, 38.6, 50.9), 0, "entry of another frame")]
    det = _table([dict(frame=f, detection_id=k, bb_left=b[0], bb_top=b[1], bb_right=b[2], bb_bot=b[3]) for k, (f, b, _, _) in enumerate(rows)],
                 ROI_COLUMNS)
    return det, np.asarray([r[2] for r in rows], np.int32), [r[3] for r in rows]
