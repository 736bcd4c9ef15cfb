"""numpy restatement of ``mpntrackseg_amd.rcnn_heads`` (``csrc/rcnn_heads.hip``), without torchvision:

box branch     ``TwoMLPHead``, ``FastRCNNPredictor``, ``F.softmax`` and torchvision 0.6.0's ``BoxCoder.decode_single`` +
               ``resize_boxes``, in ``dtype`` = float64 (the reference) or float32 (a CPU evaluation of the same inputs);
NMS            the greedy rule ``include/mpnhip.h`` fixes for ``mpnhip_nms_batched``, in float64 and in float32 -- in float32
               every operation is a numpy float32 one, rounded on its own: the kernel's bits;
mask tail      the 3 x 3 convolutions, the 2 x 2 / 2 transposed convolution, the 1 x 1 logits, the sigmoid and aten's bilinear x 2
               for ``align_corners=False``;
table          ``FRCNNPreprocessor.step`` + ``save_results`` for given refined boxes.

``test_rcnn_heads_cpu.py`` pins these against float64 torch on the CPU."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
CLIP = math.log(1000.0 / 16)


# ------------------------------------------------------------------------------------------------ box branch
def linear(x, w, b, relu=False):
    y = x @ w.T + b
    return np.maximum(y, 0) if relu else y


def softmax(logits):
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def decode_single(deltas, proposals, weights=WEIGHTS, clip=CLIP, dtype=F64):
    """``BoxCoder.decode_single`` for one class: ``deltas`` [n, 4], ``proposals`` [n, 4] -> [n, 4]"""
    d, p = np.asarray(deltas, dtype), np.asarray(proposals, dtype)
    half, clip = dtype(0.5), dtype(F32(clip))
    out = np.zeros_like(d)
    for ax in (0, 1):
        w = p[:, 2 + ax] - p[:, ax]
        c = p[:, ax] + half * w
        dc = d[:, ax] / dtype(weights[ax])
        ds = d[:, 2 + ax] / dtype(weights[2 + ax])
        ds = np.where(ds > clip, clip, ds)
        pc = dc * w + c
        pw = np.exp(ds) * w
        out[:, ax], out[:, 2 + ax] = pc - half * pw, pc + half * pw
    assert out.dtype == dtype
    return out


def box_predict(h, w_cls, b_cls, w_box, b_box, proposals, label=1, weights=WEIGHTS, clip=CLIP, ratio_h=1.0, ratio_w=1.0, dtype=F64):
    """``mpnhip_box_predict``: ``dict(boxes, scores, logits, deltas, logit_mag, delta_mag)``; the ``*_mag`` are sum |h w| + |b|.
    ``ratio_h``, ``ratio_w`` are rounded to float32 first: the values the kernel is handed."""
    c = lambda a: np.asarray(a, dtype)
    h, w_cls, b_cls, w_box, b_box = c(h), c(w_cls), c(b_cls), c(w_box), c(b_box)
    rows = slice(4 * label, 4 * label + 4)
    logits = linear(h, w_cls, b_cls)
    deltas = linear(h, w_box[rows], b_box[rows])
    boxes = decode_single(deltas, proposals, weights, clip, dtype)
    ratio = np.array([F32(ratio_w), F32(ratio_h), F32(ratio_w), F32(ratio_h)], dtype)
    return dict(boxes=boxes * ratio, scores=softmax(logits)[:, label], logits=logits, deltas=deltas,
                logit_mag=np.abs(h) @ np.abs(w_cls).T + np.abs(b_cls), delta_mag=np.abs(h) @ np.abs(w_box[rows]).T + np.abs(b_box[rows]))


def box_extent(boxes):
    """the magnitude a coordinate's bound is stated in: the box's reach, the largest |coordinate| of its four"""
    return np.abs(np.asarray(boxes, F64)).max(axis=1, keepdims=True)


def case_bound(got32, ref64, mag):
    """the project's form of bound: ``max(16 u, 4 x the float32 CPU evaluation's worst error / magnitude) * magnitude``"""
    mag = np.asarray(mag, F64)
    ratio = float((np.abs(np.asarray(got32, F64) - ref64) / mag).max()) if ref64.size else 0.0
    return max(16 * U, 4 * ratio) * mag, ratio


# ------------------------------------------------------------------------------------------------ NMS
def iou(a, b, dtype):
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    zero = dtype(0)
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), zero)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), zero)
    inter = dtype(iw * ih)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dtype(inter / dtype(dtype(area_a + area_b) - inter))


def nms_frame(boxes, scores, iou_threshold, score_threshold=-math.inf, dtype=F32, margin=None):
    """The kept rows of one frame in visiting order.  ``margin`` (a list): receives |iou - threshold| of every comparison."""
    boxes, scores = np.asarray(boxes, dtype).reshape(-1, 4), np.asarray(scores, F32).reshape(-1)
    cand = [i for i in range(scores.size) if scores[i] >= F32(score_threshold)]        # NaN: never
    cand.sort(key=lambda i: (-float(scores[i]), i))
    thr = dtype(F32(iou_threshold))
    kept = []
    for i in cand:
        ok = True
        for j in kept:
            v = iou(boxes[j], boxes[i], dtype)
            if margin is not None and v == v:
                margin.append(abs(float(v) - float(thr)))
            if v > thr:
                ok = False
                break
        if ok:
            kept.append(i)
    return kept


def nms_batched(boxes, scores, ptr, iou_threshold, score_threshold=-math.inf, dtype=F32, margin=None):
    """``mpnhip_nms_batched``: ``(keep uint8 [n], order int32 [n], count int32 [F])``"""
    n = len(scores)
    keep, order, count = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.zeros(len(ptr) - 1, np.int32)
    for f in range(len(ptr) - 1):
        a, b = int(ptr[f]), int(ptr[f + 1])
        kept = nms_frame(boxes[a:b], scores[a:b], iou_threshold, score_threshold, dtype, margin)
        count[f] = len(kept)
        order[a:a + len(kept)] = np.asarray(kept, np.int32) + a
        keep[np.asarray(kept, np.int64) + a] = 1
    return keep, order, count


def nms_frame_fast(boxes, scores, iou_threshold, score_threshold=-math.inf, dtype=F32):
    """``nms_frame`` with the IoU row of a kept box computed at once (a frame of thousands); the same operations per pair"""
    boxes, scores = np.asarray(boxes, dtype).reshape(-1, 4), np.asarray(scores, F32).reshape(-1)
    cand = np.array([i for i in np.lexsort((np.arange(scores.size), -scores.astype(F64))) if scores[i] >= F32(score_threshold)], np.int64)
    b = boxes[cand]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    alive = np.ones(cand.size, bool)
    thr, zero = dtype(F32(iou_threshold)), dtype(0)
    kept = []
    for k in range(cand.size):
        if not alive[k]:
            continue
        kept.append(int(cand[k]))
        iw = np.maximum(np.minimum(b[k, 2], b[k + 1:, 2]) - np.maximum(b[k, 0], b[k + 1:, 0]), zero)
        ih = np.maximum(np.minimum(b[k, 3], b[k + 1:, 3]) - np.maximum(b[k, 1], b[k + 1:, 1]), zero)
        inter = iw * ih
        with np.errstate(invalid="ignore", divide="ignore"):
            v = inter / ((area[k] + area[k + 1:]) - inter)
        assert v.dtype == dtype
        alive[k + 1:] &= ~(v > thr)
    return kept


# ------------------------------------------------------------------------------------------------ mask tail
def conv3x3(x, w, b, relu=True):
    """``nn.Conv2d(cin, cout, 3, padding=1)`` + ReLU on ``x`` [n, cin, H, W]"""
    n, _, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((n, w.shape[0], H, W), x.dtype) + b[None, :, None, None]
    for dy in range(3):
        for dx in range(3):
            y = y + np.einsum("nchw,oc->nohw", xp[:, :, dy:dy + H, dx:dx + W], w[:, :, dy, dx])
    return np.maximum(y, 0) if relu else y


def conv_transpose2x2(x, w, b, relu=True):
    """``nn.ConvTranspose2d(cin, cout, 2, stride 2)`` + ReLU: ``w`` [cin, cout, 2, 2]"""
    n, _, H, W = x.shape
    y = np.zeros((n, w.shape[1], 2 * H, 2 * W), x.dtype)
    for dy in range(2):
        for dx in range(2):
            y[:, :, dy::2, dx::2] = np.einsum("nchw,co->nohw", x, w[:, :, dy, dx])
    y = y + b[None, :, None, None]
    return np.maximum(y, 0) if relu else y


def conv1x1(x, w, b):
    return np.einsum("nchw,oc->nohw", x, w[:, :, 0, 0]) + b[None, :, None, None]


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


def up2_axis(S, dtype):
    """aten's source index and weights of ``Upsample(scale_factor=2, mode='bilinear')`` per output index, in float32 (the index
    arithmetic is float32 whatever the data's type): ``(i0, i1, l0, l1)``"""
    dst = np.arange(2 * S, dtype=F32)
    src = np.maximum((dst + F32(0.5)) * F32(0.5) - F32(0.5), F32(0))
    i0 = src.astype(np.int64)
    i1 = np.minimum(i0 + 1, S - 1)
    l1 = src - i0.astype(F32)
    assert l1.dtype == F32
    return i0, i1, (F32(1) - l1).astype(dtype), l1.astype(dtype)


def upsample2(x):
    """[n, S, S] -> [n, 2 S, 2 S], rows and columns combined as aten combines them"""
    S = x.shape[-1]
    i0, i1, l0, l1 = up2_axis(S, x.dtype.type)
    top = l0[None, None, :] * x[:, i0][:, :, i0] + l1[None, None, :] * x[:, i0][:, :, i1]
    bot = l0[None, None, :] * x[:, i1][:, :, i0] + l1[None, None, :] * x[:, i1][:, :, i1]
    return l0[None, :, None] * top + l1[None, :, None] * bot


def roi_mask_finish(logits, label, up, dtype=F64):
    """``mpnhip_roi_mask_finish`` on ``logits`` [n, C, S, S]"""
    p = sigmoid(np.asarray(logits, dtype)[:, label])
    out = upsample2(p) if up == 2 else p
    assert out.dtype == dtype
    return out


def mask_branch(pooled, W, label=1, up=1, dtype=F64):
    """mask head + predictor + ``roi_mask_finish`` from the heads' ``state_dict`` arrays ``W``: [n, 1, 28 up, 28 up]"""
    x = np.asarray(pooled, dtype)
    i = 1
    while "mask_head.mask_fcn%d.weight" % i in W:
        x = conv3x3(x, W["mask_head.mask_fcn%d.weight" % i].astype(dtype), W["mask_head.mask_fcn%d.bias" % i].astype(dtype))
        i += 1
    x = conv_transpose2x2(x, W["mask_predictor.conv5_mask.weight"].astype(dtype), W["mask_predictor.conv5_mask.bias"].astype(dtype))
    x = conv1x1(x, W["mask_predictor.mask_fcn_logits.weight"].astype(dtype), W["mask_predictor.mask_fcn_logits.bias"].astype(dtype))
    return roi_mask_finish(x, label, up, dtype)[:, None]


def box_branch(pooled, W, proposals, label=1, ratio_h=1.0, ratio_w=1.0, dtype=F64):
    """box head + ``box_predict`` from the heads' ``state_dict`` arrays ``W``"""
    g = lambda k: W[k].astype(dtype)
    h = np.asarray(pooled, dtype).reshape(len(pooled), -1)
    h = linear(h, g("box_head.fc6.weight"), g("box_head.fc6.bias"), True)
    h = linear(h, g("box_head.fc7.weight"), g("box_head.fc7.bias"), True)
    return box_predict(h, g("box_predictor.cls_score.weight"), g("box_predictor.cls_score.bias"), g("box_predictor.bbox_pred.weight"),
                       g("box_predictor.bbox_pred.bias"), proposals, label, ratio_h=ratio_h, ratio_w=ratio_w, dtype=dtype)


# ------------------------------------------------------------------------------------------------ FRCNNPreprocessor's table
def det_table(boxes, scores, box_frame, frame_numbers, detect_score_thresh, nms_thresh, dtype=F32):
    """``FRCNNPreprocessor.step`` per frame + ``save_results`` on refined ``boxes`` float32 [n, 4] and ``scores`` float32 [n]
    (rows of a frame consecutive): float64 [m, 7] and the kept rows.  The NMS decides in ``dtype``; the columns are float32
    arithmetic, as the reference's float32 DataFrame columns."""
    boxes, scores, box_frame = np.asarray(boxes, F32), np.asarray(scores, F32), np.asarray(box_frame)
    rows, kept_rows = [], []
    for f in np.unique(box_frame):
        idx = np.flatnonzero(box_frame == f)
        for k in nms_frame(boxes[idx], scores[idx], nms_thresh, detect_score_thresh, dtype):
            b, r = boxes[idx[k]], idx[k]
            kept_rows.append(int(r))
            rows.append([float(frame_numbers[f]), -1.0, float(b[0] + F32(1)), float(b[1] + F32(1)), float(b[2] - b[0]), float(b[3] - b[1]),
                         float(scores[r])])
    return np.asarray(rows, F64).reshape(-1, 7), kept_rows
