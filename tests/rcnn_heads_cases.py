"""Inputs shared by ``test_rcnn_heads_cpu.py`` (which asserts that the float32 and the float64 NMS references agree on every one
of them) and the GPU tests of the RoI heads."""
import numpy as np

from mpntrackseg_amd import synth

F32 = np.float32
MIXED_COUNTS = (0, 1, 63, 64, 65, 130)      # one call; the counts cross the word boundaries of the bit matrix


def random_boxes(seed, n, span=200.0, lo=10.0, hi=80.0):
    """[n, 4] float32 boxes: corners uniform in [0, span), sides uniform in [lo, hi); [n] float32 scores in (0, 1)"""
    u = synth.uniform01(seed, 5 * n).reshape(n, 5).astype(np.float64)
    x1, y1 = u[:, 0] * span, u[:, 1] * span
    b = np.stack([x1, y1, x1 + lo + u[:, 2] * (hi - lo), y1 + lo + u[:, 3] * (hi - lo)], axis=1).astype(F32)
    return b, (0.01 + 0.98 * u[:, 4]).astype(F32)


def edge_frames():
    """The hand-made frames: ``[(name, boxes, scores, expected kept rows in visiting order)]``, all at IoU threshold 0.5 and
    score threshold 0.25"""
    nan = float("nan")
    return [
        # A suppresses B (IoU 2/3), B would have suppressed C (2/3), IoU(A, C) = 3/7: C is kept
        ("chain", [[0, 0, 10, 10], [0, 2, 10, 12], [0, 4, 10, 14]], [0.9, 0.8, 0.7], [0, 2]),
        ("identical", [[3, 3, 9, 9]] * 3, [0.6, 0.6, 0.6], [0]),
        # row 3 comes first and suppresses row 1; the equal scores are then visited by increasing row: row 0 is kept and suppresses row 2
        ("tied",[[0, 0, 10, 10], [50, 50, 60, 60], [0, 1, 10, 11], [50, 51, 60, 61]], [0.5, 0.5, 0.5, 0.75], [3, 0]),
        ("zero_area", [[5, 5, 5, 5], [5, 5, 5, 5], [5, 5, 5, 9]], [0.9, 0.8, 0.7], [0, 1, 2]),          # 0 / 0 suppresses nothing
        ("exact_half", [[0, 0, 2, 2], [0, 0, 2, 1]], [0.9, 0.8], [0, 1]),                                   # IoU = 0.5 exactly: strict
        ("just_above", [[0, 0, 1024, 1024], [0, 0, 1024, 513]], [0.9, 0.8], [0]),                           # IoU = 513 / 1024
        ("threshold_equal", [[0, 0, 4, 4], [10, 0, 14, 4], [20, 0, 24, 4]], [0.25, 0.2499, 0.5], [2, 0]),   # a score equal to it is kept
        ("nan_score", [[0, 0, 4, 4], [0, 0, 4, 4], [10, 0, 14, 4]], [nan, 0.5, nan], [1]),
    ]


def nms_cases():
    """``[(name, boxes [n, 4], scores [n], ptr [F + 1], iou_threshold, score_threshold or None)]``"""
    cases = []
    parts = [random_boxes(100 + k, c) for k, c in enumerate(MIXED_COUNTS)]
    cases.append(("mixed", np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                  np.concatenate([[0], np.cumsum(MIXED_COUNTS)]).astype(np.int32), 0.5, None))
    cases.append(("mixed_filtered",) + cases[0][1:4] + (0.3, 0.2))
    edges = edge_frames()
    cases.append(("edges", np.concatenate([np.asarray(e[1], F32) for e in edges]), np.concatenate([np.asarray(e[2], F32) for e in edges]),
                  np.concatenate([[0], np.cumsum([len(e[2]) for e in edges])]).astype(np.int32), 0.5, 0.25))
    b, s = random_boxes(7, 4096, span=1500.0)
    cases.append(("frame_of_4096", b, s, np.array([0, 4096], np.int32), 0.5, None))
    return cases


def embedded_frame():
    """the 130-box frame of ``mixed`` alone, and as the 3rd of 5 frames: ``(boxes, scores, ptr, slice of the frame)`` twice"""
    b, s = random_boxes(105, 130)
    others = [random_boxes(200 + k, c) for k, c in enumerate((17, 64, 0, 70))]
    order = [others[0], others[1], (b, s), others[2], others[3]]
    ptr = np.concatenate([[0], np.cumsum([len(p[1]) for p in order])]).astype(np.int32)
    return (b, s, np.array([0, 130], np.int32)), (np.concatenate([p[0] for p in order]), np.concatenate([p[1] for p in order]), ptr, 2)


# ------------------------------------------------------------------------------------------------ small heads on a synthetic pyramid
SMALL = dict(channels=32, representation_size=64)
IMAGE_SIZE, ORIGINAL_SIZE = (64, 96), (90, 135)
LEVEL_SHAPES = ((16, 24), (8, 12), (4, 6), (2, 3))


def pyramid(seed, channels, frames=2):
    """four float32 levels [frames, channels, h, w] of a ``IMAGE_SIZE`` image, N(0, 1)"""
    return [synth.normal(seed, (frames, channels) + s, stream=l) for l, s in enumerate(LEVEL_SHAPES)]


def boxes_on_frames(seed, n, frames=2):
    """[n, 4] float32 boxes inside ``ORIGINAL_SIZE`` (sides 12 .. 60 pixels) and their frames, non-decreasing"""
    u = synth.uniform01(seed, 4 * n).reshape(n, 4).astype(np.float64)
    w, h = 12 + 48 * u[:, 2], 12 + 48 * u[:, 3]
    x1, y1 = u[:, 0] * (ORIGINAL_SIZE[1] - w), u[:, 1] * (ORIGINAL_SIZE[0] - h)
    return np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(F32), (np.arange(n) * frames // n).astype(np.int64)
