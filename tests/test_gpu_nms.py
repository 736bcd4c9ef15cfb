"""mpnhip_nms_batched on the device: exact equality of keep, order and count with the float32 reference of rcnn_heads_ref.py on the
inputs of rcnn_heads_cases.py (test_rcnn_heads_cpu.py asserts that the float64 reference decides the same on every one of them, so
no case is left out for closeness to the threshold)."""
import math

import numpy as np
import pytest
import torch

import rcnn_heads_cases as K
import rcnn_heads_ref as R
from mpntrackseg_amd import capi, rcnn_heads as RH

pytestmark = pytest.mark.gpu
F32 = np.float32


def frames_of(ptr):
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def run(boxes, scores, ptr, iou_thr, score_thr):
    dev = torch.device("cuda:0")
    capi.path_counters(reset=True)
    keep, order, count = RH.nms_batched_raw(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), frames_of(ptr), iou_thr, score_thr,
                                            n_frames=len(ptr) - 1)
    torch.cuda.synchronize()
    assert capi.path_counters()["nms_batched"] == 1
    return keep.cpu().numpy(), order.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("case", K.nms_cases(), ids=lambda c: c[0])
def test_nms_equals_the_float32_reference(case):
    name, boxes, scores, ptr, iou_thr, score_thr = case
    st = -math.inf if score_thr is None else score_thr
    if name == "frame_of_4096":
        kept = R.nms_frame_fast(boxes, scores, iou_thr, st, F32)
        want = (np.zeros(4096, np.uint8), np.full(4096, -1, np.int32), np.array([len(kept)], np.int32))
        want[0][kept] = 1
        want[1][:len(kept)] = kept
    else:
        want = R.nms_batched(boxes, scores, ptr, iou_thr, st, F32)
    got = run(boxes, scores, ptr, iou_thr, score_thr)
    print(name, "kept", int(got[2].sum()), "of", len(scores), "in", len(ptr) - 1, "frames")
    for g, w, what in zip(got, want, ("keep", "order", "count")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, what)


def test_edge_frames_as_stated():
    """the hand-made frames against what their definitions say, not only against the reference"""
    edges = K.edge_frames()
    name, boxes, scores, ptr, iou_thr, score_thr = [c for c in K.nms_cases() if c[0] == "edges"][0]
    keep, order, count = run(boxes, scores, ptr, iou_thr, score_thr)
    for f, (ename, _, _, want) in enumerate(edges):
        a = int(ptr[f])
        assert count[f] == len(want), ename
        assert list(order[a:a + len(want)] - a) == want and (order[a + len(want):ptr[f + 1]] == -1).all(), ename
        assert sorted(np.flatnonzero(keep[a:ptr[f + 1]])) == sorted(want), ename


def test_a_frame_alone_and_inside_a_batch_gives_the_same_bits():
    (b, s, p), (bb, ss, pp, f) = K.embedded_frame()
    alone, inside = run(b, s, p, 0.5, None), run(bb, ss, pp, 0.5, None)
    a, e = int(pp[f]), int(pp[f + 1])
    assert np.array_equal(alone[0], inside[0][a:e]) and alone[2][0] == inside[2][f] and 0 < alone[2][0] < 130
    shifted = np.where(inside[1][a:e] >= 0, inside[1][a:e] - a, -1)
    assert np.array_equal(alone[1], shifted)
    # the wrapper: the kept rows frame after frame, and max_per_frame is the largest frame, not the cap
    dev = torch.device("cuda:0")
    rows = RH.nms_batched(torch.from_numpy(bb).to(dev), torch.from_numpy(ss).to(dev), frames_of(pp), 0.5).cpu().numpy()
    assert rows.dtype == np.int64 and np.array_equal(rows, inside[1][inside[1] >= 0])
    empty = RH.nms_batched(torch.zeros((0, 4), device=dev), torch.zeros((0,), device=dev), [], 0.5)
    assert empty.numel() == 0


def test_refusals():
    dev = torch.device("cuda:0")
    b, s = K.random_boxes(3, 12)
    tb, ts = torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev)
    with pytest.raises(ValueError):
        RH.nms_batched(tb, ts, [0] * 6 + [2] * 3 + [1] * 3, 0.5)          # a descending box_frame
    with pytest.raises(ValueError):
        RH.nms_batched(tb, ts, [0] * 11, 0.5)
    l = capi.load()
    keep, order = torch.zeros(12, dtype=torch.uint8, device=dev), torch.zeros(12, dtype=torch.int32, device=dev)
    count, ptr = torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([0, 12], dtype=torch.int32, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    rc = l.mpnhip_nms_batched(capi.ptr(tb), capi.ptr(ts), capi.ptr(ptr), 12, 1, 4097, -math.inf, 0.5, capi.ptr(keep), capi.ptr(order), capi.ptr(count),
                              capi.ptr(ws), ws.numel(), capi.stream_ptr())
    assert rc == -1 and b"max_per_frame 4097" in l.mpnhip_last_error()
    # a frame with more rows than max_per_frame says: count -1, nothing kept, nothing written out of place
    rc = l.mpnhip_nms_batched(capi.ptr(tb), capi.ptr(ts), capi.ptr(ptr), 12, 1, 8, -math.inf, 0.5, capi.ptr(keep), capi.ptr(order), capi.ptr(count),
                              capi.ptr(ws), ws.numel(), capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and int(count[0]) == -1 and int(keep.sum()) == 0 and bool((order == -1).all())
