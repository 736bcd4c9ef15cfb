"""Full-frame MOTS masks on the device (``csrc/full_masks.hip`` through ``mpntrackseg_amd.masks`` and ``tracker.to_full_masks`` /
``tracker.mots_sequence``) against the numpy restatement of tests/full_masks_ref.py, bit for bit: labels, winner values (NaN
positions as NaN positions), run boundaries, their counts and the COCO strings.  The restatement itself is pinned to the
reference by tests/test_full_masks_cpu.py.  Image 37 x 53 unless a case says otherwise: one tile row, four tile columns, two
event blocks per frame; the g20 inputs (96 x 128) add a second tile row, the crowded frame a second chunk of boxes."""
import numpy as np
import pytest
import torch

from mpntrackseg_amd import masks as M, tracker
from mpntrackseg_amd.capi import MpnhipError
import full_masks_ref as R

pytestmark = pytest.mark.gpu

H, W, THR = 37, 53, 0.5


def dev():
    return torch.device("cuda:0")


def same_values(got, want):
    """Bit for bit, with NaN positions compared as NaN positions."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def expect(masks, boxes, frame_ptr, h, w, thr):
    """The restatement over the frames of one launch: labels [F, h, w] numbered over the launch's list, values, positions sorted
    by (detection, position), counts per detection, strings."""
    labels, values, pos, counts, strings = [], [], [], [], []
    for f in range(len(frame_ptr) - 1):
        a, b = int(frame_ptr[f]), int(frame_ptr[f + 1])
        lab, val = R.np_frame(masks[a:b], boxes[a:b], h, w, thr)
        p, c = R.np_events(lab, b - a)
        strings += R.np_strings(lab, b - a)
        labels.append(np.where(lab >= 0, lab + a, -1).astype(np.int32))
        values.append(val)
        pos.append(p)
        counts.append(c)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return np.stack(labels), np.stack(values), cat(pos, np.int64), cat(counts, np.int64), strings


def check_launch(masks, boxes, frame_ptr, h=H, w=W, thr=THR):
    """One launch against the restatement; returns the restatement's (labels, values, strings)."""
    masks, boxes = np.asarray(masks, np.float32), np.asarray(boxes, np.float64).reshape(-1, 4)
    n = masks.shape[0]
    want_lab, want_val, want_pos, want_cnt, want_str = expect(masks, boxes, frame_ptr, h, w, thr)
    t = torch.from_numpy(masks).to(dev())
    labels, values = M.paste_unique_masks(t.view(n, 1, *masks.shape[1:]), boxes, frame_ptr, (h, w), thr, return_values=True)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (len(frame_ptr) - 1, w, h) and tuple(values.shape) == tuple(labels.shape)
    got_lab = labels.cpu().numpy().transpose(0, 2, 1)
    assert np.array_equal(got_lab, want_lab)
    assert same_values(values.cpu().numpy().transpose(0, 2, 1), want_val)
    # without the value image the labels are the same
    assert torch.equal(M.paste_unique_masks(t, torch.from_numpy(boxes).to(dev()), torch.tensor(frame_ptr), (h, w), thr), labels)
    pos, counts = M.mask_run_events(labels, n)
    assert np.array_equal(counts, want_cnt) and np.array_equal(pos, want_pos)
    ends = np.cumsum(counts)
    got_str = [M.rle_string(M.rle_counts_from_events(pos[e - c:e], h * w)) for e, c in zip(ends, counts)]
    assert got_str == want_str
    # every string decodes to its detection's pixels, and the masks of a frame are pairwise disjoint
    total = np.zeros((len(frame_ptr) - 1, h, w), np.int64)
    for f in range(len(frame_ptr) - 1):
        for j in range(int(frame_ptr[f]), int(frame_ptr[f + 1])):
            m = M.rle_to_mask(got_str[j], h, w)
            assert np.array_equal(m, got_lab[f] == j)
            total[f] += m
    assert total.max(initial=0) <= 1
    # the same bits on every call
    again, again_values = M.paste_unique_masks(t, boxes, frame_ptr, (h, w), thr, return_values=True)
    assert torch.equal(again, labels) and torch.equal(again_values.view(torch.int32), values.view(torch.int32))
    pos2, counts2 = M.mask_run_events(labels, n)
    assert np.array_equal(pos2, pos) and np.array_equal(counts2, counts)
    return want_lab, want_val, want_str


def blobs(seed, n, mh=56, mw=56):
    return R.blob_masks(np.random.default_rng(seed), n, mh, mw)


def empty_string(h=H, w=W):
    return M.rle_string([h * w])


# ------------------------------------------------------------------------------------------------ the g20 inputs
def test_g20_inputs(golden):
    z = golden("g20_full_masks.npz")
    (h, w), thr = z["img_shape"].tolist(), float(z["mask_threshold"])
    lab, _, strings = check_launch(z["masks"], z["boxes"], z["frame_ptr"].tolist(), h, w, thr)
    # ... and the reference's masks where the literal pipeline decides by more than 1e-5 (tests/test_full_masks_cpu.py)
    from test_full_masks_cpu import _excluded
    ref = np.unpackbits(z["binary_bits"])[:11 * h * w].reshape(11, h, w)
    fp = z["frame_ptr"]
    for f in range(3):
        a, b = int(fp[f]), int(fp[f + 1])
        ex = _excluded(R.literal_paste(z["masks"][a:b], z["boxes"][a:b], h, w), thr)
        got = (lab[f][None] == np.arange(a, b).reshape(-1, 1, 1))
        assert np.array_equal(got[:, ~ex], ref[a:b][:, ~ex].astype(bool))
        if not ex.any():
            assert strings[a:b] == [str(s) for s in z["rle"][a:b]]


# ------------------------------------------------------------------------------------------------ boxes
BOX_CASES = {
    "inside": [[10.0, 8.0, 30.0, 28.0]],
    "cut_left": [[-12.5, 6.0, 14.0, 30.0]],
    "cut_top": [[12.0, -9.25, 40.0, 20.0]],
    "cut_right": [[35.0, 5.0, 70.5, 31.0]],
    "cut_bottom": [[8.0, 20.0, 44.0, 55.75]],
    "outside_left": [[-60.0, 5.0, -20.0, 30.0]],
    "outside_below": [[5.0, 80.0, 30.0, 120.0]],
    "trunc_toward_zero": [[0.0, 0.0, 20.0, 20.0]],        # expands to -0.357...: int64 conversion gives 0, a floor would give -1
    "r_less_than_l": [[30.0, 5.0, 10.0, 25.0]],
    "zero_area": [[20.0, 15.0, 20.0, 15.0]],
    "shrinking_5x4": [[20.2, 10.2, 24.3, 13.3]],
    "larger_than_image": [[-40.0, -60.0, 120.0, 110.0]],
}


@pytest.mark.parametrize("name", list(BOX_CASES))
def test_single_boxes(name):
    boxes = np.array(BOX_CASES[name], np.float64)
    bx = R.np_expand_boxes(boxes, 56)[0].tolist()
    if name == "trunc_toward_zero":
        raw = 10.0 - 10.0 * (58.0 / 56.0)
        assert -1.0 < raw < 0.0 and bx[:2] == [0, 0]
    if name == "r_less_than_l":
        assert bx[2] < bx[0] and bx[4] == 1
    if name == "zero_area":
        assert bx == [20, 15, 20, 15, 1, 1]
    if name == "shrinking_5x4":
        assert bx[4:] == [5, 4]
    if name == "larger_than_image":
        assert bx[0] < 0 and bx[1] < 0 and bx[2] >= W and bx[3] >= H
    lab, val, strings = check_launch(blobs(3, 1) + np.float32(0.2), boxes, [0, 1])
    covered = int((lab >= 0).sum())
    if name.startswith("outside") or name == "r_less_than_l":
        assert covered == 0 and strings == [empty_string()] and not val.any()
    elif name != "zero_area":
        assert covered > 0
    if name.startswith("cut") or name == "larger_than_image":   # the mask reaches the border it is cut by
        edge = {"cut_left": lab[0][:, 0], "cut_top": lab[0][0], "cut_right": lab[0][:, -1], "cut_bottom": lab[0][-1],
                "larger_than_image": lab[0][0]}[name]
        assert (edge >= 0).any()


def test_non_square_mask():
    rng = np.random.default_rng(4)
    masks = rng.random((3, 7, 12)).astype(np.float32)
    boxes = np.array([[3.0, 4.0, 40.0, 30.0], [20.5, 2.0, 50.0, 20.0], [10.0, 10.0, 14.0, 13.0]])
    # the scale of the expansion comes from the mask WIDTH, for both axes
    assert R.np_expand_boxes(boxes[:1], 12)[0].tolist() != R.np_expand_boxes(boxes[:1], 7)[0].tolist()
    lab, _, _ = check_launch(masks, boxes, [0, 3])
    assert len(np.unique(lab)) >= 3


# ------------------------------------------------------------------------------------------------ the arg-max
def test_identical_detections_first_wins():
    m = blobs(5, 1) + np.float32(0.2)
    box = [[5.0, 4.0, 45.0, 33.0]]
    lab, _, strings = check_launch(np.concatenate((m, m)), np.array(box * 2), [0, 2])
    assert (lab == 0).any() and not (lab == 1).any() and strings[1] == empty_string() and strings[0] != empty_string()


def test_nan_mask_over_a_valid_one():
    valid = blobs(6, 1) + np.float32(0.3)
    nan = np.full((1, 56, 56), np.nan, np.float32)
    boxes = np.array([[5.0, 4.0, 40.0, 33.0], [20.0, 10.0, 50.0, 30.0]])
    for order in ((0, 1), (1, 0)):
        masks = np.concatenate((valid, nan))[list(order)]
        lab, val, strings = check_launch(masks, boxes[list(order)], [0, 2])
        i_nan = order.index(1)
        assert np.isnan(val).any() and not (lab == i_nan).any() and strings[i_nan] == empty_string()
        assert (lab[np.isnan(val)] == -1).all() and (lab == 1 - i_nan).any()   # NaN wins the pixel and fails the threshold
    # partly NaN, and both NaN at a pixel: the first NaN is the winner (the values are NaN either way)
    part = valid.copy()
    part[0, 20:30, 20:30] = np.nan
    check_launch(np.concatenate((part, nan, valid)), np.array([boxes[0], boxes[1], boxes[0]]), [0, 3])


def test_negative_and_tied_values():
    """Values below zero lose to the zeros outside the other boxes (and the pixel is unset either way); +-inf and exact ties."""
    rng = np.random.default_rng(7)
    masks = (rng.random((4, 9, 9)).astype(np.float32) - np.float32(0.4)) * np.float32(2)
    masks[1, 2:5, 2:5] = np.inf
    masks[2, 3:6, 3:6] = -np.inf
    masks[3] = masks[0]
    boxes = np.array([[2.0, 2.0, 30.0, 30.0], [10.0, 5.0, 45.0, 35.0], [0.0, 0.0, 52.0, 36.0], [2.0, 2.0, 30.0, 30.0]])
    check_launch(masks, boxes, [0, 4])
    check_launch(masks[:1], boxes[:1], [0, 1])            # alone in its frame: no zero to lose to
    check_launch(masks, boxes, [0, 1, 4], thr=0.25)


# ------------------------------------------------------------------------------------------------ frames and runs
def test_frames_of_one_launch():
    """A frame without detections between two that have some, a frame with a single detection, and several in the others."""
    masks = blobs(8, 8) + np.float32(0.15)
    boxes = R.random_boxes(np.random.default_rng(8), 8, H, W, lo=8.0, hi=45.0)
    lab, _, _ = check_launch(masks, boxes, [0, 4, 4, 5, 8])
    assert (lab[1] == -1).all() and len(np.unique(lab[0])) >= 3 and set(np.unique(lab[2]).tolist()) <= {-1, 4}
    check_launch(masks[:0], boxes[:0], [0, 0, 0])         # no detection at all
    check_launch(masks, boxes, [0, 8])
    check_launch(masks, boxes, list(range(9)))


def test_runs_at_the_ends_of_the_image():
    ones = np.ones((1, 8, 8), np.float32)
    # a box that covers the whole image with a margin: every pixel set, the string of the full mask, pixel 0 and the last pixel
    lab, _, strings = check_launch(ones, np.array([[-10.0, -10.0, 70.0, 50.0]]), [0, 1])
    assert (lab == 0).all() and strings == [M.rle_string([0, H * W])]
    # touching pixel 0 only / the last pixel only
    lab, _, strings = check_launch(ones, np.array([[-6.0, -6.0, 9.0, 7.0]]), [0, 1])
    assert lab[0, 0, 0] == 0 and lab[0, -1, -1] == -1 and M.rle_counts(strings[0])[0] == 0
    lab, _, strings = check_launch(ones, np.array([[44.0, 30.0, 60.0, 44.0]]), [0, 1])
    assert lab[0, -1, -1] == 0 and lab[0, 0, 0] == -1 and M.rle_counts(strings[0]).size % 2 == 0
    # full columns: the run goes on across the column ends -- three counts for a band of whole columns
    lab, _, strings = check_launch(ones, np.array([[12.0, -20.0, 30.0, 60.0]]), [0, 1])
    cols = np.flatnonzero((lab[0] == 0).all(axis=0))
    assert cols.size >= 10 and M.rle_counts(strings[0]).size == 3
    # two frames whose runs meet at the frame boundary: the last pixel of one and pixel 0 of the next stay separate runs
    lab, _, strings = check_launch(np.concatenate((ones, ones)), np.array([[44.0, 30.0, 60.0, 44.0], [-6.0, -6.0, 9.0, 7.0]]), [0, 1, 2])
    assert lab[0, -1, -1] == 0 and lab[1, 0, 0] == 1 and M.rle_counts(strings[1])[0] == 0


def test_crowded_frame_takes_a_second_chunk_of_boxes():
    """More than 256 detections in one frame: the cull walks them in chunks and keeps the order across chunks."""
    rng = np.random.default_rng(9)
    n = 300
    masks = rng.random((n, 4, 4)).astype(np.float32)
    boxes = R.random_boxes(rng, n, H, W, lo=3.0, hi=14.0)
    masks[3] = 2.0                 # above every other value: detection 3 owns its box ...
    boxes[3] = (10.0, 10.0, 20.0, 20.0)
    masks[290] = masks[3]          # ... also against its copy in the second chunk: on a tie the earlier one wins
    boxes[290] = boxes[3]
    lab, _, strings = check_launch(masks, boxes, [0, n])
    assert (lab >= 256).any() and (lab == 3).any() and strings[290] == empty_string()


# ------------------------------------------------------------------------------------------------ tracker level
def _np_full_masks(node_preds, boxes, frame, keep, h, w, thr):
    out = np.full(len(frame), None, dtype=object)
    for f in np.unique(frame[keep]):
        ids = np.flatnonzero(keep & (frame == f))
        lab, _ = R.np_frame(node_preds[ids, 0], boxes[ids], h, w, thr)
        for j, s in zip(ids, R.np_strings(lab, ids.size)):
            out[j] = s
    return out


def test_to_full_masks_keep_and_frames_per_launch(golden):
    z = golden("g20_full_masks.npz")
    (h, w), thr = z["img_shape"].tolist(), float(z["mask_threshold"])
    masks, boxes = z["masks"], z["boxes"]
    frame = np.array([1] * 6 + [2] + [4] * 4)            # no detection in frame 3
    node_preds = torch.from_numpy(masks).view(11, 1, 56, 56).to(dev())
    everything = np.ones(11, bool)
    all_kept = _np_full_masks(masks[:, None], boxes, frame, everything, h, w, thr)
    # dropping a detection that owns pixels hands them to the others
    lab_all, _ = R.np_frame(masks[:6], boxes[:6], h, w, thr)
    owner = int(np.bincount(lab_all[lab_all >= 0], minlength=6).argmax())
    keep = everything.copy()
    keep[[owner, 8]] = False
    want = _np_full_masks(masks[:, None], boxes, frame, keep, h, w, thr)
    assert sum(a != b for a, b in zip(want[:6], all_kept[:6])) >= 2      # the dropped one and whoever inherits its pixels
    results = []
    for fpl in (1, 2, 8):
        got = tracker.to_full_masks(node_preds, boxes, frame, torch.from_numpy(keep).to(dev()), (h, w), thr, frames_per_launch=fpl)
        assert got.dtype == object and got.shape == (11,)
        assert got[owner] is None and got[8] is None and got.tolist() == want.tolist()
        results.append(got.tolist())
    assert results[0] == results[1] == results[2]
    assert tracker.to_full_masks(node_preds, boxes, frame, everything, (h, w), thr).tolist() == all_kept.tolist()
    # frames that are not in order are grouped by a stable sort; nothing kept: nothing to do
    perm = np.array([6, 0, 7, 1, 2, 8, 3, 9, 4, 10, 5])
    got = tracker.to_full_masks(node_preds[perm], boxes[perm], frame[perm], keep[perm], (h, w), thr, frames_per_launch=2)
    assert got.tolist() == want[perm].tolist()
    assert tracker.to_full_masks(node_preds, boxes, frame, ~everything, (h, w), thr).tolist() == [None] * 11
    with pytest.raises(MpnhipError, match="mask_threshold"):
        tracker.to_full_masks(node_preds, boxes, frame, everything, (h, w), 0.0)


def test_mots_sequence(golden, tmp_path):
    from test_gpu_tracker_tail import _cfg, _inputs, _model
    z = golden("g17_window_tail.npz")
    args, x_ext = _inputs(z, "s")
    frame = np.asarray(z["s:frame"])
    n = frame.shape[0]
    boxes = R.random_boxes(np.random.default_rng(10), n, H, W, lo=6.0, hi=40.0)
    model = _model()
    # the small model's mask probabilities lie in 0.13 .. 0.56 with a median of 0.39 (the reference's own, g17_window_tail_masks.npz):
    # a threshold of 0.4 sets a good third of every mask, the configs' 0.5 next to nothing
    thr = 0.4
    res, rles = tracker.mots_sequence(model, *args, x_ext=x_ext, boxes=boxes, img_shape=(H, W), mask_threshold=thr, min_track_len=3,
                                      **_cfg(z, "s1"))
    plain = tracker.track_sequence(model, *args, x_ext=x_ext, min_track_len=3, **_cfg(z, "s1"))
    assert torch.equal(res.ped_ids, plain.ped_ids) and torch.equal(res.keep, plain.keep) and torch.equal(res.node_preds, plain.node_preds)
    keep, node_preds = res.keep.cpu().numpy(), res.node_preds.cpu().numpy()
    assert keep.any() and not keep.all() and tuple(node_preds.shape) == (n, 1, 56, 56)
    want = _np_full_masks(node_preds, boxes, frame, keep, H, W, thr)
    assert rles.shape == (n,) and rles.tolist() == want.tolist()
    assert sum(s is not None and s != empty_string() for s in rles) >= 3
    # the text file parses back to the same rows
    path = tmp_path / "seq.txt"
    rows = tracker.save_results_to_file(str(path), frame, res.ped_ids, 2, (H, W), rles, res.keep)
    parsed = [line.split(" ") for line in path.read_text().splitlines()]
    assert len(parsed) == int(keep.sum()) == len(rows)
    ped = res.ped_ids.cpu().numpy()
    order = [i for i in np.lexsort((ped, frame)) if keep[i]]
    for i, cols in zip(order, parsed):
        assert [int(c) for c in cols[:5]] == [int(frame[i]), int(ped[i]) + 2001, 2, H, W] and cols[5] == rles[i]
    with pytest.raises(MpnhipError, match="mask branch"):
        tracker.mots_sequence(model, *args, x_ext=None, boxes=boxes, img_shape=(H, W), **_cfg(z, "s1"))
