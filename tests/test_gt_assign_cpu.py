"""Ground-truth assignment and RoI mask targets without a GPU: the numpy restatement (tests/gt_assign_ref.py) pinned by checks
that need none of the reference's libraries, the scenes of the GPU tests, and the host-side checks of the entry points."""
import ctypes

import numpy as np
import pytest

import gt_assign_ref as R
from mpntrackseg_amd import capi, gt_assign as GA, masks as M


# ------------------------------------------------------------------------------------------------ the assignment contract
def random_problem(rng, na, nb, p_forbidden):
    iou = rng.uniform(0.0, 1.0, (na, nb))
    return np.where(rng.random((na, nb)) < p_forbidden, rng.uniform(0.0, 0.49, (na, nb)), np.maximum(iou, 0.5))


def test_ref_assign_is_the_lexicographic_optimum_of_a_brute_force_search():
    rng = np.random.default_rng(11)
    shapes = [(na, nb) for na in range(6) for nb in range(6)]
    seen_drop = 0
    for na, nb in shapes:
        for p in (0.0, 0.3, 0.7, 1.0):
            iou = random_problem(rng, na, nb, p)
            match, allowed = R.ref_assign(iou, 0.5)
            assert np.array_equal(allowed, iou >= 0.5)
            want, count, total, gap = R.brute_force(iou, allowed)
            got_pairs = [(i, j) for i, j in enumerate(match) if j >= 0]
            assert all(allowed[i, j] for i, j in got_pairs)
            assert len(got_pairs) == count, (na, nb, p)
            assert abs(sum(1.0 - iou[i, j] for i, j in got_pairs) - total) <= 1e-12, (na, nb, p)
            if gap > 1e-9:
                assert np.array_equal(match, want), (na, nb, p)
            seen_drop += count < min(na, nb)
            if p == 1.0:
                assert (match == -1).all()
    assert seen_drop > 10   # problems where the padded solution had pairs to drop


def test_the_contract_prefers_more_pairs_to_a_better_pair():
    iou = np.array([[0.90, 0.67], [0.60, 0.30]])
    match, allowed = R.ref_assign(iou, 0.5)
    assert match.tolist() == [1, 0] and not allowed[1, 1]
    assert R.brute_force(iou, allowed)[0].tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------ box IoU
def literal_iou(box_a, box_b):
    """the reference's formula pair by pair in numpy scalars: (top, left, bottom, right), + 1 on every extent"""
    out = np.zeros((len(box_a), len(box_b)))
    for i, (t1, l1, b1, r1) in enumerate(box_a):
        for j, (t2, l2, b2, r2) in enumerate(box_b):
            t, l, b, r = np.maximum(t1, t2), np.maximum(l1, l2), np.minimum(b1, b2), np.minimum(r1, r2)
            inter = np.maximum(b - t + 1, 0) * np.maximum(r - l + 1, 0)
            area_1 = (b1 - t1 + 1) * (r1 - l1 + 1)
            area_2 = (b2 - t2 + 1) * (r2 - l2 + 1)
            out[i, j] = inter / (area_1 + area_2 - inter)
    return out


def test_box_iou_equals_the_formula_bit_for_bit():
    rng = np.random.default_rng(12)
    tl = rng.uniform(0, 300, (40, 2))
    a = np.concatenate((tl, tl + rng.uniform(1, 200, (40, 2))), axis=1)
    b = a[rng.permutation(40)[:25]] + rng.normal(0, 15, (25, 4))
    got, want = R.box_iou(a, b), literal_iou(a, b)
    assert np.array_equal(got, want) and (got > 0.5).any() and (got == 0).any()
    assert R.box_iou(a, a).diagonal().tolist() == [1.0] * 40
    assert R.box_iou(a, np.zeros((0, 4))).shape == (40, 0)


def test_scenes_hold_what_their_docstrings_say():
    det, gt, named = R.box_scene()
    _, _, frames = R.assign_scene(det, gt, 0.5)
    assert sorted(frames) == [1, 2, 4, 5, 6] and 3 in gt["frame"]
    for f, (dr, gr, iou, allowed, match) in frames.items():
        assert R.brute_force(iou, allowed)[3] > 1e-9, f
    assert frames[1][0].size > frames[1][1].size and frames[2][0].size < frames[2][1].size and frames[4][1].size == 0
    assert frames[5][2].size and not frames[5][3].any()
    dr, gr = named["greedy"]
    iou = R.box_iou(*[np.stack([t[c][r] for c in GA.BOX_TLBR], 1) for t, r in ((det, dr), (gt, gr))])
    assert (iou >= 0.5).all() and iou[0, 0] == iou.max() and iou[0, 0] + iou[1, 1] < iou[0, 1] + iou[1, 0]
    det, gt, dense = R.mask_scene()
    for min_iou in (0.5, 0.2):
        _, _, frames = R.assign_scene(det, gt, min_iou, dense)
        for f, (dr, gr, iou, allowed, match) in frames.items():
            assert R.brute_force(iou, allowed)[3] > 1e-9, (f, min_iou)
    assert frames[1][0].size > frames[1][1].size and frames[2][0].size < frames[2][1].size and not frames[5][3].any()
    assert frames[6][4].tolist() == [1, 0] and frames[6][2][0, 0] == 0.5 and not frames[6][3][1, 1]
    for (side, row), m in dense.items():   # the strings decode to the masks
        t = det if side == "det" else gt
        assert np.array_equal(M.rle_to_mask(t["rle"][row], R.H, R.W), m)


# ------------------------------------------------------------------------------------------------ RoIAlign
def test_roi_align_of_a_full_image_is_one_inside_and_zero_beyond_the_frame():
    ones = np.ones((R.H, R.W), np.uint8)
    for box in ((10.25, 7.5, 80.75, 60.0), (3.0, 2.0, 128.5, 95.0), (40.0, 40.0, 41.0, 41.0)):
        out, _ = R.roi_align(ones, box)
        assert (out == 1.0).all(), box
    out, (gh, gw) = R.roi_align(ones, (R.W + 1.5, 10.0, R.W + 90.0, 60.0))
    assert (out == 0.0).all() and gw == 2
    out, _ = R.roi_align(ones, (20.0, R.H + 1.25, 60.0, R.H + 30.0))
    assert (out == 0.0).all()


def test_roi_align_of_a_56_pixel_box_at_integer_corners_is_the_mean_of_four_pixels():
    rng = np.random.default_rng(13)
    img = (rng.random((R.H, R.W)) < 0.5).astype(np.uint8)
    x1, y1 = 31, 17
    out, grid = R.roi_align(img, (x1, y1, x1 + 56, y1 + 56))
    win = img[y1:y1 + 57, x1:x1 + 57].astype(np.float64)
    assert grid == (1, 1)
    assert np.array_equal(out, (win[:-1, :-1] + win[:-1, 1:] + win[1:, :-1] + win[1:, 1:]) / 4)
    out32, _ = R.roi_align(img, (x1, y1, x1 + 56, y1 + 56), acc=np.float32)
    assert out32.dtype == np.float32 and np.array_equal(out32, out.astype(np.float32))


def test_roi_align_of_a_box_narrower_than_a_pixel_uses_a_width_of_one():
    rng = np.random.default_rng(14)
    img = (rng.random((R.H, R.W)) < 0.5).astype(np.uint8)
    for acc in (np.float64, np.float32):
        thin, grid = R.roi_align(img, (50.25, 20.0, 50.55, 70.0), acc=acc)
        one, _ = R.roi_align(img, (50.25, 20.0, 51.25, 70.0), acc=acc)
        assert grid == (1, 1) and np.array_equal(thin, one) and thin.std() > 0
        flipped, _ = R.roi_align(img, (50.25, 20.0, 40.0, 70.0), acc=acc)   # x2 < x1: the same
        assert np.array_equal(flipped, one)


def test_roi_align_in_float32_stays_within_the_derived_bound_of_float64():
    rng = np.random.default_rng(15)
    img = (rng.random((R.H, R.W)) < 0.6).astype(np.uint8)
    for box in ((0.2, 0.3, 130.7, 96.6), (-20.5, -10.25, 60.3, 40.9), (70.1, 50.2, 150.0, 110.0), (5.5, 6.5, 35.8, 27.2)):
        a, (gh, gw) = R.roi_align(img, box)
        b, _ = R.roi_align(img, box, acc=np.float32)
        assert np.abs(a - b).max() <= (4 * gh * gw + 2) * 2.0 ** -24, box


# ------------------------------------------------------------------------------------------------ host checks
def test_overlapping_masks_are_refused_with_the_mots_loaders_error():
    det, gt, dense = R.mask_scene()
    rows = {k: v.copy() for k, v in gt.items()}
    a, b = np.flatnonzero(rows["frame"] == 2)[:2]
    rows["rle"][b] = R.rle_of(dense[("gt", a)] | dense[("gt", b)])
    with pytest.raises(ValueError, match="Objects with overlapping masks in frame 2"):
        GA.mask_rows(rows)
    rows["rle"][b] = R.rle_of(np.ones((R.H + 1, R.W), np.uint8))
    with pytest.raises(ValueError, match="do not describe a 97 x 131 mask"):
        GA.mask_rows(rows)
    loaded = GA.mask_rows(gt)
    assert loaded["run_row"].size and (np.diff(loaded["run_row"]) >= 0).all()


def test_entry_point_argument_checks_without_gpu():
    """everything below returns before a kernel is launched (the non-null pointers are host dummies, never dereferenced)"""
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    capi.path_counters(reset=True)

    def box(a_boxes=p, n_a=3, b_boxes=p, n_b=4, a_ptr=p, b_ptr=p, cell_ptr=p, n_frames=1, cells=12, iou=p, allowed=p, cost=p):
        return l.mpnhip_box_iou_costs(a_boxes, n_a, b_boxes, n_b, a_ptr, b_ptr, cell_ptr, n_frames, cells, 0.5, iou, allowed, cost, None)

    def overlap(table=p, table_cells=20, table_ptr=p, a_ptr=p, n_a=3, b_ptr=p, n_b=4, cell_ptr=p, n_frames=1, cells=12, iou=p, allowed=p, cost=p):
        return l.mpnhip_overlap_iou_costs(table, table_cells, table_ptr, a_ptr, n_a, b_ptr, n_b, cell_ptr, n_frames, cells, 0.5, iou, allowed,
                                          cost, None)

    def finish(match_b=p, allowed=p, cells=12, cell_ptr=p, a_ptr=p, n_a=3, b_ptr=p, n_b=4, n_frames=1, gt_ids=p, n_out=3, entry=p, det_id=p):
        return l.mpnhip_gt_assign_finish(match_b, allowed, cells, cell_ptr, a_ptr, n_a, b_ptr, n_b, n_frames, gt_ids, None, None, n_out, entry,
                                         det_id, None)

    def roi(labels=p, n_frames=1, h=97, w=131, det_ptr=p, gt_ptr=p, boxes=p, n_dets=3, entry=p, n_out=3, gt_label=p, gt_ids=p, n_gt=4,
            ignore=p, n_ignore=2, ph=56, pw=56, masks=p, valid=p):
        return l.mpnhip_roi_align_labels(labels, n_frames, h, w, det_ptr, gt_ptr, boxes, n_dets, None, entry, n_out, gt_label, gt_ids, n_gt,
                                         ignore, n_ignore, ph, pw, masks, valid, None)
    # nothing to do: successful no-ops, whatever is null
    assert l.mpnhip_box_iou_costs(None, 3, None, 0, None, None, None, 1, 0, 0.5, None, None, None, None) == 0
    assert l.mpnhip_box_iou_costs(None, 0, None, 0, None, None, None, 0, 0, 0.5, None, None, None, None) == 0
    assert l.mpnhip_overlap_iou_costs(None, 0, None, None, 0, None, 4, None, 1, 0, 0.5, None, None, None, None) == 0
    assert l.mpnhip_gt_assign_finish(None, None, 0, None, None, 0, None, 4, 1, None, None, None, 0, None, None, None) == 0
    assert l.mpnhip_roi_align_labels(None, 0, 97, 131, None, None, None, 0, None, None, 0, None, None, 0, None, 0, 56, 56, None, None, None) == 0
    # null pointers with work to do, by the operator's name
    for call, name, args in ((box, b"box_iou_costs", ("a_boxes", "b_boxes", "a_ptr", "b_ptr", "cell_ptr", "iou", "allowed", "cost")),
                             (overlap, b"overlap_iou_costs", ("table", "table_ptr", "a_ptr", "b_ptr", "cell_ptr", "iou", "allowed", "cost")),
                             (finish, b"gt_assign_finish", ("match_b", "allowed", "cell_ptr", "a_ptr", "b_ptr", "gt_ids", "entry", "det_id")),
                             (roi, b"roi_align_labels", ("labels", "det_ptr", "gt_ptr", "boxes", "entry", "gt_label", "gt_ids", "ignore", "masks",
                                                         "valid"))):
        for arg in args:
            assert call(**{arg: None}) == -1, (name, arg)
            assert name in l.mpnhip_last_error(), (name, arg)
        for bad in (dict(n_frames=-1), dict(n_frames=65536), dict(n_frames=0)):
            assert call(**bad) == -1, (name, bad)
            assert name in l.mpnhip_last_error(), (name, bad)
    for call in (box, overlap, finish):
        assert call(cells=-1) == -1 and call(n_a=-1) == -1 and call(n_b=-1) == -1
        assert call(cells=1 << 31) == -4
    assert overlap(table_cells=1 << 31) == -4 and overlap(table_cells=-1) == -1
    assert finish(n_out=-1) == -1
    for bad in (dict(ph=0), dict(pw=-1), dict(h=-1), dict(h=1 << 16, w=1 << 15), dict(n_dets=-1), dict(n_gt=-1), dict(n_ignore=-1), dict(n_out=-1)):
        assert roi(**bad) == -1, bad
        assert b"roi_align_labels" in l.mpnhip_last_error(), bad
    assert not any(capi.path_counters(reset=True).values())


def test_host_wrappers_refuse_bad_input_before_the_device():
    import torch
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        GA.box_iou_costs(np.zeros((0, 4)), np.zeros((0, 4)), [0], [0], device="cpu")
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        GA.gt_roi_masks({"frame": [1]}, {}, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        GA.overlap_iou_costs(torch.zeros(4, dtype=torch.int32), [0, 4], [0, 1], [0, 1])
