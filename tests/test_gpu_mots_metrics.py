"""The MOTS metrics on the device (``csrc/mots_eval.hip`` through ``mpntrackseg_amd.mots_eval`` and
``tracker.evaluate_mots_sequence``) against the numpy restatements of tests/mots_metrics_ref.py: every integer and decision
equal, the float metrics within 1e-12 relative (a handful of double operations on equal integers).  The restatements and the
host bookkeeping are pinned to the evaluation kit's own results by tests/test_mots_metrics_cpu.py (g22).  Images are 37 x 29
(hw = 1073: the frames of a launch start at every residue modulo 4) unless a case says otherwise."""
import numpy as np
import pytest
import torch

import full_masks_ref as FR
import mots_metrics_ref as R
from mpntrackseg_amd import capi, mots_eval as ME, tracker

pytestmark = pytest.mark.gpu

H, W = 37, 29
HW = H * W


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(R.GOLDEN))


def check_paint(run_entry, run_begin, run_end, frame_ptr, n_entries, hw=HW):
    want = R.paint_label_runs(run_entry, run_begin, run_end, frame_ptr, n_entries, hw)
    got = ME.paint_label_runs(run_entry, run_begin, run_end, frame_ptr, n_entries, hw, dev())
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    return want


def test_paint_label_runs():
    ptr = np.array([0, 2, 2, 5])   # 3 frames, the middle one without entries
    # one run covers a whole frame; the others stay -1
    lab = check_paint([3], [0], [HW], ptr, 5)
    assert (lab[2] == 3).all() and (lab[:2] == -1).all()
    # every pixel of the two frames with entries is a run of its own
    pos = np.arange(HW)
    ent = np.concatenate((pos % 2, 2 + pos % 3))
    lab = check_paint(ent, np.concatenate((pos, pos)), np.concatenate((pos, pos)) + 1, ptr, 5)
    assert (lab[0] >= 0).all() and (lab[1] == -1).all() and (lab[2] >= 2).all()
    # a run continues across a column's end, and the runs COCO would give for random blobs
    lab = check_paint([0, 4], [H - 7, 5 * H - 1], [H + 13, 5 * H + 1], ptr, 5)
    assert (lab[0, H - 7:H + 13] == 0).all() and (lab[0] == 0).sum() == 20 and (lab[2] == 4).sum() == 2
    blobs, bptr = R.ellipse_labels(np.random.default_rng(1), 3, H, W, [3, 0, 2])
    assert np.array_equal(check_paint(*R.label_runs(blobs), bptr, 5), blobs)
    # no run at all
    assert (check_paint([], [], [], ptr, 5) == -1).all()
    # an entry outside the list, an end beyond the frame, a negative begin, an empty run: they paint nothing, the others do
    lab = check_paint([5, -1, 1, 0, 0, 4], [0, 0, HW - 3, -1, 9, 10], [10, 10, HW + 1, 4, 9, 20], ptr, 5)
    assert (lab[2, 10:20] == 4).all() and (lab >= 0).sum() == 10
    # no frame
    assert tuple(ME.paint_label_runs([], [], [], [0], 0, HW, dev()).shape) == (0, HW)


def check_overlap(labels_a, labels_b, a_ptr, b_ptr):
    """the table of one launch against np.add.at; returns (table on the device, table_ptr, counters of the two forms)"""
    F = len(a_ptr) - 1
    want, want_tp = R.label_overlap(labels_a, labels_b, a_ptr, b_ptr)
    capi.path_counters(reset=True)
    table, tp = ME.label_overlap(torch.from_numpy(np.ascontiguousarray(labels_a, np.int32)).to(dev()),
                                 torch.from_numpy(np.ascontiguousarray(labels_b, np.int32)).to(dev()), a_ptr, b_ptr)
    pc = capi.path_counters()
    got = table.cpu().numpy()
    assert np.array_equal(tp, want_tp) and got.dtype == np.int32
    assert np.array_equal(got, want)
    hw = np.asarray(labels_a).size // F if F else 0
    for f in range(F):
        assert got[tp[f]:tp[f + 1]].sum() == hw
    return table, tp, (pc["label_overlap_lds"], pc["label_overlap_global"])


def check_match(table, tp, L):
    want = R.frame_match(table.cpu().numpy(), tp, L["a_ptr"], L["b_ptr"], L["a_ignore"], L["a_traj"], L["b_traj"], L["n_a_traj"],
                         L["n_b_traj"])
    got = ME.frame_match(table, tp, L["a_ptr"], L["b_ptr"], L["a_ignore"], L["a_traj"], L["b_traj"], L["n_a_traj"], L["n_b_traj"])
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    return want


def small_frames():
    """case (a): 3 frames of 37 x 29 with 2-3 objects a side, as rectangles [y0, y1) x [x0, x1): an ignore region, a pair at IoU
    exactly 0.5 (3 x 2 against the same shifted by one row: 4 / 8), a prediction mostly inside the ignore region, a miss"""
    a = [[(2, 10, 2, 7, 0), (14, 17, 10, 12, 1), (0, H, 22, W, -1)],
         [(2, 10, 2, 7, 0), (20, 30, 3, 9, 2)],
         [(5, 12, 5, 12, 1), (14, 22, 2, 7, 2), (0, H, 22, W, -1)]]
    b = [[(3, 11, 2, 7, 0), (15, 18, 10, 12, 1), (26, 32, 20, 26, 2)],
         [(2, 10, 3, 8, 3), (0, 5, 20, 25, 1)],
         [(5, 12, 5, 12, 0), (30, 35, 2, 7, 2)]]

    def side(frames):
        lab = np.full((len(frames), H, W), -1, np.int32)
        ptr, traj = [0], []
        for f, rects in enumerate(frames):
            for y0, y1, x0, x1, t in rects:
                lab[f, y0:y1, x0:x1] = len(traj)
                traj.append(t)
            ptr.append(len(traj))
        return np.ascontiguousarray(lab.transpose(0, 2, 1)).reshape(len(frames), HW), np.asarray(ptr, np.int64), np.asarray(traj, np.int32)
    la, a_ptr, a_traj = side(a)
    lb, b_ptr, b_traj = side(b)
    return {"labels_a": la, "labels_b": lb, "a_ptr": a_ptr, "b_ptr": b_ptr, "a_ignore": (a_traj < 0).astype(np.uint8), "a_traj": a_traj,
            "b_traj": b_traj, "n_a_traj": 3, "n_b_traj": 4}


def test_overlap_and_match_small_frames_lds_form():
    L = small_frames()
    table, tp, forms = check_overlap(L["labels_a"], L["labels_b"], L["a_ptr"], L["b_ptr"])
    assert forms == (3, 0)
    o = check_match(table, tp, L)
    # frame 0: a clear match, the pair at exactly 0.5 (no CLEAR match, an id match), an ignored prediction
    assert o["match_b"].tolist()[:3] == [0, -1, -1] and (o["inter"][1], o["uni"][1]) == (0, 0)
    assert o["id_match"].tolist() == [[1, 0, 0, 1], [1, 1, 0, 0], [0, 0, 0, 0]] and o["b_ignored"].tolist()[:3] == [False, False, True]
    assert o["match_b"].tolist()[3:] == [3, -1, 5, -1, -1] and o["b_matched"].tolist() == [True, False, False, True, False, True, False]


def test_overlap_and_match_crowded_scene_global_form(gold):
    L = R.scene_lists(gold["crowded:gt"], gold["crowded:pred"])
    table, tp, forms = check_overlap(L["labels_a"], L["labels_b"], L["a_ptr"], L["b_ptr"])
    assert forms == (0, 3) and (np.diff(tp) > R.LDS_CELLS).all()
    o = check_match(table, tp, L)
    assert (o["match_b"] >= 0).sum() == int(gold["crowded:m:tp"])


def test_overlap_and_match_both_forms_in_one_launch(gold):
    """a crowded frame between two frames of three objects a side (64 x 48)"""
    C = R.scene_lists(gold["crowded:gt"][:1], gold["crowded:pred"][:1])
    h, w = gold["crowded:gt"].shape[1:]
    rng = np.random.default_rng(3)
    fa, fa_ptr = R.ellipse_labels(rng, 2, h, w, [3, 3], 4.0, 12.0)
    fb, fb_ptr = R.ellipse_labels(rng, 2, h, w, [3, 2], 4.0, 12.0)
    na, nb = int(C["a_ptr"][-1]), int(C["b_ptr"][-1])

    def weave(few, crowded, n_c):   # entries: the first small frame's 3, the crowded frame's, the last small frame's
        first = few[0]
        mid = np.where(crowded[0] >= 0, crowded[0] + 3, -1)
        last = np.where(few[1] >= 0, few[1] + n_c, -1)
        return np.stack((first, mid, last)).astype(np.int32)
    L = {"labels_a": weave(fa, C["labels_a"], na), "labels_b": weave(fb, C["labels_b"], nb),
         "a_ptr": np.array([0, 3, 3 + na, 6 + na]), "b_ptr": np.array([0, 3, 3 + nb, 5 + nb])}
    L["a_ignore"] = (np.arange(6 + na) % 7 == 3).astype(np.uint8)
    L["a_traj"] = np.where(L["a_ignore"] == 1, -1, np.arange(6 + na) % 50).astype(np.int32)
    L["b_traj"] = (np.arange(5 + nb) % 40).astype(np.int32)
    L["n_a_traj"], L["n_b_traj"] = 50, 40
    table, tp, forms = check_overlap(L["labels_a"], L["labels_b"], L["a_ptr"], L["b_ptr"])
    assert forms == (2, 1)
    check_match(table, tp, L)


def test_overlap_labels_outside_the_frames_range_count_as_no_object():
    L = small_frames()
    la, lb = L["labels_a"].copy(), L["labels_b"].copy()
    lb[1, 100:140] = 0              # an entry of frame 0 in frame 1
    lb[0, 7:19] = 3                 # ... of frame 1 in frame 0
    la[2, 500:520] = 8              # beyond the list
    la[2, 520:523] = -5
    lb[2, 1000:HW] = 1 << 30
    table, tp, _ = check_overlap(la, lb, L["a_ptr"], L["b_ptr"])
    clean = R.label_overlap(L["labels_a"], L["labels_b"], L["a_ptr"], L["b_ptr"])[0]
    assert not np.array_equal(table.cpu().numpy(), clean)


def test_overlap_without_frames_and_with_empty_lists():
    table, tp, forms = check_overlap(np.zeros((0, HW), np.int32), np.zeros((0, HW), np.int32), [0], [0])
    assert table.numel() == 0 and forms == (0, 0)
    rng = np.random.default_rng(5)
    junk = rng.integers(-3, 4, (2, HW)).astype(np.int32)
    table, tp, forms = check_overlap(junk, junk[::-1], [0, 0, 0], [0, 0, 0])   # one cell a frame: every pixel is "no object"
    assert table.cpu().tolist() == [HW, HW] and forms == (2, 0)
    L = {"a_ptr": [0, 0, 0], "b_ptr": [0, 0, 0], "a_ignore": [], "a_traj": [], "b_traj": [], "n_a_traj": 0, "n_b_traj": 0}
    check_match(table, tp, L)
    # objects on one side only
    la, a_ptr = R.ellipse_labels(rng, 2, H, W, [2, 1])
    table, tp, _ = check_overlap(la, junk, a_ptr, [0, 0, 0])
    L = {"a_ptr": a_ptr, "b_ptr": [0, 0, 0], "a_ignore": [0, 1, 0], "a_traj": [0, -1, 1], "b_traj": [], "n_a_traj": 2, "n_b_traj": 0}
    check_match(table, tp, L)
    table, tp, _ = check_overlap(junk, la, [0, 0, 0], a_ptr)
    L = {"a_ptr": [0, 0, 0], "b_ptr": a_ptr, "a_ignore": [], "a_traj": [], "b_traj": [0, 1, 1], "n_a_traj": 0, "n_b_traj": 2}
    assert check_match(table, tp, L)["b_area"].tolist() == [int((la == e).sum()) for e in range(3)]


def test_overlap_one_cell_takes_every_pixel():
    n = 256 * 256
    table, tp, forms = check_overlap(np.zeros((1, n), np.int32), np.zeros((1, n), np.int32), [0, 1], [0, 1])
    assert table.cpu().tolist() == [0, 0, 0, n] and forms == (1, 0)
    # ... and in the global form: the same pair among 70 x 70 entries
    table, tp, forms = check_overlap(np.full((1, n), 69, np.int32), np.full((1, n), 5, np.int32), [0, 70], [0, 70])
    assert int(table[70 * 71 + 6]) == n and forms == (0, 1)


def test_overlap_full_hd_frame_of_random_blobs():
    """1080 x 1920: several blocks per frame, both forms over the same images (the LDS form sees the first 40 / 60 entries,
    the pixels of the others count as no object)"""
    h, w = 1080, 1920
    rng = np.random.default_rng(7)
    la, _ = R.ellipse_labels(rng, 1, h, w, [70], 20.0, 160.0)
    lb, _ = R.ellipse_labels(rng, 1, h, w, [70], 20.0, 160.0)
    assert (la >= 0).mean() > 0.2 and (lb >= 0).mean() > 0.2
    _, tp, forms = check_overlap(la, lb, [0, 70], [0, 70])
    assert forms == (0, 1) and tp[1] == 71 * 71
    _, tp, forms = check_overlap(la, lb, [0, 40], [0, 60])
    assert forms == (1, 0)


@pytest.mark.parametrize("scene", R.SCENES)
def test_evaluate_mots_files_equals_the_kit(gold, scene, tmp_path):
    pred, gt, seq_length = R.scene_files(gold, scene, tmp_path)
    capi.path_counters(reset=True)
    for fpl in (1, 5, 64):
        m = ME.evaluate_mots_files(pred, gt, seq_length, frames_per_launch=fpl, device=dev(), details=True)
        R.assert_metrics_equal(m, gold, scene)
    pc = capi.path_counters()
    assert pc["label_overlap_lds" if scene == "cases" else "label_overlap_global"] > 0


def tracked_sequence():
    """six frames (1 .. 6) of 48 x 64 with four detections each (RoI masks 28 x 28), host arrays: detections of another class
    that only occlude, two tracks that swap, a dropped detection, a frame the tracker left empty; the ground truth as id
    images (frame 0 is empty): the masks of the first three detections of a frame moved by a pixel, one missing, and an ignore
    strip"""
    h, w, F, per = 48, 64, 6, 4
    rng = np.random.default_rng(22)
    n = F * per
    masks = FR.blob_masks(rng, n, 28, 28)
    frame = np.repeat(np.arange(1, F + 1), per)
    cx, cy = np.tile([14.0, 44.0, 20.0, 40.0], F) + rng.uniform(-3, 3, n), np.tile([12.0, 14.0, 34.0, 30.0], F) + rng.uniform(-3, 3, n)
    bw, bh = rng.uniform(16, 26, n), rng.uniform(14, 22, n)
    boxes = np.stack((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), axis=1)
    ped = np.tile(np.arange(per), F)
    ped[per * 3:per * 3 + 2] = [1, 0]                                  # two tracks swap in frame 4
    label = np.full(n, 2)
    label[3::per] = 1                                                  # the fourth detection of every frame is a car
    keep = np.ones(n, bool)
    keep[[5, 8, 9, 10, 11]] = False                                    # one dropped in frame 2, frame 3 left empty
    gt = np.zeros((F + 1, h, w), np.uint16)
    for f in range(1, F + 1):                                          # what ALL detections of the frame paste, moved by a pixel
        idx = np.flatnonzero(frame == f)
        lab = np.roll(FR.np_frame(masks[idx], boxes[idx], h, w, 0.5)[0], tuple(rng.integers(-1, 2, 2)), axis=(0, 1))
        for j in range(3):
            if not (f == 5 and j == 2):
                gt[f][lab == j] = 2001 + j
    for f in (1, 2, 4):
        win = gt[f, :, w - 8:]
        win[win == 0] = 10000
    return masks, boxes, frame, ped, label, keep, gt, (h, w), F


def test_evaluate_mots_sequence_equals_the_route_through_the_text_file(tmp_path):
    """the metrics straight from the pasted label images equal those of the rows save_results_to_file writes"""
    masks, boxes, frame, ped, label, keep, gt, (h, w), F = tracked_sequence()
    n = masks.shape[0]
    node_preds = torch.from_numpy(masks).to(dev()).view(n, 1, 28, 28)
    gt_txt = R.write_txt(str(tmp_path / "gt.txt"), R.id_image_rows(gt))
    keep_t = torch.from_numpy(keep).to(dev())
    rles = tracker.to_full_masks(node_preds, boxes, frame, keep_t, (h, w), 0.5, frames_per_launch=4)
    tracker.save_results_to_file(str(tmp_path / "pred.txt"), frame, ped, label, (h, w), rles, keep)
    want = ME.evaluate_mots_files(str(tmp_path / "pred.txt"), gt_txt, F, frames_per_launch=3, device=dev(), details=True)
    assert want["tp"] >= 8 and want["fn"] >= 1 and want["fp"] >= 1 and want["id_switches"] >= 1 and want["n_tr"] == 3 * (F - 1) - 1
    for fpl in (1, 4, 64):
        got = tracker.evaluate_mots_sequence(node_preds, boxes, frame, torch.from_numpy(ped).to(dev()), label, keep_t, (h, w), gt_txt, F,
                                             mask_threshold=0.5, frames_per_launch=fpl, details=True)
        assert sorted(got) == sorted(want)
        for k in ME.METRIC_NAMES:
            assert got[k] == want[k], (k, got[k], want[k])
        assert np.array_equal(got["per_frame"], want["per_frame"]) and got["trajectories"] == want["trajectories"]
    loaded = ME.load_mots_txt(gt_txt)
    assert tracker.evaluate_mots_sequence(node_preds, boxes, frame, ped, label, keep, (h, w), loaded, F)["sMOTSA"] == want["sMOTSA"]
