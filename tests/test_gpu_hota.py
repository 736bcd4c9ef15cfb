"""HOTA on the device (``csrc/hota.hip`` through ``mpntrackseg_amd.hota_eval`` and ``tracker.evaluate_hota_sequence``) against the
numpy restatements of tests/hota_ref.py, operator by operator.  Integers, decisions, ``sim`` (one IEEE division of equal
integers) and ``b_removed`` are exact; float64 sums are within 1e-9 relative, absolute where the value is 0 (each is fewer than
10^6 additions of terms in [0, 1], so another order moves it by less than 10^6 x 2.2e-16).  The restatements and the host
bookkeeping are pinned to TrackEval's own results by tests/test_hota_cpu.py (g23)."""
import numpy as np
import pytest
import torch

import full_masks_ref as FR
import hota_ref as HR
import mots_metrics_ref as R
from mpntrackseg_amd import hota_eval as HE, mots_eval as ME, tracker

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(HR.GOLDEN))


@pytest.fixture(scope="module")
def gold22():
    return dict(np.load(R.GOLDEN))


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def ref_tables(L):
    return R.label_overlap(L["labels_a"], L["labels_b"], L["a_ptr"], L["b_ptr"])


def similarity_pair(table, tp, L):
    """frame_similarity on the device and restated, compared; the table is a host array"""
    want = HR.frame_similarity(table, tp, L["a_ptr"], L["b_ptr"], L["a_ignore"], L["b_scored"])
    got = HE.frame_similarity(torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(dev()), tp, L["a_ptr"], L["b_ptr"], L["a_ignore"],
                              L["b_scored"])
    assert np.array_equal(got["sim_ptr"], want["sim_ptr"]) and host(got["sim"]).dtype == np.float64
    assert np.array_equal(host(got["sim"]), want["sim"])
    assert np.array_equal(host(got["b_removed"]), want["b_removed"]) and np.array_equal(got["b_removed_host"], want["b_removed_host"])
    HR.close(host(got["row_sum"]), want["row_sum"], "row_sum")
    HR.close(host(got["col_sum"]), want["col_sum"], "col_sum")
    return got, want


def compare_acc(got, want, keys):
    for k in keys:
        if k in ("potential", "loca"):
            HR.close(host(got[k]), want[k], k)
        else:
            assert np.array_equal(host(got[k]), want[k]), k


def check_launches(launches, G, T):
    """every operator over the launches (table, table_ptr, lists), both ways; returns the two accumulators, the restated
    launches and the association sums"""
    acc_g, acc_w = HE.accumulators(G, T, dev()), HR.accumulators(G, T)
    pairs = []
    for table, tp, L in launches:
        got, want = similarity_pair(table, tp, L)
        HE.accumulate_alignment(got, L["a_traj"], L["b_traj"], acc_g)
        HR.accumulate_alignment(want, L["a_traj"], L["b_traj"], acc_w)
        pairs.append((got, want, L))
    compare_acc(acc_g, acc_w, ("potential", "gt_count", "tr_count"))
    for got, want, L in pairs:
        s_g, s_w = HE.frame_scores(got, L["a_traj"], L["b_traj"], acc_g), HR.frame_scores(want, L["a_traj"], L["b_traj"], acc_w)
        HR.close(s_g, s_w, "score")
        assert ((s_g == 0) == (s_w == 0)).all()
        mb = HE.assign_frames(want, L["a_traj"], L["b_traj"], s_w)
        HE.alpha_accumulate(got, L["a_traj"], L["b_traj"], mb, HE.ALPHAS, acc_g)
        HR.alpha_accumulate(want, L["a_traj"], L["b_traj"], mb, HR.ALPHAS, acc_w)
    compare_acc(acc_g, acc_w, ("tp", "loca", "matches_count"))
    out_g, out_w = HE.association(acc_g), HR.association(acc_w)
    HR.close(out_g["ass"], out_w["ass"], "association")
    assert np.array_equal(out_g["tp"], out_w["tp"])
    return acc_g, acc_w, pairs, out_w


def test_operators_small_frames():
    L = HR.small_frames()
    table, tp = ref_tables(L)
    acc_g, acc_w, pairs, out = check_launches([(table, tp, L)], L["n_a_traj"], L["n_b_traj"])
    S = pairs[0][1]
    # frame 0: a clear pair, the pair at IoU exactly 4 / 8, a prediction four columns of six inside the ignore region: removed
    assert S["sim"][4] == 0.5 and S["b_removed"].tolist() == [0, 0, 1, 0, 0, 0, 0] and S["sim"][S["sim_ptr"][1]] > 0.5
    assert acc_w["gt_count"].tolist() == [2, 2, 2] and acc_w["tr_count"].tolist() == [2, 2, 1, 1]
    assert out["tp"][0] == 4 and out["tp"][9] == 4 and out["tp"][10] == 3 and out["tp"][18] == 1   # 0.5 counts up to alpha 0.5


def crowded_frame(gold22):
    return HR.scene_lists(gold22["crowded:gt"][:1], gold22["crowded:pred"][:1])


def test_operators_crowded_frame(gold22):
    """64 x 48 with 110 objects a side: a table of more than 4096 cells, G x T > 10^4, several blocks per association sum"""
    L = crowded_frame(gold22)
    table, tp = ref_tables(L)
    assert tp[-1] > R.LDS_CELLS and L["n_a_traj"] * L["n_b_traj"] > 10 ** 4 and L["n_a_traj"] * L["n_b_traj"] > 4 * 1024
    acc_g, acc_w, pairs, out = check_launches([(table, tp, L)], L["n_a_traj"], L["n_b_traj"])
    assert out["tp"][0] == 110 and pairs[0][1]["b_removed"].sum() >= 1


def test_operators_small_and_crowded_frames_in_one_launch(gold22):
    """a crowded frame between the small ones (the operators read tables, so the frames of a launch need not share a size)"""
    Ls, Lc = HR.small_frames(), crowded_frame(gold22)
    (ts, tps), (tc, tpc) = ref_tables(Ls), ref_tables(Lc)
    na, nb = int(Lc["a_ptr"][-1]), int(Lc["b_ptr"][-1])
    sa, sb = Ls["a_ptr"], Ls["b_ptr"]

    def weave(key, ptr):   # the entries of small frames 0 and 1, of the crowded frame, of small frame 2
        cut = int(ptr[2])
        return np.concatenate((Ls[key][:cut], Lc[key], Ls[key][cut:]))
    L = {"a_ptr": np.array([0, sa[1], sa[2], sa[2] + na, sa[3] + na]), "b_ptr": np.array([0, sb[1], sb[2], sb[2] + nb, sb[3] + nb]),
         "a_ignore": weave("a_ignore", sa), "a_traj": weave("a_traj", sa), "b_traj": weave("b_traj", sb),
         "b_scored": weave("b_scored", sb)}
    table = np.concatenate((ts[:tps[2]], tc, ts[tps[2]:]))
    tp = np.concatenate(([0], np.cumsum((np.diff(L["a_ptr"]) + 1) * (np.diff(L["b_ptr"]) + 1))))
    acc_g, acc_w, pairs, out = check_launches([(table, tp, L)], Lc["n_a_traj"], Lc["n_b_traj"])
    assert out["tp"][0] == 110 + 4


def split(L, table, tp, f0, f1):
    """the frames [f0, f1) of a launch as a launch of their own"""
    a0, a1, b0, b1 = int(L["a_ptr"][f0]), int(L["a_ptr"][f1]), int(L["b_ptr"][f0]), int(L["b_ptr"][f1])
    P = {"a_ptr": L["a_ptr"][f0:f1 + 1] - a0, "b_ptr": L["b_ptr"][f0:f1 + 1] - b0}
    for k, lo, hi in (("a_ignore", a0, a1), ("a_traj", a0, a1), ("b_traj", b0, b1), ("b_scored", b0, b1)):
        P[k] = L[k][lo:hi]
    return table[tp[f0]:tp[f1]], tp[f0:f1 + 1] - tp[f0], P


def test_tracks_across_a_launch_boundary_give_the_same_bits(gold):
    """the association scene (tracks present in every frame) in one launch and in launches of 5 + 1 + 6 frames: a cell of
    ``potential`` and the LocA sums are added in frame order either way"""
    L = HR.scene_lists(gold["association:gt"], gold["association:pred"])
    table, tp = ref_tables(L)
    G, T = L["n_a_traj"], L["n_b_traj"]
    one = check_launches([(table, tp, L)], G, T)
    cut = check_launches([split(L, table, tp, 0, 5), split(L, table, tp, 5, 6), split(L, table, tp, 6, 12)], G, T)
    for k in ("potential", "gt_count", "tr_count", "tp", "loca", "matches_count"):
        assert np.array_equal(host(one[0][k]), host(cut[0][k])), k
    assert one[1]["gt_count"].max() == 11 and (one[3]["tp"] > 0).all() and one[3]["tp"][0] > one[3]["tp"][18]


def test_no_ids_and_frames_empty_on_one_side():
    rng = np.random.default_rng(11)
    H, W = 37, 29
    la, a_ptr = R.ellipse_labels(rng, 3, H, W, [2, 0, 2])
    lb, b_ptr = R.ellipse_labels(rng, 3, H, W, [0, 3, 2])
    L = {"labels_a": la, "labels_b": lb, "a_ptr": a_ptr, "b_ptr": b_ptr, "a_ignore": np.array([0, 0, 0, 1], np.uint8),
         "b_scored": np.array([1, 1, 0, 1, 1], np.uint8), "a_traj": np.array([0, 1, 1, -1], np.int32),
         "b_traj": np.array([0, 1, -1, 0, 2], np.int32)}
    table, tp = ref_tables(L)
    acc_g, acc_w, pairs, out = check_launches([(table, tp, L)], 2, 3)
    assert pairs[0][1]["sim_cells"] == 4 and acc_w["gt_count"].tolist() == [1, 2]
    # G = 0: no ground-truth id (every a-entry is an ignore row), T = 0: no scored prediction; then neither
    for G, T in ((0, 3), (2, 0), (0, 0)):
        P = dict(L)
        if G == 0:
            P["a_ignore"], P["a_traj"] = np.ones(4, np.uint8), np.full(4, -1, np.int32)
        if T == 0:
            P["b_scored"], P["b_traj"] = np.zeros(5, np.uint8), np.full(5, -1, np.int32)
        acc_g, acc_w, pairs, out = check_launches([(table, tp, P)], G, T)
        assert (out["ass"] == 0).all() and (out["tp"] == 0).all() and (pairs[0][1]["sim"] == 0).all()
    # no entry and no frame at all
    E = {"a_ptr": [0], "b_ptr": [0], "a_ignore": [], "b_scored": [], "a_traj": [], "b_traj": []}
    check_launches([(np.zeros(0, np.int32), np.array([0]), E)], 2, 3)


def test_junk_matches_and_trajectory_indices_write_nothing(gold):
    """match_b outside the frame's entries (or the list, or int32's ends), trajectory indices outside [0, G) / [0, T): such
    entries take no part, and nothing is written outside the accumulators"""
    L = HR.scene_lists(gold["association:gt"][:3], gold["association:pred"][:3])
    table, tp = ref_tables(L)
    G, T = L["n_a_traj"], L["n_b_traj"]
    n_a, n_b = int(L["a_ptr"][-1]), int(L["b_ptr"][-1])
    P = dict(L)
    P["a_traj"], P["b_traj"] = L["a_traj"].copy(), L["b_traj"].copy()
    P["a_traj"][[1, 9]] = [G, -(2 ** 31)]
    P["b_traj"][[0, 5, 12]] = [T + 7, 2 ** 31 - 1, -3]
    want = HR.frame_similarity(table, tp, P["a_ptr"], P["b_ptr"], P["a_ignore"], P["b_scored"])
    clean = HE.assign_frames(want, L["a_traj"], L["b_traj"], want["sim"])   # (any assignment inside the frames)
    mb = clean.copy()
    mb[[0, 2, 3, 4, 6]] = [n_b, -(2 ** 31), 2 ** 31 - 1, int(L["b_ptr"][1]) + 1, -2]   # (entry 4 of frame 0: a prediction of frame 1)
    # the accumulators inside guarded buffers
    acc = HE.accumulators(G, T, dev())
    guards = {}
    for k in ("potential", "gt_count", "tr_count", "tp", "loca", "matches_count"):
        n = acc[k].numel()
        big = torch.full((n + 128,), 77, dtype=acc[k].dtype, device=dev())
        big[64:64 + n] = 0
        guards[k], acc[k] = big, big[64:64 + n]
    acc_w = HR.accumulators(G, T)
    got = HE.frame_similarity(torch.from_numpy(table).to(dev()), tp, P["a_ptr"], P["b_ptr"], P["a_ignore"], P["b_scored"])
    HE.accumulate_alignment(got, P["a_traj"], P["b_traj"], acc)
    HR.accumulate_alignment(want, P["a_traj"], P["b_traj"], acc_w)
    HR.close(HE.frame_scores(got, P["a_traj"], P["b_traj"], acc), HR.frame_scores(want, P["a_traj"], P["b_traj"], acc_w), "score")
    HE.alpha_accumulate(got, P["a_traj"], P["b_traj"], mb, HE.ALPHAS, acc)
    HR.alpha_accumulate(want, P["a_traj"], P["b_traj"], mb, HR.ALPHAS, acc_w)
    compare_acc(acc, acc_w, ("potential", "gt_count", "tr_count", "tp", "loca", "matches_count"))
    assert 0 < acc_w["tp"][0] < (clean >= 0).sum() and acc_w["gt_count"].sum() == (L["a_traj"] >= 0).sum() - 2
    for k, big in guards.items():
        n = big.numel() - 128
        assert (big[:64] == 77).all() and (big[64 + n:] == 77).all(), k


@pytest.mark.parametrize("scene", HR.SCENES)
def test_evaluate_hota_files_equals_trackeval(gold, gold22, scene, tmp_path):
    pred, gt, T = HR.scene_files(gold, gold22, scene, tmp_path)
    for fpl in (1, 5, 64):
        first = HE.evaluate_hota_files(pred, gt, T, frames_per_launch=fpl, device=dev(), details=True)
        HR.assert_hota_equal(first, gold, scene)
        HR.assert_kept_ids(first, gold, scene)
        again = HE.evaluate_hota_files(pred, gt, T, frames_per_launch=fpl, device=dev(), details=True)
        assert sorted(again) == sorted(first)
        for k in HR.FIELDS + HE.COUNT_FIELDS:
            assert np.array_equal(first[k], again[k]), (fpl, k)   # the same bits on every call


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


def test_evaluate_hota_sequence_equals_the_route_through_the_text_file(tmp_path):
    """HOTA straight from the pasted label images equals that of the rows save_results_to_file writes"""
    masks, boxes, frame, ped, label, keep, gt, (h, w), F = tracked_sequence()
    n = masks.shape[0]
    node_preds = torch.from_numpy(masks).to(dev()).view(n, 1, 28, 28)
    gt_txt = R.write_txt(str(tmp_path / "gt.txt"), R.id_image_rows(gt))
    keep_t = torch.from_numpy(keep).to(dev())
    rles = tracker.to_full_masks(node_preds, boxes, frame, keep_t, (h, w), 0.5, frames_per_launch=4)
    tracker.save_results_to_file(str(tmp_path / "pred.txt"), frame, ped, label, (h, w), rles, keep)
    want = HE.evaluate_hota_files(str(tmp_path / "pred.txt"), gt_txt, F + 1, frames_per_launch=3, device=dev(), details=True)
    assert want["HOTA_TP"][0] >= 8 and want["HOTA_FN"][0] >= 1 and want["HOTA_FP"][0] >= 1 and 0 < want["AssA"][0] < 1
    assert want["num_tracker_dets"] == 3 * (F - 1) - 1 and want["num_gt_ids"] == 3
    for fpl in (1, 4, 64):
        got = tracker.evaluate_hota_sequence(node_preds, boxes, frame, torch.from_numpy(ped).to(dev()), label, keep_t, (h, w), gt_txt, F + 1,
                                             mask_threshold=0.5, frames_per_launch=fpl, details=True)
        assert sorted(got) == sorted(want)
        for k in HR.FIELDS + HE.COUNT_FIELDS:
            assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
        assert got["kept_tracker_ids"] == want["kept_tracker_ids"]
    loaded = ME.load_mots_txt(gt_txt)
    assert tracker.evaluate_hota_sequence(node_preds, boxes, frame, ped, label, keep, (h, w), loaded, F + 1)["HOTA(0)"] == want["HOTA(0)"]
    with pytest.raises(ValueError, match="invalid timesteps: 6"):
        tracker.evaluate_hota_sequence(node_preds, boxes, frame, ped, label, keep, (h, w), loaded, F)
