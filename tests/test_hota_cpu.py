"""The host side of the HOTA evaluation (``mpntrackseg_amd.hota_eval``) over the numpy restatements of the operators
(tests/hota_ref.py), against TrackEval's own results (g23: the kit's KittiMOTS preprocessing and HOTA.eval_sequence /
combine_sequences on three scenes).  No device: what runs here is the launch bookkeeping, the assignments and the kit's final
fields -- and the restatements the GPU tests compare the kernels with.  Integer fields and counts are exact; float fields are
within 1e-9 (sums of fewer than 10^6 terms in [0, 1] in another order)."""
import numpy as np
import pytest

import hota_ref as HR
import mots_metrics_ref as R
from mpntrackseg_amd import hota_eval as HE


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(HR.GOLDEN))


@pytest.fixture(scope="module")
def gold22():
    return dict(np.load(R.GOLDEN))


@pytest.fixture(scope="module")
def results(gold, gold22, tmp_path_factory):
    """every scene once, at the default frames_per_launch"""
    d = tmp_path_factory.mktemp("hota")
    out = {}
    for scene in HR.SCENES:
        pred, gt, T = HR.scene_files(gold, gold22, scene, d)
        out[scene] = HE.evaluate_hota_files(pred, gt, T, details=True, _ops=HR)
    return out


@pytest.mark.parametrize("scene", HR.SCENES)
def test_evaluate_hota_files_equals_trackeval(gold, results, scene):
    res = results[scene]
    assert sorted(k for k in res if k != "kept_tracker_ids") == sorted(HR.FIELDS + HE.COUNT_FIELDS)
    HR.assert_hota_equal(res, gold, scene)
    HR.assert_kept_ids(res, gold, scene)


def test_combine_hota_equals_trackeval(gold, results):
    comb = HE.combine_hota([results[s] for s in HR.SCENES])
    HR.assert_hota_equal(comb, gold, "combined")
    assert comb["num_gt_dets"] == sum(int(gold[s + ":num_gt_dets"]) for s in HR.SCENES)


@pytest.mark.parametrize("scene", ("cases", "association"))
def test_result_does_not_depend_on_frames_per_launch(gold, gold22, results, scene, tmp_path):
    pred, gt, T = HR.scene_files(gold, gold22, scene, tmp_path)
    for fpl in (1, 5, 64):
        res = HE.evaluate_hota_files(pred, gt, T, frames_per_launch=fpl, details=True, _ops=HR)
        for k in HR.FIELDS + HE.COUNT_FIELDS:
            assert np.array_equal(res[k], results[scene][k]), (fpl, k)   # the sums run in frame order: the same bits
        assert res["kept_tracker_ids"] == results[scene]["kept_tracker_ids"]


def rect_rows(frames, H=12, W=16):
    """MOTS rows of frames given as {id: (y0, y1, x0, x1)}"""
    ids = np.zeros((len(frames), H, W), np.uint16)
    for f, objs in enumerate(frames):
        for obj, (y0, y1, x0, x1) in objs.items():
            ids[f, y0:y1, x0:x1] = obj
    return R.id_image_rows(ids)


def test_half_half_star_is_resolved_by_list_order(tmp_path):
    """A ground-truth mask split EXACTLY in half by two predictions is eligible (2 i = u) with both; the kit's assignment
    keeps one by scipy's tie order, the operator the earlier of the list.  Eligibility with both forces i = A / 2 = B for
    each, so both halves lie inside the object and away from the ignore region: neither can be removed, whichever is the
    matched one -- the rule is restated here because no frame of the fixture may hold the case."""
    a_ptr, b_ptr = [0, 2], [0, 3]
    lab_a, lab_b = np.full((1, 8, 8), -1, np.int32), np.full((1, 8, 8), -1, np.int32)
    lab_a[0, 0:4, 0:4] = 0          # the object: 16 pixels
    lab_a[0, 6:8, :] = 1            # the ignore region
    lab_b[0, 0:2, 0:4] = 1          # the object's upper half is the list's SECOND prediction,
    lab_b[0, 2:4, 0:4] = 0          # its lower half the first
    lab_b[0, 6:8, 0:3] = 2          # a third one inside the ignore region
    table, tp = HR.label_overlap(lab_a.reshape(1, -1), lab_b.reshape(1, -1), a_ptr, b_ptr)
    S = HR.frame_similarity(table, tp, a_ptr, b_ptr, [0, 1], [1, 1, 1])
    assert S["sim"].tolist() == [0.5, 0.5, 0.0, 0.0, 0.0, 0.0] and S["b_removed"].tolist() == [0, 0, 1]
    assert S["row_sum"].tolist() == [1.0, 0.0] and S["col_sum"].tolist() == [0.5, 0.5, 0.0]
    # the same frame through the evaluation: two detections kept, one of them a true positive up to alpha 0.5
    ids_gt, ids_pr = np.zeros((1, 8, 8), np.uint16), np.zeros((1, 8, 8), np.uint16)
    ids_gt[0, 0:4, 0:4], ids_gt[0, 6:8, :] = 2001, 10000
    ids_pr[0, 0:2, 0:4], ids_pr[0, 2:4, 0:4], ids_pr[0, 6:8, 0:3] = 2002, 2001, 2003
    res = HE.evaluate_hota_files(HR.loaded(ids_pr, tmp_path, "pred"), HR.loaded(ids_gt, tmp_path, "gt"), 1, details=True, _ops=HR)
    assert res["kept_tracker_ids"] == {0: [2001, 2002]} and res["num_tracker_dets"] == 2
    assert res["HOTA_TP"].tolist() == [1.0] * 10 + [0.0] * 9 and res["HOTA_FP"].tolist() == [1.0] * 10 + [2.0] * 9


def test_empty_sides_return_early(tmp_path):
    gt = R.write_txt(str(tmp_path / "gt.txt"), rect_rows([{2001: (1, 5, 1, 5)}, {2001: (1, 5, 2, 6), 2002: (6, 10, 2, 6)}]))
    pred = R.write_txt(str(tmp_path / "pred.txt"), rect_rows([{2007: (1, 5, 1, 5)}, {}]))
    empty = R.write_txt(str(tmp_path / "empty.txt"), [])
    cars = R.write_txt(str(tmp_path / "cars.txt"), rect_rows([{1001: (1, 5, 1, 5)}, {}]))
    for p in (empty, cars):   # no scored prediction: every ground-truth detection is a false negative
        res = HE.evaluate_hota_files(p, gt, 2, _ops=HR)
        assert res["HOTA_FN"].tolist() == [3.0] * 19 and res["HOTA_TP"].tolist() == [0.0] * 19 and res["HOTA_FP"].tolist() == [0.0] * 19
        assert res["LocA"].tolist() == [1.0] * 19 and res["LocA(0)"] == 1.0 and res["HOTA(0)"] == 0 and res["HOTA"].tolist() == [0.0] * 19
        assert (res["num_gt_dets"], res["num_tracker_dets"], res["num_gt_ids"], res["num_tracker_ids"]) == (3, 0, 2, 0)
    for g in (empty, cars):   # no ground-truth object: every prediction is a false positive
        res = HE.evaluate_hota_files(pred, g, 2, _ops=HR)
        assert res["HOTA_FP"].tolist() == [1.0] * 19 and res["HOTA_FN"].tolist() == [0.0] * 19 and res["LocA"].tolist() == [1.0] * 19
        assert (res["num_gt_dets"], res["num_tracker_dets"], res["num_gt_ids"], res["num_tracker_ids"]) == (0, 1, 0, 1)
    # a prediction that the preprocessing removes leaves the tracker side empty as well
    gt_ign = R.write_txt(str(tmp_path / "gt_ign.txt"), rect_rows([{2001: (1, 5, 1, 5), 10000: (6, 12, 0, 16)}]))
    pred_ign = R.write_txt(str(tmp_path / "pred_ign.txt"), rect_rows([{2003: (7, 11, 2, 6)}]))
    res = HE.evaluate_hota_files(pred_ign, gt_ign, 1, details=True, _ops=HR)
    assert res["num_tracker_dets"] == 0 and res["num_tracker_ids"] == 0 and res["HOTA_FN"].tolist() == [1.0] * 19
    assert res["kept_tracker_ids"] == {0: []}
    # the kit combines such results like any other
    comb = HE.combine_hota([res, res])
    assert comb["HOTA_FN"].tolist() == [2.0] * 19 and comb["HOTA"].tolist() == [0.0] * 19


def test_a_frame_outside_the_sequence_is_refused(tmp_path):
    frames = [{2001: (1, 5, 1, 5)}, {2001: (1, 5, 2, 6)}, {2001: (1, 5, 3, 7)}]
    three, two = R.write_txt(str(tmp_path / "three.txt"), rect_rows(frames)), R.write_txt(str(tmp_path / "two.txt"), rect_rows(frames[:2]))
    assert HE.evaluate_hota_files(three, three, 3, _ops=HR)["HOTA(0)"] == 1.0
    with pytest.raises(ValueError, match="Tracking data contains the following invalid timesteps: 2"):
        HE.evaluate_hota_files(three, two, 2, _ops=HR)
    with pytest.raises(ValueError, match="Ground-truth data contains the following invalid timesteps: 2"):
        HE.evaluate_hota_files(two, three, 2, _ops=HR)


def test_hota_from_accumulators_is_the_kits_arithmetic():
    """hota.py:103-117 and :166-179 on hand-made sums"""
    tp = np.arange(19, 0, -1)
    loca = tp * 0.75
    ass = np.stack((tp * 0.5, tp * 0.6, tp * 0.7), axis=1)
    res = HE.hota_from_accumulators(tp, loca, ass, 30, 25, 4, 5)
    HR.close(res["AssA"], np.full(19, 0.5)); HR.close(res["AssRe"], np.full(19, 0.6)); HR.close(res["AssPr"], np.full(19, 0.7))
    HR.close(res["LocA"], np.full(19, 0.75))
    assert np.array_equal(res["HOTA_FN"], 30 - tp) and np.array_equal(res["HOTA_FP"], 25 - tp)
    HR.close(res["DetA"], tp / (30 + 25 - tp)); HR.close(res["DetRe"], tp / 30); HR.close(res["DetPr"], tp / 25)
    HR.close(res["HOTA"], np.sqrt(res["DetA"] * 0.5)); HR.close(res["RHOTA"], np.sqrt(res["DetRe"] * 0.5))
    assert res["HOTA(0)"] == res["HOTA"][0] and res["HOTALocA(0)"] == res["HOTA"][0] * res["LocA"][0]
    # no match at an alpha: LocA is 1e-10 / 1e-10
    res = HE.hota_from_accumulators(np.zeros(19), np.zeros(19), np.zeros((19, 3)), 3, 2, 1, 1)
    assert res["LocA"].tolist() == [1.0] * 19 and res["HOTA"].tolist() == [0.0] * 19


def test_entry_point_argument_checks_without_gpu():
    """Size queries and the argument checks of the HOTA entry points run on the host: G * T * 19 >= 2^31 is refused with
    MPNHIP_ERR_UNSUPPORTED, empty launches are successful no-ops, null pointers are refused -- all before any device work (the
    non-null pointers are host dummies that are never dereferenced)."""
    import ctypes
    from mpntrackseg_amd import capi
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    small, big = l.mpnhip_hota_workspace_bytes(10, 10, 2, 5, 5), l.mpnhip_hota_workspace_bytes(1000, 1000, 64, 500, 500)
    assert 0 < small < big
    G, T = 20000, 6000   # 19 G T = 2.28e9
    assert l.mpnhip_hota_workspace_bytes(10, 10, 2, G, T) == 0 and l.mpnhip_hota_workspace_bytes(10, 10, 65535, 40000, 1) == 0
    assert l.mpnhip_hota_workspace_bytes(-1, 10, 2, 5, 5) == 0
    assert l.mpnhip_hota_accumulate_alignment(p, 4, p, p, 2, p, 2, 1, p, p, p, p, p, G, T, p, p, p, p, 256, None) == -4
    assert b"not supported" in l.mpnhip_last_error()
    assert l.mpnhip_hota_frame_scores(p, 4, p, p, 2, p, 2, 1, p, p, p, G, T, p, p, p, p, None) == -4
    assert l.mpnhip_hota_alpha_accumulate(p, 4, p, p, 2, p, 2, 1, p, p, p, p, p, G, T, p, p, p, p, 256, None) == -4
    assert l.mpnhip_hota_association(p, p, p, G, T, p, p, 256, None) == -4
    assert b"hota_association" in l.mpnhip_last_error()
    # nothing to do
    assert l.mpnhip_hota_frame_similarity(None, 0, None, None, 0, None, 0, 0, None, None, None, 0, None, None, None, None, None, 0, None) == 0
    assert l.mpnhip_hota_accumulate_alignment(None, 0, None, None, 0, None, 0, 0, None, None, None, None, None, 3, 4, None, None, None, None, 0, None) == 0
    assert l.mpnhip_hota_frame_scores(None, 0, None, None, 0, None, 0, 0, None, None, None, 3, 4, None, None, None, None, None) == 0
    # null pointers, negative sizes and an undersized workspace
    assert l.mpnhip_hota_frame_similarity(None, 12, p, p, 2, p, 2, 1, p, p, p, 4, p, p, p, p, p, 1 << 20, None) == -1
    assert b"hota_frame_similarity" in l.mpnhip_last_error()
    assert l.mpnhip_hota_frame_similarity(p, 12, p, p, 2, p, 2, 1, p, p, p, 4, p, p, p, p, p, 16, None) == -3
    assert l.mpnhip_hota_accumulate_alignment(p, 4, p, p, 2, p, 2, 1, None, p, p, p, p, 3, 4, p, p, p, p, 1 << 20, None) == -1
    assert l.mpnhip_hota_accumulate_alignment(p, 4, p, p, 2, p, 2, 1, p, p, p, p, p, 3, 4, p, p, p, p, 16, None) == -3
    assert l.mpnhip_hota_frame_scores(p, 4, p, p, 2, p, 2, 1, p, p, p, 3, 4, p, p, p, None, None) == -1
    assert l.mpnhip_hota_alpha_accumulate(p, 4, p, p, 2, p, 2, 1, p, p, p, p, None, 3, 4, p, p, p, p, 1 << 20, None) == -1
    assert l.mpnhip_hota_alpha_accumulate(p, 4, p, p, 2, p, 2, 1, p, p, p, p, p, 3, 4, p, p, p, p, 16, None) == -3
    assert l.mpnhip_hota_association(p, p, p, -1, 4, p, p, 256, None) == -1
    assert l.mpnhip_hota_association(p, p, p, 3, 4, None, p, 1 << 20, None) == -1
    assert l.mpnhip_hota_association(p, p, p, 3, 4, p, p, 16, None) == -3
