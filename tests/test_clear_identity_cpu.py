"""The host side of the KITTI-MOTS table (``mpntrackseg_amd.kitti_mots_eval``) over the numpy restatements of the operators
(tests/clear_identity_ref.py, tests/hota_ref.py), against TrackEval's own results (g24: the kit's KittiMOTS preprocessing, then
CLEAR, Identity, Count and HOTA .eval_sequence and the three combine methods, on four scenes and two classes).  No device: what
runs here is the launch bookkeeping, Identity's reduced assignment, the kit's final fields and the combinations -- and the
restatements the GPU tests compare the kernels with.  Integer fields and counts are exact; float fields are within 1e-9 relative,
absolute where the value is 0 (sums of fewer than 10^6 terms in [0, 1] in another order)."""
import numpy as np
import pytest

import clear_identity_ref as CR
import hota_ref as HR
import mots_metrics_ref as R
from mpntrackseg_amd import hota_eval as HE, kitti_mots_eval as KE
from mpntrackseg_amd.capi import MpnhipError


@pytest.fixture(scope="module")
def golds():
    return CR.golds()


@pytest.fixture(scope="module")
def files(golds, tmp_path_factory):
    d = tmp_path_factory.mktemp("kitti_mots")
    return {scene: CR.scene_files(*golds, scene, d) for scene in CR.SCENES}


@pytest.fixture(scope="module")
def results(files):
    """every scene once, both classes, at the default frames_per_launch"""
    return {scene: KE.evaluate_sequence_files(*files[scene], _ops=CR) for scene in CR.SCENES}


@pytest.mark.parametrize("cls", CR.CLASSES)
@pytest.mark.parametrize("scene", CR.SCENES)
def test_evaluate_sequence_files_equals_trackeval(golds, results, scene, cls):
    res = results[scene][cls]
    assert sorted(res) == ["CLEAR", "Count", "HOTA", "Identity"]
    assert sorted(res["CLEAR"]) == sorted(KE.CLEAR_FIELDS) and sorted(res["Identity"]) == sorted(KE.IDENTITY_FIELDS)
    assert sorted(res["Count"]) == sorted(KE.COUNT_FIELDS)
    assert sorted(res["HOTA"]) == sorted(HR.FIELDS + HE.COUNT_FIELDS)
    CR.assert_metrics_equal(res, golds[0], "%s:%s" % (scene, cls))


def test_the_clear_scene_holds_its_cases(results):
    ped, car = results["clear"]["pedestrian"], results["clear"]["car"]
    assert [ped["CLEAR"][k] for k in ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag")] == [20, 6, 3, 1, 3, 2, 0, 1]
    assert [car["CLEAR"][k] for k in ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "Frag")] == [8, 2, 1, 1, 0] and car["Count"]["Dets"] == 9


@pytest.mark.parametrize("scene", CR.SCENES)
def test_the_hota_part_is_evaluate_hota_files(files, results, scene):
    for cls in CR.CLASSES:
        want = HE.evaluate_hota_files(*files[scene], class_id=KE.CLASS_IDS[cls], _ops=CR)
        CR.assert_same_bits(results[scene][cls]["HOTA"], want, scene + ":" + cls)


def test_requested_metrics_and_classes_only(files):
    res = KE.evaluate_sequence_files(*files["clear"], classes=("pedestrian",), metrics=("Identity",), _ops=CR)
    assert list(res) == ["pedestrian"] and sorted(res["pedestrian"]) == ["Count", "Identity"]
    with pytest.raises(ValueError, match="metric"):
        KE.evaluate_sequence_files(*files["clear"], metrics=("JAndF",), _ops=CR)
    with pytest.raises(ValueError, match="class"):
        KE.evaluate_sequence_files(*files["clear"], classes=("cyclist",), _ops=CR)
    with pytest.raises(ValueError, match="assignment"):
        KE.evaluate_sequence_files(*files["clear"], assignment="scipy", _ops=CR)


def test_combinations_equal_trackeval(golds, results):
    gold = golds[0]
    per_class = {}
    for cls in CR.CLASSES:
        per_class[cls] = KE.combine_sequences({scene: results[scene][cls] for scene in CR.SCENES})
        CR.assert_metrics_equal(per_class[cls], gold, "COMBINED_SEQ:" + cls)
    CR.assert_metrics_equal(KE.combine_classes_class_averaged(per_class), gold, "COMBINED_SEQ:cls_comb_cls_av")
    CR.assert_metrics_equal(KE.combine_classes_det_averaged(per_class), gold, "COMBINED_SEQ:cls_comb_det_av")
    assert "Frames" not in per_class["car"]["Count"]   # count.py:25-30


def test_eval_kitti_mots_nesting(golds, files, results):
    res = KE.eval_kitti_mots({scene: files[scene] for scene in ("clear", "cases")}, _ops=CR)
    assert sorted(res) == ["COMBINED_SEQ", "cases", "clear"]
    assert sorted(res["COMBINED_SEQ"]) == ["car", "cls_comb_cls_av", "cls_comb_det_av", "pedestrian"]
    for scene in ("clear", "cases"):
        CR.assert_same_bits(res[scene], results[scene], scene)
    for row in res["COMBINED_SEQ"].values():
        assert sorted(row) == ["CLEAR", "Count", "HOTA", "Identity"]
    want = KE.combine_sequences([results["cases"]["pedestrian"], results["clear"]["pedestrian"]])
    CR.assert_same_bits(res["COMBINED_SEQ"]["pedestrian"], want, "COMBINED_SEQ")
    det = res["COMBINED_SEQ"]["cls_comb_det_av"]
    assert det["CLEAR"]["CLR_TP"] == sum(results[s][c]["CLEAR"]["CLR_TP"] for s in ("clear", "cases") for c in CR.CLASSES)
    assert det["Count"]["GT_Dets"] == 33 + 1 + 26 + 10
    with pytest.raises(ValueError, match="COMBINED_SEQ"):
        KE.eval_kitti_mots({"COMBINED_SEQ": files["clear"]}, _ops=CR)


@pytest.mark.parametrize("scene", ("cases", "association", "clear"))
def test_result_does_not_depend_on_frames_per_launch(files, results, scene):
    for fpl in (1, 5, 64):
        res = KE.evaluate_sequence_files(*files[scene], frames_per_launch=fpl, _ops=CR)
        CR.assert_same_bits(res, results[scene], "%s:%d" % (scene, fpl))   # every sum runs in frame order: the same bits


def test_reduced_identity_problem_equals_the_kits_formulation():
    """identity.py:63-85 solves a (G + T) x (G + T) problem with 1e10 walls; the operators solve "maximise the sum of
    potential_count over a complete assignment of min(G, T) pairs".  Random count tables with many ties (small counts, many
    zeros, repeated rows), every shape: the three numbers agree."""
    rng = np.random.default_rng(24)
    for G, T in ((1, 1), (1, 7), (6, 1), (5, 5), (9, 4), (4, 11), (23, 17), (12, 30)):
        for density in (0.15, 0.5, 1.0):
            table = (rng.integers(0, 4, (G, T)) * (rng.random((G, T)) < density)).astype(np.int32)
            if G > 2:
                table[1] = table[0]   # two ids with the same row
            gt_count = table.sum(axis=1) + rng.integers(0, 3, G)        # a detection is a potential match of at most ... any count
            tr_count = table.sum(axis=0) + rng.integers(0, 3, T)        # at least the row / column sum keeps the kit's costs >= 0
            acc = CR.identity_accumulators(G, T)
            acc["potential_count"][:] = table.reshape(-1)
            match_b = KE.identity_assign_host(CR.identity_table(acc))
            assert (match_b >= 0).sum() == min(G, T) and np.unique(match_b[match_b >= 0]).size == min(G, T)
            idtp = CR.identity_sums(acc, match_b)
            want = CR.identity_kit(table, gt_count, tr_count)
            assert (idtp, int(gt_count.sum()) - idtp, int(tr_count.sum()) - idtp) == want, (G, T, density)


def rect_rows(frames, H=12, W=16):
    """MOTS rows of frames given as {id: (y0, y1, x0, x1)}"""
    ids = np.zeros((len(frames), H, W), np.uint16)
    for f, objs in enumerate(frames):
        for obj, (y0, y1, x0, x1) in objs.items():
            ids[f, y0:y1, x0:x1] = obj
    return R.id_image_rows(ids)


def test_empty_sides_return_early(tmp_path):
    """clear.py:45-53 and identity.py:40-45"""
    gt = R.write_txt(str(tmp_path / "gt.txt"), rect_rows([{2001: (1, 5, 1, 5)}, {2001: (1, 5, 2, 6), 2002: (6, 10, 2, 6)}]))
    pred = R.write_txt(str(tmp_path / "pred.txt"), rect_rows([{2007: (1, 5, 1, 5)}, {}]))
    empty = R.write_txt(str(tmp_path / "empty.txt"), [])
    zero = lambda res, but: all(res[k] == 0 for k in res if k not in but)
    for p in (empty, R.write_txt(str(tmp_path / "cars.txt"), rect_rows([{1001: (1, 5, 1, 5)}, {}]))):   # no scored prediction
        res = KE.evaluate_sequence_files(p, gt, 2, classes=("pedestrian",), _ops=CR)["pedestrian"]
        c, i = res["CLEAR"], res["Identity"]
        assert (c["CLR_FN"], c["ML"], c["MLR"]) == (3, 2, 1.0) and zero(c, ("CLR_FN", "ML", "MLR")) and sorted(c) == sorted(KE.CLEAR_FIELDS)
        assert i["IDFN"] == 3 and zero(i, ("IDFN",)) and sorted(i) == sorted(KE.IDENTITY_FIELDS)
        assert res["Count"] == {"Dets": 0, "GT_Dets": 3, "IDs": 0, "GT_IDs": 2, "Frames": 2}
        assert res["HOTA"]["HOTA_FN"].tolist() == [3.0] * 19
    res = KE.evaluate_sequence_files(pred, empty, 2, classes=("pedestrian",), _ops=CR)["pedestrian"]   # no ground-truth object
    c, i = res["CLEAR"], res["Identity"]
    assert (c["CLR_FP"], c["MLR"]) == (1, 1.0) and zero(c, ("CLR_FP", "MLR")) and i["IDFP"] == 1 and zero(i, ("IDFP",))
    assert res["Count"] == {"Dets": 1, "GT_Dets": 0, "IDs": 1, "GT_IDs": 0, "Frames": 2}
    # neither side: the first of the kit's two returns
    res = KE.evaluate_sequence_files(empty, empty, 2, _ops=CR)
    for cls in CR.CLASSES:
        assert res[cls]["CLEAR"]["MLR"] == 1.0 and zero(res[cls]["CLEAR"], ("MLR",)) and zero(res[cls]["Identity"], ())
    # the combinations take such results like any other
    comb = KE.combine_classes_class_averaged(res)
    assert comb["CLEAR"]["MLR"] == 1.0 and comb["CLEAR"]["CLR_FN"] == 0 and comb["Identity"]["IDF1"] == 0


def star_launch(first_frame_pred=None):
    """Two frames of 8 x 8.  Frame 1: the object (trajectory 0, 16 pixels) is split exactly in half by the predictions of
    trajectories 1 (the list's first) and 2.  Frame 0: the object under the prediction of ``first_frame_pred``, or no frame-0
    prediction at all -- then nothing carries continuity into the star."""
    lab_a, lab_b = np.full((2, 8, 8), -1, np.int32), np.full((2, 8, 8), -1, np.int32)
    lab_a[0, 0:4, 0:4], lab_a[1, 0:4, 0:4] = 0, 1
    n0 = 0 if first_frame_pred is None else 1
    if n0:
        lab_b[0, 0:4, 0:4] = 0
    lab_b[1, 0:2, 0:4], lab_b[1, 2:4, 0:4] = n0, n0 + 1
    a_ptr, b_ptr = [0, 1, 2], [0, n0, n0 + 2]
    b_traj = ([first_frame_pred] if n0 else []) + [1, 2]
    table, tp = CR.label_overlap(lab_a.reshape(2, -1), lab_b.reshape(2, -1), a_ptr, b_ptr)
    S = CR.frame_similarity(table, tp, a_ptr, b_ptr, [0, 0], [1] * len(b_traj))
    return S, np.array([0, 0], np.int32), np.asarray(b_traj, np.int32)


def scan(S, at, bt, G, T):
    state = CR.clear_accumulators(G)
    cand = CR.clear_frame_candidates(S, at, bt, G, T)
    match_b = CR.clear_sequence_scan(S, at, bt, cand, T, state)
    return cand, match_b, state


def test_star_without_continuity_is_resolved_by_list_order():
    """The one deliberate difference from the kit (which follows scipy's tie order): without an arm that continues the previous
    frame's match the earlier entry wins; with one, that arm wins wherever it stands.  No frame of the fixture holds the former."""
    S, at, bt = star_launch(None)
    cand, match_b, state = scan(S, at, bt, 1, 3)
    assert S["sim"].tolist() == [0.5, 0.5] and cand["a_cand"].tolist() == [-1, -1, 0, 1] and cand["status"].tolist() == [0]
    assert match_b.tolist() == [-1, 0] and state["counters"].tolist() == [1, 1, 1, 0] and state["prev_tracker_id"].tolist() == [1]
    for first, winner in ((1, 1), (2, 2), (0, 1)):   # continuity on the earlier arm, on the later arm, on neither
        S, at, bt = star_launch(first)
        cand, match_b, state = scan(S, at, bt, 1, 3)
        assert match_b.tolist() == [0, winner] and state["prev_tracker_id"].tolist() == [winner]
        assert state["counters"].tolist() == [2, 0, 1, 0 if first == winner else 1] and state["motp_sum"].tolist() == [1.5]
        assert state["gt_frag_count"].tolist() == [1]
    # a column star: one prediction is exactly the union of two equal objects (trajectories 0 and 1)
    lab_a, lab_b = np.full((1, 8, 8), -1, np.int32), np.full((1, 8, 8), -1, np.int32)
    lab_a[0, 0:2, 0:4], lab_a[0, 2:4, 0:4], lab_b[0, 0:4, 0:4] = 0, 1, 0
    table, tp = CR.label_overlap(lab_a.reshape(1, -1), lab_b.reshape(1, -1), [0, 2], [0, 1])
    S = CR.frame_similarity(table, tp, [0, 2], [0, 1], [0, 0], [1])
    for prev, want in (([-1, -1], [0, -1]), ([0, -1], [0, -1]), ([-1, 0], [-1, 0]), ([5, 7], [0, -1])):
        state = CR.clear_accumulators(2)
        state["prev_timestep_tracker_id"][:] = prev
        cand = CR.clear_frame_candidates(S, [0, 1], [0], 2, 1)
        assert cand["b_cand"].tolist() == [0, 1] and cand["a_cand"].tolist() == [0, -1, 0, -1] and cand["status"].tolist() == [0]
        assert CR.clear_sequence_scan(S, [0, 1], [0], cand, 1, state).tolist() == want
        assert state["counters"].tolist() == [1, 1, 0, 0] and state["motp_sum"].tolist() == [0.5]


def test_three_candidates_raise():
    """Masks that overlap on one side cannot come from label images; a hand-made similarity block with three eligible cells in
    a row (and one with two stars sharing an arm) sets the status word and the summary raises"""
    def launch(sim, na, nb):
        sim = np.asarray(sim, np.float64).reshape(-1)
        return {"F": 1, "n_a": na, "n_b": nb, "a_ptr": np.array([0, na]), "b_ptr": np.array([0, nb]), "sim_ptr": np.array([0, na * nb]),
                "sim_cells": na * nb, "sim": sim, "b_removed": np.zeros(nb, np.uint8)}
    for sim, na, nb, status in (([0.5, 0.6, 0.7], 1, 3, 1), ([0.5, 0.5, 0.5], 3, 1, 1), ([0.5, 0.5, 0.0, 0.5], 2, 2, 2),
                                ([0.5, 0.5, 0.0, 0.4], 2, 2, 0)):
        S = launch(sim, na, nb)
        at, bt = np.arange(na, dtype=np.int32), np.arange(nb, dtype=np.int32)
        cand = CR.clear_frame_candidates(S, at, bt, na, nb)
        assert cand["status"].tolist() == [status]
        state = CR.clear_accumulators(na)
        CR.clear_sequence_scan(S, at, bt, cand, nb, state)
        if status:
            with pytest.raises(MpnhipError, match="status %d" % status):
                CR.clear_track_summary(state)
        else:
            assert CR.clear_track_summary(state)["CLR_TP"] == 1
    # a removed prediction and an entry of another class are no candidates
    S = launch([0.5, 0.6, 0.7], 1, 3)
    S["b_removed"][1] = 1
    assert CR.clear_frame_candidates(S, [0], [0, 1, -1], 1, 2)["a_cand"].tolist() == [0, -1]


def test_track_summary_boundaries():
    """clear.py:117-121: matched / count > 0.8 and >= 0.2 at the exact boundaries, an id that was never present, Frag"""
    state = CR.clear_accumulators(7)
    state["gt_id_count"][:] = [5, 5, 5, 10, 0, 5, 5]
    state["gt_matched_count"][:] = [5, 4, 1, 1, 0, 0, 3]
    state["gt_frag_count"][:] = [1, 3, 1, 1, 0, 0, 2]
    res = CR.clear_track_summary(state)
    assert (res["MT"], res["PT"], res["ML"], res["Frag"]) == (1, 3, 3, 3)


def test_final_fields_are_the_kits_arithmetic():
    res = KE.clear_from_sums({"CLR_TP": 20, "CLR_FN": 6, "CLR_FP": 3, "IDSW": 10, "MT": 3, "PT": 2, "ML": 0, "Frag": 1, "MOTP_sum": 17.5}, 26, 23,
                             5, 12)
    assert res["MOTA"] == (20 - 3 - 10) / 26 and res["MOTAL"] == (20 - 3 - 1.0) / 26 and res["sMOTA"] == (17.5 - 3 - 10) / 26
    assert res["MOTP"] == 17.5 / 20 and res["FP_per_frame"] == 3 / 12 and res["CLR_F1"] == 20 / (20 + 3 + 1.5) and res["MTR"] == 0.6
    res = KE.identity_from_sums(19, 26, 23)
    assert (res["IDTP"], res["IDFN"], res["IDFP"]) == (19, 7, 4) and res["IDF1"] == 19 / (19 + 2 + 3.5) and res["IDR"] == 19 / 26


def test_entry_point_argument_checks_without_gpu():
    """Size queries and the argument checks of the new entry points run on the host, before any device work (the non-null
    pointers are host dummies that are never dereferenced): null pointers are refused, empty inputs are successful no-ops that
    touch no device memory beyond their zeroed outputs, G * T >= 2^31 is MPNHIP_ERR_UNSUPPORTED and an undersized workspace
    MPNHIP_ERR_WORKSPACE."""
    import ctypes
    from mpntrackseg_amd import capi
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    small, big = l.mpnhip_clear_identity_workspace_bytes(10, 10, 2, 5, 5), l.mpnhip_clear_identity_workspace_bytes(10, 10, 2, 5000, 5)
    assert 0 < small < big
    assert l.mpnhip_clear_identity_workspace_bytes(10, 10, 2, 1 << 16, 1 << 15) == 0 and l.mpnhip_clear_identity_workspace_bytes(-1, 10, 2, 5, 5) == 0
    G, T = 1 << 16, 1 << 15
    assert l.mpnhip_identity_accumulate(p, 4, p, p, 2, p, 2, 1, p, p, p, G, T, p, None) == -4
    assert b"not supported" in l.mpnhip_last_error()
    assert l.mpnhip_identity_sums(p, p, G, T, p, None) == -4
    # nothing to do
    assert l.mpnhip_identity_accumulate(None, 0, None, None, 0, None, 0, 0, None, None, None, 3, 4, None, None) == 0
    assert l.mpnhip_identity_accumulate(p, 4, p, p, 2, p, 2, 1, p, p, p, 0, 4, None, None) == 0
    assert l.mpnhip_clear_sequence_scan(None, 0, None, None, 0, None, 0, 0, None, None, None, None, None, 3, 4, None, None, None, None, None, p, p,
                                        None, None, 0, None) == 0
    # null pointers and negative sizes
    assert l.mpnhip_identity_accumulate(p, 4, p, p, 2, p, 2, 1, p, p, p, 3, 4, None, None) == -1
    assert b"identity_accumulate" in l.mpnhip_last_error()
    assert l.mpnhip_identity_accumulate(None, 4, p, p, 2, p, 2, 1, p, p, p, 3, 4, p, None) == -1
    assert l.mpnhip_identity_accumulate(p, -4, p, p, 2, p, 2, 1, p, p, p, 3, 4, p, None) == -1
    assert l.mpnhip_identity_sums(p, p, 3, 4, None, None) == -1
    assert l.mpnhip_identity_sums(None, p, 3, 4, p, None) == -1
    assert l.mpnhip_identity_sums(p, p, -3, 4, p, None) == -1
    assert l.mpnhip_clear_frame_candidates(p, 4, p, p, 2, p, 2, 1, p, p, p, 3, 4, p, p, None, None) == -1
    assert b"clear_frame_candidates" in l.mpnhip_last_error()
    assert l.mpnhip_clear_frame_candidates(p, 4, p, p, 2, p, 2, 1, p, p, p, 3, 4, None, p, p, None) == -1
    assert l.mpnhip_clear_frame_candidates(p, 4, p, p, 2, p, 2, 0, p, p, p, 3, 4, p, p, p, None) == -1
    assert l.mpnhip_clear_sequence_scan(p, 4, p, p, 2, p, 2, 1, p, p, p, p, p, 3, 4, p, p, p, p, p, None, p, p, p, 1 << 20, None) == -1
    assert l.mpnhip_clear_sequence_scan(p, 4, p, p, 2, p, 2, 1, p, p, p, None, p, 3, 4, p, p, p, p, p, p, p, p, p, 1 << 20, None) == -1
    assert l.mpnhip_clear_sequence_scan(p, 4, p, p, 2, p, 2, 1, p, p, p, p, p, 3, 4, p, None, p, p, p, p, p, p, p, 1 << 20, None) == -1
    assert l.mpnhip_clear_track_summary(p, p, p, 3, None, None) == -1
    assert l.mpnhip_clear_track_summary(p, None, p, 3, p, None) == -1
    assert l.mpnhip_clear_track_summary(p, p, p, -1, p, None) == -1
    # an undersized workspace
    assert l.mpnhip_clear_sequence_scan(p, 4, p, p, 2, p, 2, 1, p, p, p, p, p, 300, 4, p, p, p, p, p, p, p, p, p, 16, None) == -3
    assert b"clear_sequence_scan: workspace" in l.mpnhip_last_error()
    assert l.mpnhip_clear_sequence_scan(p, 4, p, p, 2, p, 2, 1, p, p, p, p, p, 300, 4, p, p, p, p, p, p, p, p, None, 1 << 20, None) == -3
