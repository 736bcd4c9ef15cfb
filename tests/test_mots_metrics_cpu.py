"""The MOTS metrics without a device: the host side of ``mpntrackseg_amd.mots_eval`` over the numpy restatements of the three
operators (``tests/mots_metrics_ref.py``) reproduces what the evaluation kit's own ``MOTSMetrics`` computed for the two scenes of
``tests/golden/g22_mots_metrics.npz`` (``tools/make_golden.py --only g22``); the text loader round-trips the scenes and refuses
what the kit's ``load_txt`` refuses; the sizing entry and the argument checks of the C entry points run on the host.

Integers and decisions are compared for equality; the float metrics within 1e-12 relative -- they are a handful of double
operations on equal integers, and ``total_cost`` is summed in the kit's order."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mots_metrics_ref as R
from mpntrackseg_amd import capi, mots_eval as ME

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPNHIP_ERR_ARG, MPNHIP_ERR_WORKSPACE, MPNHIP_ERR_UNSUPPORTED = -1, -3, -4   # include/mpnhip.h


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(R.GOLDEN))


@pytest.mark.parametrize("scene", R.SCENES)
@pytest.mark.parametrize("frames_per_launch", (1, 5, 64))
def test_restated_operators_and_host_metrics_reproduce_g22(gold, scene, frames_per_launch, tmp_path):
    pred, gt, seq_length = R.scene_files(gold, scene, tmp_path)
    m = ME.evaluate_mots_files(pred, gt, seq_length, frames_per_launch=frames_per_launch, device=None, details=True, _ops=R)
    R.assert_metrics_equal(m, gold, scene)


def test_one_side_empty(gold, tmp_path):
    """no prediction: every ground-truth object is a miss; no ground truth: every prediction a false positive"""
    pred, gt, seq_length = R.scene_files(gold, "cases", tmp_path)
    empty = R.write_txt(str(tmp_path / "empty.txt"), [])
    n_gt, n_tr = int(gold["cases:m:n_gt"]), int(gold["cases:m:n_tr"])
    m = ME.evaluate_mots_files(empty, gt, seq_length, device=None, _ops=R)
    assert (m["fn"], m["tp"], m["fp"], m["n_gt"], m["n_tr"], m["sMOTSA"], m["IDF1"], m["ML"]) == (n_gt, 0, 0, n_gt, 0, 0.0, 0.0, 6)
    m = ME.evaluate_mots_files(pred, empty, seq_length, device=None, _ops=R)
    assert (m["fp"], m["tp"], m["fn"], m["n_tr"], m["sMOTSA"], m["IDF1"]) == (n_tr, 0, 0, n_tr, -float("inf"), 0.0)


def test_fixture_holds_the_cases_it_promises(gold):
    """the "cases" scene: an id switch, a fragment, misses, false positives, an ignored prediction, one MT / PT / ML trajectory
    each, a pair at IoU exactly 0.5 (no CLEAR match, an IDF1 match), frames without ground truth / predictions / ignore region;
    the "crowded" scene: tables beyond the LDS bound of the overlap kernel"""
    g = lambda k: float(gold["cases:m:" + k])
    assert min(g("id_switches"), g("fragments"), g("fn"), g("fp"), g("n_itr"), g("MT"), g("PT"), g("ML")) >= 1
    L = R.scene_lists(gold["cases:gt"], gold["cases:pred"])
    table, tp = R.label_overlap(L["labels_a"], L["labels_b"], L["a_ptr"], L["b_ptr"])
    o = R.frame_match(table, tp, L["a_ptr"], L["b_ptr"], L["a_ignore"], L["a_traj"], L["b_traj"], L["n_a_traj"], L["n_b_traj"])
    assert int(o["id_match"].sum()) == int(g("tp")) + 1
    na, nb = np.diff(L["a_ptr"]), np.diff(L["b_ptr"])
    assert (na == 0).any() and (nb == 0).any()
    has_ignore = np.add.reduceat(np.concatenate((L["a_ignore"], [0])), L["a_ptr"][:-1])[na > 0]
    assert (has_ignore == 0).any() and (has_ignore == 2).any()
    assert (gold["cases:gt"] // 1000 == 1).any()
    C = R.scene_lists(gold["crowded:gt"], gold["crowded:pred"])
    assert (np.diff(R.table_offsets(C["a_ptr"], C["b_ptr"])) > R.LDS_CELLS).all()
    for scene in R.SCENES:   # no empty mask: every id of every frame has pixels by construction; every area is positive
        assert gold[scene + ":gt"].dtype == np.uint16 and gold[scene + ":pred"].dtype == np.uint16


@pytest.mark.parametrize("scene", R.SCENES)
def test_load_mots_txt_round_trips_the_scenes(gold, scene, tmp_path):
    for side in ("gt", "pred"):
        ids = gold["%s:%s" % (scene, side)]
        F, H, W = ids.shape
        rows = R.id_image_rows(ids)
        d = ME.load_mots_txt(R.write_txt(str(tmp_path / "rows.txt"), rows))
        assert d["frame"].size == len(rows) and (d["h"] == H).all() and (d["w"] == W).all()
        assert (d["class_id"] == d["track_id"] // 1000).all()
        back = np.zeros((F, W * H), np.int64)
        for r, b, e in zip(d["run_row"], d["run_begin"], d["run_end"]):
            assert (back[d["frame"][r], b:e] == 0).all()
            back[d["frame"][r], b:e] = d["track_id"][r]
        np.testing.assert_array_equal(back.reshape(F, W, H).transpose(0, 2, 1), ids)
        np.testing.assert_array_equal(d["area"], [(ids[f] == t).sum() for f, t in zip(d["frame"], d["track_id"])])


def test_load_mots_txt_refuses_what_the_kit_refuses(gold, tmp_path):
    rows = R.id_image_rows(gold["cases:gt"])
    first = rows[0].split(" ")
    path = str(tmp_path / "bad.txt")
    with pytest.raises(ValueError, match="Multiple objects with track id"):
        ME.load_mots_txt(R.write_txt(path, rows + [rows[0]]))
    with pytest.raises(ValueError, match="Unknown object class"):
        ME.load_mots_txt(R.write_txt(path, rows + [" ".join([first[0], "3999", "3"] + first[3:])]))
    with pytest.raises(ValueError, match="overlapping masks"):   # the first object once more, under another id
        ME.load_mots_txt(R.write_txt(path, rows + [" ".join([first[0], "2999"] + first[2:])]))
    with pytest.raises(ValueError, match="Error in bad.txt"):
        ME.load_mots_txt(R.write_txt(path, ["x 1 2 3"]))
    # masks that only touch are fine
    ids = np.zeros((1, 5, 4), np.uint16)
    ids[0, :, :2], ids[0, :, 2:] = 2001, 2002
    assert ME.load_mots_txt(R.write_txt(path, R.id_image_rows(ids)))["area"].tolist() == [10, 10]


def test_metrics_of_an_empty_sequence():
    """nothing on either side: the kit's values for n_gt = 0 (MODSP 1 per frame, -inf accuracies, no trajectory)"""
    z = np.zeros(0, np.int64)
    m = ME.metrics_from_matches(z, z, z, z, z, z, z, z, z, z, np.zeros((0, 0), np.int64), 4)
    assert m["total_num_frames"] == 5 and m["MODSP"] == 100.0 and m["sMOTSA"] == -float("inf") and m["MOTSP"] == float("inf")
    assert m["IDF1"] == 0.0 and m["recall"] == 0.0 and m["FAR"] == 0.0 and m["n_gt_trajectories"] == 0
    with pytest.raises(ValueError):
        ME.metrics_from_matches(np.array([7]), np.array([0]), [0], [-1], [0], [0], z, z, z, z, np.zeros((1, 0), np.int64), 4)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.lib_path()):
        subprocess.check_call(["make", "-C", REPO, "-j4"], stdout=subprocess.DEVNULL)
    return capi.load()


def test_sizing_and_argument_checks_without_gpu(lib):
    """everything below returns before a HIP call (the non-null pointers are host dummies that are never dereferenced)"""
    size = lib.mpnhip_mots_workspace_bytes
    assert size(0, 0, 0, 0, 0) == 0 and size(0, 0, 50, 3, 1073) == 0          # nothing needed
    assert size(100000, 5, 5, 3, 1073) > size(1000, 5, 5, 3, 1073) >= 1001 * 20
    assert size(0, 1000, 5, 3, 1073) >= 4000
    for bad in ((-1, 5, 5, 3, 1073), (5, -1, 5, 3, 1073), (5, 5, -1, 3, 1073), (5, 5, 5, 65536, 1073), (5, 5, 5, 3, 1 << 31),
                (1 << 30, 5, 5, 3, 1073)):
        assert size(*bad) == 0, bad
    dummy = ctypes.create_string_buffer(512)
    p = ctypes.c_void_p((ctypes.addressof(dummy) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    big = size(10, 5, 5, 3, 1073)

    paint = lib.mpnhip_paint_label_runs
    assert paint(None, None, None, 0, None, 0, 0, 1073, None, None, 0, None) == 0                     # no frame: nothing to do
    assert paint(p, p, p, 10, p, 5, 3, 0, None, None, 0, None) == 0                                   # no pixel
    assert paint(p, p, p, -1, p, 5, 3, 1073, p, p, big, None) == MPNHIP_ERR_ARG
    assert b"paint_label_runs" in lib.mpnhip_last_error()
    assert paint(p, p, p, 10, p, 5, 65536, 1073, p, p, big, None) == MPNHIP_ERR_ARG
    assert paint(p, p, p, 10, p, 5, 3, 1073, None, p, big, None) == MPNHIP_ERR_ARG                    # null labels
    assert paint(p, p, p, 10, None, 5, 3, 1073, p, p, big, None) == MPNHIP_ERR_ARG                    # null frame_ptr
    assert paint(p, None, p, 10, p, 5, 3, 1073, p, p, big, None) == MPNHIP_ERR_ARG                    # null runs
    assert paint(p, p, p, 10, p, 5, 3, 1073, p, p, 16, None) == MPNHIP_ERR_WORKSPACE
    assert b"paint_label_runs: workspace 16 <" in lib.mpnhip_last_error()
    assert paint(p, p, p, 10, p, 5, 3, 1073, p, None, 0, None) == MPNHIP_ERR_WORKSPACE

    overlap = lib.mpnhip_label_overlap
    assert overlap(None, None, None, 0, None, 0, None, None, 0, 1073, None, 0, None) == 0             # no frame, no cell
    assert overlap(p, p, p, 5, p, 5, p, None, 3, 1073, p, 1 << 31, None) == MPNHIP_ERR_UNSUPPORTED
    assert b"label_overlap" in lib.mpnhip_last_error()
    assert overlap(p, p, p, 5, p, 5, p, None, 3, 1073, None, 40, None) == MPNHIP_ERR_ARG              # null table
    assert overlap(None, p, p, 5, p, 5, p, None, 3, 1073, p, 40, None) == MPNHIP_ERR_ARG
    assert overlap(p, p, p, 5, p, 5, None, None, 3, 1073, p, 40, None) == MPNHIP_ERR_ARG              # null table_ptr
    assert overlap(p, odd, p, 5, p, 5, p, None, 3, 1073, p, 40, None) == MPNHIP_ERR_ARG
    assert b"16-byte" in lib.mpnhip_last_error()
    assert overlap(p, p, p, 5, p, 5, p, None, 3, 1 << 31, p, 40, None) == MPNHIP_ERR_ARG

    match = lib.mpnhip_mots_frame_match

    def call(table=p, cells=40, tptr=p, aptr=p, n_a=5, bptr=p, n_b=5, frames=3, ign=p, at=p, bt=p, nat=4, nbt=4, mb=p, it=p, un=p, bm=p,
             bi=p, ba=p, idm=p, ws=p, wsb=big):
        return match(table, cells, tptr, aptr, n_a, bptr, n_b, frames, ign, at, bt, nat, nbt, mb, it, un, bm, bi, ba, idm, ws, wsb, None)
    assert call(n_a=0, n_b=0, nat=0, nbt=0, frames=0, table=None, tptr=None, aptr=None, bptr=None, idm=None, ws=None, wsb=0) == 0
    assert call(cells=1 << 31) == MPNHIP_ERR_UNSUPPORTED
    assert call(nat=1 << 16, nbt=1 << 15) == MPNHIP_ERR_UNSUPPORTED
    assert b"mots_frame_match" in lib.mpnhip_last_error()
    for bad in (dict(n_a=-1), dict(idm=None), dict(table=None), dict(tptr=None), dict(frames=0), dict(ign=None), dict(mb=None),
                dict(bt=None), dict(ba=None), dict(bm=None)):
        assert call(**bad) == MPNHIP_ERR_ARG, bad
    assert call(wsb=16) == MPNHIP_ERR_WORKSPACE
    assert call(ws=None, wsb=0) == MPNHIP_ERR_WORKSPACE
    names = capi.path_counters()
    assert "label_overlap_lds" in names and "label_overlap_global" in names
