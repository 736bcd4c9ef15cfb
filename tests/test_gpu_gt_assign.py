"""Ground-truth assignment and RoI mask targets on the device (``csrc/gt_assign.hip`` through ``mpntrackseg_amd.gt_assign``)
against the numpy restatement of tests/gt_assign_ref.py: identities and entries exactly, IoU cells to 1e-15, RoIAlign within the
float32 bound derived from each box's sample count and bit for bit against the restatement in the operator's order, whatever
the launch grouping; then the stored files through ``graph.assign_mask_labels``."""
import numpy as np
import pytest
import torch

import gt_assign_ref as R
from mpntrackseg_amd import gt_assign as GA, graph as G
from mpntrackseg_amd.capi import MpnhipError

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def unique_optimum(frames):
    """a tie in a scene is a bug of the scene: only a unique optimum is compared pair by pair"""
    for f, (dr, gr, iou, allowed, match) in frames.items():
        want, count, total, gap = R.brute_force(iou, allowed)
        assert gap > 1e-9, f
        assert np.array_equal(match, want), f


@pytest.fixture(scope="module")
def boxes():
    det, gt, named = R.box_scene()
    det_id, entry, frames = R.assign_scene(det, gt, 0.5)
    unique_optimum(frames)
    return det, gt, named, det_id, entry, frames


@pytest.fixture(scope="module")
def masks():
    det, gt, dense = R.mask_scene()
    want = {}
    for min_iou in (0.5, 0.2):
        want[min_iou] = R.assign_scene(det, gt, min_iou, dense)
        unique_optimum(want[min_iou][2])
    return det, gt, want


def compare_assignment(got, want, fpl):
    det_id, entry, launches = got
    want_id, want_entry, frames = want
    assert det_id.dtype == torch.int64 and entry.dtype == torch.int32 and det_id.is_cuda and entry.is_cuda
    assert np.array_equal(entry.cpu().numpy(), want_entry)
    assert np.array_equal(det_id.cpu().numpy(), want_id)
    seen = []
    for launch in launches:
        assert launch["frames"].size <= fpl
        iou, allowed, cp = launch["iou"].cpu().numpy(), launch["allowed"].cpu().numpy(), launch["cell_ptr"]
        for i, f in enumerate(launch["frames"]):
            dr, gr, want_iou, want_allowed, _ = frames[int(f)]
            assert np.array_equal(launch["det_row"][launch["a_ptr"][i]:launch["a_ptr"][i + 1]], dr)
            assert np.array_equal(launch["gt_row"][launch["b_ptr"][i]:launch["b_ptr"][i + 1]], gr)
            cells = slice(cp[i], cp[i + 1])
            assert np.abs(iou[cells].reshape(want_iou.shape) - want_iou).max(initial=0) <= 1e-15, f
            assert np.array_equal(allowed[cells].reshape(want_iou.shape).astype(bool), want_allowed), f
            seen.append(int(f))
    assert seen == sorted(frames)


@pytest.mark.parametrize("fpl", (1, 4))
def test_box_assignment_equals_the_restatement(boxes, fpl):
    det, gt, named, want_id, want_entry, frames = boxes
    got = GA.assign_gt(det, gt, 0.5, frames_per_launch=fpl, device=dev(), details=True)
    compare_assignment(got, (want_id, want_entry, frames), fpl)
    entry = got[1].cpu().numpy()
    (d0, d1), (g0, g1) = named["cardinality"]          # two pairs, not the best single one
    assert entry[d0] == g1 and entry[d1] == g0 and got[0].cpu().numpy()[d0] == gt["id"][g1]
    (d0, d1), (g0, g1) = named["greedy"]               # the best pair is not part of the best matching
    assert entry[d0] == g1 and entry[d1] == g0
    assert (entry[det["frame"] == 4] == -1).all() and (entry[det["frame"] == 5] == -1).all()
    assert not np.isin(np.flatnonzero(gt["frame"] == 3), entry).any()


@pytest.mark.parametrize("min_iou", (0.5, 0.2))
@pytest.mark.parametrize("fpl", (1, 4))
def test_mask_assignment_equals_the_restatement(masks, fpl, min_iou):
    det, gt, want = masks
    got = GA.assign_gt(det, gt, min_iou, mask_priority=True, frames_per_launch=fpl, device=dev(), details=True)
    compare_assignment(got, want[min_iou], fpl)
    entry = got[1].cpu().numpy()
    d0, d1 = np.flatnonzero(det["frame"] == 6)
    g0, g1 = np.flatnonzero(gt["frame"] == 6)
    if min_iou == 0.2:
        assert entry[d0] == g1 and entry[d1] == g0     # the cardinality case among disjoint masks
    else:
        assert entry[d0] == g0 and entry[d1] == -1


def test_launch_grouping_does_not_change_the_assignment(boxes, masks):
    for det, gt, kw in ((boxes[0], boxes[1], {}), (masks[0], masks[1], {"mask_priority": True, "min_iou": 0.2})):
        a = GA.assign_gt(det, gt, frames_per_launch=1, device=dev(), details=True, **kw)
        b = GA.assign_gt(det, gt, frames_per_launch=4, device=dev(), details=True, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for key in ("iou", "allowed"):
            assert torch.equal(torch.cat([l[key] for l in a[2]]), torch.cat([l[key] for l in b[2]])), key


def test_a_frame_the_solver_does_not_take_is_reported(boxes):
    det, gt = {k: v.copy() for k, v in boxes[0].items()}, boxes[1]
    det["bb_top"][np.flatnonzero(det["frame"] == 2)[0]] = np.nan
    with pytest.raises(MpnhipError, match="assign_gt.*problem 1 of 5.*not finite"):
        GA.assign_gt(det, gt, device=dev())


def test_empty_files_give_empty_or_unmatched_results(boxes):
    det, gt = boxes[0], boxes[1]
    none = {k: v[:0] for k, v in det.items()}
    det_id, entry = GA.assign_gt(none, gt, device=dev())
    assert det_id.numel() == 0 and entry.numel() == 0 and det_id.is_cuda
    det_id, entry = GA.assign_gt(det, {k: v[:0] for k, v in gt.items()}, device=dev())
    assert (det_id == -1).all() and (entry == -1).all() and entry.numel() == det["frame"].size


@pytest.fixture(scope="module")
def roi(masks):
    gt = masks[1]
    det, entry, what = R.roi_scene()
    want64 = R.gt_roi_masks(det, gt, entry)
    want32 = R.gt_roi_masks(det, gt, entry, acc=np.float32)
    got = {fpl: GA.gt_roi_masks(det, gt, torch.from_numpy(entry).to(dev()), frames_per_launch=fpl) for fpl in (1, 4)}
    return det, gt, entry, what, want64, want32, got


def test_roi_align_stays_within_the_float32_bound_of_each_box(roi):
    det, gt, entry, what, (want, want_valid, grids), _, got = roi
    m, valid = got[4]
    assert m.dtype == torch.float32 and tuple(m.shape) == (len(what), 1, 56, 56) and valid.dtype == torch.uint8 and m.is_cuda and valid.is_cuda
    m, valid = m.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(valid, want_valid)
    assert [w for w, v in zip(what, want_valid) if not v] == ["ignored id", "unmatched", "frame without ground truth", "entry of another frame"]
    assert [tuple(g) for g in grids[[0, 3, 6]]] == [(1, 1), (2, 3), (1, 1)]
    for k, name in enumerate(what):
        tol = (4 * grids[k, 0] * grids[k, 1] + 2) * 2.0 ** -24
        err = np.abs(m[k].astype(np.float64) - want[k]).max()
        print("%-28s grid %d x %d  max |device - float64| = %.3e  (bound %.3e)" % (name, grids[k, 0], grids[k, 1], err, tol))
        assert err <= tol, name
        if want_valid[k]:
            assert ((want[k] > 0.01) & (want[k] < 0.99)).any() and (want[k] == 0).any(), name
        else:
            assert not m[k].any(), name


def test_roi_align_has_the_bits_of_the_float32_restatement(roi):
    _, _, _, what, _, (want32, want_valid, _), got = roi
    m = got[4][0].cpu().numpy()
    for k, name in enumerate(what):
        assert np.array_equal(m[k], want32[k]), name


def test_launch_grouping_does_not_change_the_roi_masks(roi):
    got = roi[-1]
    assert torch.equal(got[1][0], got[4][0]) and torch.equal(got[1][1], got[4][1])


def test_stored_masks_come_back_through_assign_mask_labels(roi, tmp_path):
    det, got = roi[0], roi[-1]
    m, valid = got[4]
    GA.store_gt_masks(str(tmp_path), det, m, valid)
    stored = torch.load(str(tmp_path / "processed_data" / "gt" / "gt_mask" / "masks" / "2.pt"))
    assert tuple(stored.shape) == (4, 2, 56, 56) and stored[:, 0, 0, 0].tolist() == [4.0, 5.0, 6.0, 7.0]
    assert tuple(torch.load(str(tmp_path / "processed_data" / "gt" / "gt_mask" / "valid_ixs" / "2.pt")).shape) == (4, 2)
    back, ixs = G.assign_mask_labels(det, {"seq_path": str(tmp_path)})
    assert back.is_cuda and torch.equal(back, m) and ixs.dtype == torch.bool and torch.equal(ixs, valid.bool())


def test_boxes_the_operator_does_not_take_are_refused_on_the_host(roi):
    det, gt, entry = roi[0], roi[1], torch.from_numpy(roi[2]).to(dev())
    for column, value, text in (("bb_left", np.nan, "not finite"), ("bb_right", 131.0 + 56 * 300, "more than 256 samples")):
        bad = {k: v.copy() for k, v in det.items()}
        bad[column][3] = value
        with pytest.raises(ValueError, match=text):
            GA.gt_roi_masks(bad, gt, entry)
