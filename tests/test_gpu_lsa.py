"""The batched linear sum assignment on the device (``csrc/assignment.hip`` through the C ABI and ``mpntrackseg_amd.assignment``)
against its numpy restatement (tests/lsa_ref.py), bit for bit -- ties included: both follow the tie rule of include/mpnhip.h --
and against scipy where the optimum is unique; then HOTA with ``assignment='device'`` against the fixture of TrackEval's own
results (g23) and against the host route."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

import full_masks_ref as FR
import hota_ref as HR
import lsa_ref as LR
import mots_metrics_ref as R
from mpntrackseg_amd import assignment, capi, hota_eval as HE, tracker
from mpntrackseg_amd.capi import MpnhipError, ptr

pytestmark = pytest.mark.gpu
GUARD = 64


def dev():
    return torch.device("cuda:0")


def up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev())


def guarded(n):
    """an int32 buffer of n entries (holding 55: the call itself must write the -1) between guard words"""
    big = torch.full((n + 2 * GUARD,), 77, dtype=torch.int32, device=dev())
    big[GUARD:GUARD + n] = 55
    return big, big[GUARD:GUARD + n]


def run_guarded(cost, cp, ap, bp, ka, kb, maximize):
    """mpnhip_lsa_batched on guarded outputs -> (match_b, match_a, status) as host arrays"""
    lib = capi.load()
    n_a, n_b, F = int(ap[-1]), int(bp[-1]), ap.size - 1
    t = [up(cost, np.float64), up(cp, np.int64), up(ap, np.int32), up(bp, np.int32)]
    keeps = [None if k is None else up(k, np.uint8) for k in (ka, kb)]
    bufs = [guarded(n) for n in (n_a, n_b, F)]
    ws = capi.workspace(lib.mpnhip_lsa_workspace_bytes(n_a, n_b, F), dev(), "lsa")
    with torch.cuda.device(dev()):
        capi.check(lib.mpnhip_lsa_batched(ptr(t[0]), t[0].numel(), ptr(t[1]), ptr(t[2]), n_a, ptr(t[3]), n_b, F, ptr(keeps[0]), ptr(keeps[1]),
                                          int(maximize), ptr(bufs[0][1]), ptr(bufs[1][1]), ptr(bufs[2][1]), ptr(ws), ws.numel(),
                                          capi.stream_ptr()), "mpnhip_lsa_batched")
    out = []
    for big, view in bufs:
        h = big.cpu().numpy()
        assert (h[:GUARD] == 77).all() and (h[GUARD + view.numel():] == 77).all()
        out.append(h[GUARD:GUARD + view.numel()].copy())
    return out


def the_batch():
    """one launch: an empty problem, empty sides, single rows and columns, sizes around the wavefront width on both sides (the
    transposed path among them), more than two columns per lane, a tie-heavy integer matrix, an all-zero matrix"""
    rng = np.random.default_rng(31)
    shapes = ((0, 0), (0, 5), (5, 0), (1, 1), (1, 7), (7, 1), (63, 64), (64, 65), (65, 63), (129, 70), (70, 129))
    problems = [rng.uniform(-1, 1, s) for s in shapes]
    problems.append(np.where(rng.random((110, 115)) < 0.8, 0.0, rng.integers(1, 10, (110, 115)).astype(np.float64)))
    problems.append(np.zeros((40, 50)))
    cost, cp, ap, bp = LR.batch(problems)
    ka, kb = rng.random(ap[-1]) >= 0.25, rng.random(bp[-1]) >= 0.25
    ka[ap[7]:ap[8]] = True                       # problem 7, 64 x 65: every row against about a third of the columns
    kb[bp[7]:bp[8]] = np.arange(65) % 3 == 0
    return problems, cost, cp, ap, bp, ka, kb


@pytest.fixture(scope="module")
def batch_and_references():
    problems, cost, cp, ap, bp, ka, kb = the_batch()
    want = {(masked, mx): LR.lsa_batched(cost, cp, ap, bp, ka if masked else None, kb if masked else None, mx)
            for masked in (False, True) for mx in (False, True)}
    return (problems, cost, cp, ap, bp, ka, kb), want


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("maximize", (False, True))
def test_operator_equals_the_restatement_bit_for_bit(batch_and_references, masked, maximize):
    (problems, cost, cp, ap, bp, ka, kb), refs = batch_and_references
    want = refs[(masked, maximize)]
    if masked:
        assert ka[ap[7]:ap[8]].sum() > kb[bp[7]:bp[8]].sum() and problems[7].shape[0] < problems[7].shape[1]
    assert (want[2] == 0).all() and (want[0] >= 0).sum() > 250
    got = run_guarded(cost, cp, ap, bp, ka if masked else None, kb if masked else None, maximize)
    for g, w, name in zip(got, want, ("match_b", "match_a", "status")):
        assert g.dtype == np.int32 and np.array_equal(g, w), name
    again = run_guarded(cost, cp, ap, bp, ka if masked else None, kb if masked else None, maximize)
    for g, a in zip(got, again):
        assert np.array_equal(g, a)
    if not masked:   # where the optimum is unique: scipy's pairs
        for f in range(3, 11):
            r, k = scipy_lsa(problems[f], maximize=maximize)
            assert np.array_equal(got[0][ap[f] + r], bp[f] + k), f


def test_one_larger_problem_equals_scipy():
    """300 x 320: the state is sized by the problem, not by a wavefront"""
    c = np.random.default_rng(32).uniform(-1, 1, (300, 320))
    for cost, maximize in ((c, False), (np.ascontiguousarray(c.T), True)):
        rows, cols = assignment.linear_sum_assignment(up(cost, np.float64), maximize)
        want = scipy_lsa(cost, maximize=maximize)
        assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1])


def test_a_nan_cell_stops_its_problem_alone():
    rng = np.random.default_rng(33)
    problems = [rng.uniform(-1, 1, s) for s in ((9, 11), (70, 66), (12, 12), (5, 8))]
    problems[2][7, 4] = np.nan
    cost, cp, ap, bp = LR.batch(problems)
    want = LR.lsa_batched(cost, cp, ap, bp)
    mb, ma, status = assignment.linear_sum_assignment_batched(up(cost, np.float64), cp, ap, bp)
    assert mb.dtype == ma.dtype == status.dtype == torch.int32 and mb.is_cuda and ma.is_cuda and status.is_cuda
    assert status.cpu().tolist() == [0, 0, 1, 0]
    assert (mb.cpu().numpy()[ap[2]:ap[3]] == -1).all() and (ma.cpu().numpy()[bp[2]:bp[3]] == -1).all()
    for g, w in zip((mb, ma, status), want):
        assert np.array_equal(g.cpu().numpy(), w)
    with pytest.raises(MpnhipError, match="problem 2 of 4.*not finite"):
        assignment.raise_on_status(status)
    with pytest.raises(MpnhipError, match="not finite"):
        assignment.linear_sum_assignment(up(problems[2], np.float64))


@pytest.mark.parametrize("shape", ((9, 14), (14, 9)))
def test_linear_sum_assignment_equals_scipy(shape):
    c = np.random.default_rng(34).uniform(-1, 1, shape)
    for maximize in (False, True):
        rows, cols = assignment.linear_sum_assignment(up(c, np.float64), maximize)
        want = scipy_lsa(c, maximize=maximize)
        assert rows.dtype == cols.dtype == np.int64 and np.array_equal(rows, want[0]) and np.array_equal(cols, want[1])


def test_the_largest_side_is_solved_and_one_more_is_refused():
    n = assignment.MAX_SIDE
    c = np.random.default_rng(36).uniform(-1, 1, (n + 1, 1))
    rows, cols = assignment.linear_sum_assignment(up(c[:n], np.float64))          # the last entry of the state's arrays
    assert rows.tolist() == [int(np.argmin(c[:n, 0]))] and cols.tolist() == [0]
    rows, cols = assignment.linear_sum_assignment(up(c[:n].T, np.float64), maximize=True)
    assert rows.tolist() == [0] and cols.tolist() == [int(np.argmax(c[:n, 0]))]
    for big in (c, c.T):
        with pytest.raises(MpnhipError, match="more than %d kept" % n):
            assignment.linear_sum_assignment(up(big, np.float64))
    keep = up(np.arange(n + 1) != 5, np.uint8)                                      # kept entries count, not the list's
    mb, ma, status = assignment.linear_sum_assignment_batched(up(c, np.float64), [0, n + 1], [0, n + 1], [0, 1], a_keep=keep)
    assert status.cpu().tolist() == [0] and int(ma.cpu()[0]) == int(np.argmin(np.where(np.arange(n + 1) == 5, np.inf, c[:, 0])))


def test_device_lists_take_their_sizes_from_the_masks():
    c = up(np.random.default_rng(35).uniform(-1, 1, 12), np.float64)
    lists = [up([0, 12], np.int64), up([0, 3], np.int32), up([0, 4], np.int32)]
    with pytest.raises(MpnhipError, match="a_keep"):
        assignment.linear_sum_assignment_batched(c, *lists)
    mb, ma, status = assignment.linear_sum_assignment_batched(c, *lists, a_keep=up(np.ones(3), np.uint8), b_keep=up(np.ones(4), np.uint8))
    r, k = scipy_lsa(c.cpu().numpy().reshape(3, 4))
    assert np.array_equal(mb.cpu().numpy(), k) and status.cpu().tolist() == [0]
    # bool masks go in as they are; entries that no problem owns (here: no problem at all) get -1
    mb, ma, status = assignment.linear_sum_assignment_batched(c, *(t[:1] for t in lists), a_keep=up(np.ones(3), bool), b_keep=up(np.ones(4), bool))
    assert mb.cpu().tolist() == [-1] * 3 and ma.cpu().tolist() == [-1] * 4 and status.numel() == 0


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(HR.GOLDEN))


@pytest.fixture(scope="module")
def gold22():
    return dict(np.load(R.GOLDEN))


@pytest.mark.parametrize("scene", HR.SCENES)
def test_evaluate_hota_files_on_the_device_equals_trackeval(gold, gold22, scene, tmp_path):
    pred, gt, T = HR.scene_files(gold, gold22, scene, tmp_path)
    for fpl in (1, 5, 64):
        first = HE.evaluate_hota_files(pred, gt, T, frames_per_launch=fpl, device=dev(), details=True, assignment="device")
        HR.assert_hota_equal(first, gold, scene)
        HR.assert_kept_ids(first, gold, scene)
        again = HE.evaluate_hota_files(pred, gt, T, frames_per_launch=fpl, device=dev(), details=True, assignment="device")
        assert sorted(again) == sorted(first)
        for k in HR.FIELDS + HE.COUNT_FIELDS:
            assert np.array_equal(first[k], again[k]), (fpl, k)   # the same bits on every call


def test_pass_two_copies_no_score_cell_and_no_match(gold, gold22, tmp_path, monkeypatch):
    """with assignment='device' the scores stay a device tensor and alpha_accumulate receives the solver's device tensor"""
    pred, gt, T = HR.scene_files(gold, gold22, "association", tmp_path)
    seen = []
    scores, accumulate = HE.frame_scores, HE.alpha_accumulate

    def frame_scores(*a, **kw):
        out = scores(*a, **kw)
        seen.append(("score", type(out), getattr(out, "is_cuda", False)))
        return out

    def alpha_accumulate(S, at, bt, match_b, *a):
        seen.append(("match", type(match_b), getattr(match_b, "is_cuda", False), getattr(match_b, "dtype", None)))
        return accumulate(S, at, bt, match_b, *a)
    monkeypatch.setattr(HE, "frame_scores", frame_scores)
    monkeypatch.setattr(HE, "alpha_accumulate", alpha_accumulate)
    monkeypatch.setattr(HE, "assign_frames", None)   # (the host solver is not reached)
    HE.evaluate_hota_files(pred, gt, T, frames_per_launch=5, device=dev(), assignment="device")
    assert len(seen) == 6 and all(s[1] is torch.Tensor and s[2] for s in seen) and all(s[3] == torch.int32 for s in seen if s[0] == "match")


def tracked_sequence():
    """the six-frame sequence of test_gpu_hota.py, restated: frames 1 .. 6 of 48 x 64 with four detections each (RoI masks
    28 x 28) -- detections of another class that only occlude, two tracks that swap, a dropped detection, a frame the tracker
    left empty; the ground truth as id images (frame 0 is empty): the masks of the first three detections of a frame moved by a
    pixel, one missing, and an ignore strip"""
    h, w, F, per = 48, 64, 6, 4
    rng = np.random.default_rng(22)
    n = F * per
    masks = FR.blob_masks(rng, n, 28, 28)
    frame = np.repeat(np.arange(1, F + 1), per)
    cx, cy = np.tile([14.0, 44.0, 20.0, 40.0], F) + rng.uniform(-3, 3, n), np.tile([12.0, 14.0, 34.0, 30.0], F) + rng.uniform(-3, 3, n)
    bw, bh = rng.uniform(16, 26, n), rng.uniform(14, 22, n)
    boxes = np.stack((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), axis=1)
    ped = np.tile(np.arange(per), F)
    ped[per * 3:per * 3 + 2] = [1, 0]
    label = np.full(n, 2)
    label[3::per] = 1
    keep = np.ones(n, bool)
    keep[[5, 8, 9, 10, 11]] = False
    gt = np.zeros((F + 1, h, w), np.uint16)
    for f in range(1, F + 1):
        idx = np.flatnonzero(frame == f)
        lab = np.roll(FR.np_frame(masks[idx], boxes[idx], h, w, 0.5)[0], tuple(rng.integers(-1, 2, 2)), axis=(0, 1))
        for j in range(3):
            if not (f == 5 and j == 2):
                gt[f][lab == j] = 2001 + j
    for f in (1, 2, 4):
        win = gt[f, :, w - 8:]
        win[win == 0] = 10000
    return masks, boxes, frame, ped, label, keep, gt, (h, w), F


def test_evaluate_hota_sequence_on_the_device_equals_the_host_route(tmp_path):
    masks, boxes, frame, ped, label, keep, gt, (h, w), F = tracked_sequence()
    n = masks.shape[0]
    node_preds = torch.from_numpy(masks).to(dev()).view(n, 1, 28, 28)
    gt_txt = R.write_txt(str(tmp_path / "gt.txt"), R.id_image_rows(gt))
    args = (node_preds, boxes, frame, torch.from_numpy(ped).to(dev()), label, torch.from_numpy(keep).to(dev()), (h, w), gt_txt, F + 1)
    want = tracker.evaluate_hota_sequence(*args, frames_per_launch=4, details=True, assignment="host")
    with pytest.raises(ValueError, match="assignment"):
        tracker.evaluate_hota_sequence(*args, assignment="Device")
    assert want["HOTA_TP"][0] >= 8 and want["HOTA_FN"][0] >= 1 and want["HOTA_FP"][0] >= 1
    for fpl in (1, 4, 64):
        got = tracker.evaluate_hota_sequence(*args, frames_per_launch=fpl, details=True, assignment="device")
        assert sorted(got) == sorted(want) and got["kept_tracker_ids"] == want["kept_tracker_ids"]
        for k in HE.INTEGER_ARRAY_FIELDS + HE.COUNT_FIELDS:
            assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
        for k in HE.FLOAT_ARRAY_FIELDS + HE.FLOAT_FIELDS:
            HR.close(got[k], want[k], k)
