"""The batched linear sum assignment without a GPU: the numpy restatement of the operator (tests/lsa_ref.py) against scipy, HOTA
over it through the evaluation's ``_ops`` route, and the host-side checks of the entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment as scipy_lsa

import hota_ref as HR
import lsa_ref as LR
import mots_metrics_ref as R
from mpntrackseg_amd import assignment, capi, hota_eval as HE

SHAPES = ((1, 1), (1, 7), (7, 1), (5, 5), (63, 64), (64, 65), (65, 63), (129, 70), (70, 129), (110, 115))


def tie_heavy(rng, shape):
    """integer-valued doubles, 80 % zeros"""
    return np.where(rng.random(shape) < 0.8, 0.0, rng.integers(1, 10, shape).astype(np.float64))


@pytest.mark.parametrize("maximize", (False, True))
def test_restatement_gives_scipys_assignment_on_continuous_costs(maximize):
    rng = np.random.default_rng(5)
    for shape in SHAPES:
        c = rng.uniform(-1, 1, shape)
        rows, cols = LR.linear_sum_assignment(c, maximize)
        want = scipy_lsa(c, maximize=maximize)
        assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1]), shape


def test_restatement_reaches_scipys_optimum_on_tie_heavy_costs():
    rng = np.random.default_rng(6)
    for shape in SHAPES:
        c = tie_heavy(rng, shape)
        rows, cols = LR.linear_sum_assignment(c, True)
        want = scipy_lsa(c, maximize=True)
        assert c[rows, cols].sum() == c[want].sum(), shape   # (integer-valued doubles sum exactly)
        assert rows.size == min(shape) and np.unique(rows).size == rows.size and np.unique(cols).size == cols.size, shape


def test_keep_masks_with_holes_equal_scipy_on_the_sub_matrix():
    rng = np.random.default_rng(7)
    problems = [rng.uniform(-1, 1, s) for s in ((9, 14), (14, 9), (20, 21), (6, 6))]
    cost, cp, ap, bp = LR.batch(problems)
    ka, kb = rng.random(ap[-1]) < 0.7, rng.random(bp[-1]) < 0.7
    ka[ap[2]:ap[3]] = True                      # problem 2: 20 x 21, but 20 kept rows against 10 kept columns
    kb[bp[2]:bp[3]] = np.arange(21) % 2 == 1
    for maximize in (False, True):
        mb, ma, status = LR.lsa_batched(cost, cp, ap, bp, ka, kb, maximize)
        assert (status == 0).all()
        for f, c in enumerate(problems):
            rows, cols = np.flatnonzero(ka[ap[f]:ap[f + 1]]), np.flatnonzero(kb[bp[f]:bp[f + 1]])
            r, k = scipy_lsa(c[np.ix_(rows, cols)], maximize=maximize)
            want = np.full(c.shape[0], -1)
            want[rows[r]] = bp[f] + cols[k]
            assert np.array_equal(mb[ap[f]:ap[f + 1]], want), (f, maximize)
        pairs = np.flatnonzero(mb >= 0)
        assert np.array_equal(ma[mb[pairs]], pairs) and (ma >= 0).sum() == pairs.size   # match_a is the inverse


def test_no_kept_row_or_no_kept_column_gives_nothing():
    rng = np.random.default_rng(8)
    cost, cp, ap, bp = LR.batch([rng.uniform(-1, 1, s) for s in ((4, 5), (0, 5), (5, 0), (3, 3), (0, 0))])
    ka, kb = np.ones(ap[-1], bool), np.ones(bp[-1], bool)
    ka[ap[0]:ap[1]] = False
    kb[bp[3]:bp[4]] = False
    mb, ma, status = LR.lsa_batched(cost, cp, ap, bp, ka, kb)
    assert (mb == -1).all() and (ma == -1).all() and (status == 0).all()


def test_costs_that_are_not_finite_stop_their_problem_alone():
    rng = np.random.default_rng(9)
    problems = [rng.uniform(-1, 1, s) for s in ((6, 7), (8, 8), (7, 6), (5, 9), (4, 4))]
    problems[1][3, 5] = np.nan
    problems[3][2, :] = np.inf
    cost, cp, ap, bp = LR.batch(problems)
    for maximize in (False, True):
        mb, ma, status = LR.lsa_batched(cost, cp, ap, bp, maximize=maximize)
        assert status.tolist() == [0, 1, 0, 1, 0]
        for f, c in enumerate(problems):
            if status[f]:
                assert (mb[ap[f]:ap[f + 1]] == -1).all() and (ma[bp[f]:bp[f + 1]] == -1).all()
            else:
                r, k = scipy_lsa(c, maximize=maximize)
                assert np.array_equal(mb[ap[f] + r], bp[f] + k), f
    # +inf cells that leave a finite complete assignment are no obstacle (scipy solves these too)
    c = rng.uniform(-1, 1, (5, 6))
    c[0, 1:] = c[1:, 0] = np.inf
    rows, cols = LR.linear_sum_assignment(c)
    want = scipy_lsa(c)
    assert np.array_equal(cols, want[1]) and cols[0] == 0


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(HR.GOLDEN))


@pytest.fixture(scope="module")
def gold22():
    return dict(np.load(R.GOLDEN))


@pytest.mark.parametrize("scene", HR.SCENES)
def test_hota_over_the_restated_solver_equals_trackeval(gold, gold22, scene, tmp_path):
    """the fixture's results do not depend on how ties among zero-score cells are broken"""
    pred, gt, T = HR.scene_files(gold, gold22, scene, tmp_path)
    results = [HE.evaluate_hota_files(pred, gt, T, frames_per_launch=fpl, details=True, _ops=LR.OPS, assignment="device") for fpl in (1, 5, 64)]
    HR.assert_hota_equal(results[0], gold, scene)
    HR.assert_kept_ids(results[0], gold, scene)
    for res in results[1:]:
        for k in HR.FIELDS + HE.COUNT_FIELDS:
            assert np.array_equal(res[k], results[0][k]), k   # the same bits whatever the launches are


def test_an_unknown_assignment_is_refused(tmp_path):
    ids = np.zeros((1, 4, 4), np.uint16)
    ids[0, :2, :2] = 2001
    txt = HR.loaded(ids, tmp_path, "one")
    with pytest.raises(ValueError, match="assignment"):
        HE.evaluate_hota_files(txt, txt, 1, _ops=HR, assignment="bogus")
    with pytest.raises(ValueError, match="assignment"):
        HE._evaluate(txt, 1, 2, 10, 8, None, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), None, None, ops=HR,
                     assignment="Device")
    assert HE.evaluate_hota_files(txt, txt, 1, _ops=HR, assignment="host")["HOTA(0)"] == 1.0


def test_an_unsolved_frame_raises_once_per_sequence():
    import torch
    solved, launches = {"assign_status": torch.zeros(3, dtype=torch.int32)}, [{}, {"assign_status": None}]
    HE.check_assignment_status(launches + [solved])
    with pytest.raises(capi.MpnhipError, match="assign_frames_device: problem 4 of 5: more than %d kept" % assignment.MAX_SIDE):
        HE.check_assignment_status([solved] + launches + [{"assign_status": torch.tensor([0, 2], dtype=torch.int32)}])


def test_max_side_is_the_headers():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpnhip.h")).read()
    side = int(re.search(r"#define MPNHIP_LSA_MAX_SIDE (\d+)", src).group(1))
    assert side == assignment.MAX_SIDE == LR.MAX_SIDE
    assert 46 * side <= 160 * 1024 < 46 * 2 * side   # the state of one problem against the LDS of one workgroup


def test_entry_point_argument_checks_without_gpu():
    """everything below returns before a kernel is launched (the non-null pointers are host dummies, never dereferenced)"""
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)

    def call(cost=p, cells=12, cell_ptr=p, a_ptr=p, n_a=3, b_ptr=p, n_b=4, n_problems=1, match_b=p, status=p, ws=p, ws_bytes=256):
        return l.mpnhip_lsa_batched(cost, cells, cell_ptr, a_ptr, n_a, b_ptr, n_b, n_problems, None, None, 0, match_b, None, status, ws,
                                    ws_bytes, None)
    # nothing to do: a successful no-op, whatever is null
    for kw in (dict(n_problems=0), dict(n_a=0, n_b=0, cells=0)):
        assert l.mpnhip_lsa_batched(None, kw.get("cells", 12), None, None, kw.get("n_a", 3), None, kw.get("n_b", 4), kw.get("n_problems", 1),
                                    None, None, 0, None, None, None, None, 0, None) == 0, kw
    for name in ("cost", "cell_ptr", "a_ptr", "b_ptr", "match_b", "status"):
        assert call(**{name: None}) == -1, name
        assert b"lsa_batched" in l.mpnhip_last_error(), name
    for kw in (dict(n_a=-1), dict(n_b=-1), dict(n_problems=-1), dict(cells=-1)):
        assert call(**kw) == -1, kw
        assert b"lsa_batched" in l.mpnhip_last_error(), kw
    assert call(ws=None) == -3 and call(ws_bytes=255) == -3
    assert b"lsa_batched" in l.mpnhip_last_error()
    assert call(cells=1 << 31) == -4 and call(cells=(1 << 31) - 1, ws=None) == -3


def test_workspace_bytes_are_monotone_and_refuse_negative_sizes():
    wb = capi.load().mpnhip_lsa_workspace_bytes
    sizes = [wb(a, b, f) for a, b, f in ((0, 0, 0), (1, 1, 1), (10, 1, 1), (10, 20, 1), (10, 20, 8), (5000, 6000, 64), (1 << 20, 1 << 20, 65535))]
    assert sizes[0] >= 0 and all(x <= y for x, y in zip(sizes, sizes[1:])) and sizes[1] > 0
    for a, b, f in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        assert wb(a, b, f) == 0
