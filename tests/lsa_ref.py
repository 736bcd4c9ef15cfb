"""numpy restatement of ``csrc/assignment.hip`` (``mpnhip_lsa_batched``) over the same batched layout, with the arithmetic order and
the tie rule of ``include/mpnhip.h``: the shortest augmenting path of Crouse 2016 on ``c = -cost if maximize else cost``, more kept
rows than kept columns on the transpose, ``r = ((minval + c[i][j]) - u[i]) - v[j]`` taken only if ``r < shortest[j]``, the next
column the unscanned one of lowest ``shortest`` -- among equals an unassigned one, lowest index first, otherwise the lowest
index.  Plus the operators of ``hota_ref`` with an ``assign_frames_device`` over it, for the evaluation's ``_ops`` route."""
import types

import numpy as np

import hota_ref as HR

MAX_SIDE = 2048   # MPNHIP_LSA_MAX_SIDE


def solve(c):
    """``c`` [nr, nc] (float64, nr <= nc) -> ``col4row`` [nr], or None where the costs are not finite (status 1)"""
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64)
    index = np.arange(nc)
    for cur in range(nr):
        shortest, path = np.full(nc, np.inf), np.full(nc, -1, np.int64)
        sr, sc = np.zeros(nr, bool), np.zeros(nc, bool)
        minval, i, sink = 0.0, cur, -1
        for _ in range(nc):
            sr[i] = True
            open_ = np.flatnonzero(~sc)
            r = ((minval + c[i, open_]) - u[i]) - v[open_]
            if np.isnan(r).any():
                return None
            less = r < shortest[open_]
            shortest[open_[less]], path[open_[less]] = r[less], i
            s = shortest[open_]
            if not np.isfinite(s.min()):
                return None
            tied = open_[s == s.min()]
            j = tied[np.lexsort((index[tied], row4col[tied] >= 0))[0]]
            minval = shortest[j]
            sc[j] = True
            if row4col[j] < 0:
                sink = j
                break
            i = row4col[j]
        if sink < 0:
            return None
        u[cur] += minval
        others = sr.copy()
        others[cur] = False
        u[others] += minval - shortest[col4row[others]]
        v[sc] -= minval - shortest[sc]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return col4row


def lsa_batched(cost, cell_ptr, a_ptr, b_ptr, a_keep=None, b_keep=None, maximize=False):
    """(match_b [n_a], match_a [n_b], status [n_problems]), int32, as ``mpnhip_lsa_batched`` writes them"""
    cost = np.asarray(cost, np.float64).reshape(-1)
    cell_ptr, a_ptr, b_ptr = (np.asarray(p, np.int64).reshape(-1) for p in (cell_ptr, a_ptr, b_ptr))
    n_a, n_b, F = int(a_ptr[-1]), int(b_ptr[-1]), a_ptr.size - 1
    ka = np.ones(n_a, bool) if a_keep is None else np.asarray(a_keep).reshape(-1).astype(bool)
    kb = np.ones(n_b, bool) if b_keep is None else np.asarray(b_keep).reshape(-1).astype(bool)
    match_b, match_a, status = np.full(n_a, -1, np.int32), np.full(n_b, -1, np.int32), np.zeros(F, np.int32)
    for f in range(F):
        a0, na, b0, nb = int(a_ptr[f]), int(a_ptr[f + 1] - a_ptr[f]), int(b_ptr[f]), int(b_ptr[f + 1] - b_ptr[f])
        rows, cols = np.flatnonzero(ka[a0:a0 + na]), np.flatnonzero(kb[b0:b0 + nb])
        if rows.size > MAX_SIDE or cols.size > MAX_SIDE:
            status[f] = 2
            continue
        if rows.size == 0 or cols.size == 0:
            continue
        c = cost[cell_ptr[f]:cell_ptr[f] + na * nb].reshape(na, nb)[np.ix_(rows, cols)]
        c = -c if maximize else c
        if rows.size > cols.size:
            col4row = solve(np.ascontiguousarray(c.T))
            pairs = None if col4row is None else (rows[col4row], cols)
        else:
            col4row = solve(c)
            pairs = None if col4row is None else (rows, cols[col4row])
        if pairs is None:
            status[f] = 1
            continue
        match_b[a0 + pairs[0]] = b0 + pairs[1]
        match_a[b0 + pairs[1]] = a0 + pairs[0]
    return match_b, match_a, status


def linear_sum_assignment(cost_2d, maximize=False):
    """(row_ind, col_ind) of one matrix, rows ascending: scipy's call over the restatement"""
    c = np.asarray(cost_2d, np.float64)
    na, nb = c.shape
    match_b, _, status = lsa_batched(c, [0, na * nb], [0, na], [0, nb], maximize=maximize)
    assert status[0] == 0
    rows = np.flatnonzero(match_b >= 0)
    return rows, match_b[rows].astype(np.int64)


def batch(problems):
    """(cost, cell_ptr, a_ptr, b_ptr) of a list of 2-D matrices, in the operator's layout"""
    shapes = np.array([p.shape for p in problems], np.int64).reshape(-1, 2)
    cost = np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in problems] + [np.zeros(0)])
    ptr = lambda n: np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    return cost, ptr(shapes[:, 0] * shapes[:, 1]), ptr(shapes[:, 0]), ptr(shapes[:, 1])


# ------------------------------------------------------------------------------------------------ the evaluation's _ops route
def frame_scores(S, a_traj, b_traj, acc, host=True):
    return HR.frame_scores(S, a_traj, b_traj, acc)   # (no device: the "device" scores are the host array)


def assign_frames_device(S, a_traj, b_traj, score_dev):
    a_keep = np.asarray(a_traj).reshape(-1) >= 0
    b_keep = (np.asarray(b_traj).reshape(-1) >= 0) & ~np.asarray(S["b_removed"]).astype(bool)
    match_b, _, status = lsa_batched(score_dev, S["sim_ptr"], S["a_ptr"], S["b_ptr"], a_keep, b_keep, maximize=True)
    assert (status == 0).all(), status
    return match_b


# hota_ref's operators with the two above: what ``evaluate_hota_files(..., assignment='device', _ops=OPS)`` runs over
OPS = types.SimpleNamespace(**{k: getattr(HR, k) for k in ("accumulators", "paint_label_runs", "label_overlap", "frame_similarity",
                                                           "accumulate_alignment", "alpha_accumulate", "association")},
                            frame_scores=frame_scores, assign_frames_device=assign_frames_device)
