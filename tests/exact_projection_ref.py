"""Numpy / scipy restatement of the exact projector's device solver (test infrastructure only): the plan of
``mpnhip_project_exact_plan`` -- the active edges' bipartite graph of out-copies against in-copies, its connected components as
problems ordered by their smallest vertex, rows and columns by ascending node id --, the cost cells of
``mpnhip_project_exact_fill`` with the winner rule for duplicate pairs, one ``scipy.optimize.linear_sum_assignment`` per problem,
and the edge values of ``mpnhip_project_exact_apply``.  tests/test_exact_projection_cpu.py pins it to the reference's LP
(``projectors.solve_with_scipy``); tests/test_gpu_exact_projection.py uses it as the expectation."""
import collections

import numpy as np

from projection_ref import np_flows, np_labels, np_violated

Plan = collections.namedtuple("Plan", ["a_slot", "b_slot", "a_ptr", "b_ptr", "cell_ptr", "n_problems", "n_a", "n_b", "max_side", "cells",
                                       "skipped_edges", "active"])


def np_active(edge_index, edge_preds, num_nodes, edges_mask):
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    in_range = (ei >= 0).all(axis=0) & (ei < num_nodes).all(axis=0)
    with np.errstate(invalid="ignore"):
        return in_range & np.asarray(edges_mask, bool) & (np.asarray(edge_preds, np.float32) > np.float32(0.5)), int((~in_range).sum())


def np_plan(edge_index, edge_preds, num_nodes, edges_mask=None):
    """``edges_mask`` None: the violated sub-problem's."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    n = int(num_nodes)
    if edges_mask is None:
        edges_mask = np_violated(ei, edge_preds, n)[1]
    active, skipped = np_active(ei, edge_preds, n, edges_mask)
    u, v = ei[0][active], ei[1][active]
    lab = np_labels(np.stack((u, n + v)), np.ones(u.size, np.float32), 2 * n)      # ranked by the component's smallest vertex
    has = np.zeros(2 * n, bool)
    has[u] = True
    has[n + v] = True
    probs = np.unique(lab[has])
    F = probs.size
    prob_of = np.searchsorted(probs, lab)
    slots, ptrs, counts = [], [], []
    for side in (0, 1):
        nodes = np.flatnonzero(has[side * n:(side + 1) * n])
        f = prob_of[side * n + nodes]
        nodes = nodes[np.lexsort((nodes, f))]
        slot = np.full(n, -1, np.int32)
        slot[nodes] = np.arange(nodes.size, dtype=np.int32)
        cnt = np.bincount(f, minlength=F).astype(np.int64)
        slots.append(slot)
        counts.append(cnt)
        ptrs.append(np.concatenate(([0], np.cumsum(cnt))).astype(np.int32))
    cell_ptr = np.concatenate(([0], np.cumsum(counts[0] * counts[1]))).astype(np.int64)
    max_side = int(max(counts[0].max(), counts[1].max())) if F else 0
    return Plan(slots[0], slots[1], ptrs[0], ptrs[1], cell_ptr, F, int(ptrs[0][-1]), int(ptrs[1][-1]), max_side, int(cell_ptr[-1]),
                skipped, active)


def np_cost(plan, edge_index, edge_preds):
    """``(cost [cells] float64, winner [K] bool, cell [K] or -1)``: per pair the largest score wins, the lowest edge id among equals."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    p = np.asarray(edge_preds, np.float32)
    cost = np.zeros(plan.cells, np.float64)
    best = {}
    cell = np.full(p.size, -1, np.int64)
    for e in np.flatnonzero(plan.active):
        sa, sb = int(plan.a_slot[ei[0, e]]), int(plan.b_slot[ei[1, e]])
        f = int(np.searchsorted(plan.a_ptr, sa, side="right")) - 1
        nb = int(plan.b_ptr[f + 1] - plan.b_ptr[f])
        cell[e] = plan.cell_ptr[f] + (sa - plan.a_ptr[f]) * nb + (sb - plan.b_ptr[f])
        if cell[e] not in best or p[e] > p[best[cell[e]]]:      # (ascending edge ids: an equal score does not replace)
            best[cell[e]] = e
    winner = np.zeros(p.size, bool)
    for c, e in best.items():
        winner[e] = True
        cost[c] = 1.0 - 2.0 * np.float64(p[e])
    return cost, winner, cell


def np_assign(plan, cost):
    """``match_b [n_a]``: scipy's assignment of every problem, as entries of the whole column list."""
    from scipy.optimize import linear_sum_assignment
    match_b = np.full(plan.n_a, -1, np.int32)
    for f in range(plan.n_problems):
        a0, b0 = int(plan.a_ptr[f]), int(plan.b_ptr[f])
        na, nb = int(plan.a_ptr[f + 1]) - a0, int(plan.b_ptr[f + 1]) - b0
        r, c = linear_sum_assignment(cost[plan.cell_ptr[f]:plan.cell_ptr[f + 1]].reshape(na, nb))
        match_b[a0 + r] = b0 + c
    return match_b


def np_exact(edge_index, edge_preds, num_nodes, edges_mask=None):
    """``(values [K] float32, plan)``: the rounded scores outside the mask; inside, 1 for the winners the assignment chose."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    if edges_mask is None:
        edges_mask = np_violated(ei, edge_preds, num_nodes)[1]
    edges_mask = np.asarray(edges_mask, bool)
    plan = np_plan(ei, edge_preds, num_nodes, edges_mask)
    cost, winner, _ = np_cost(plan, ei, edge_preds)
    match_b = np_assign(plan, cost)
    out = np_flows(ei, edge_preds, num_nodes)[0].copy()
    out[edges_mask] = 0
    for e in np.flatnonzero(winner):
        if match_b[plan.a_slot[ei[0, e]]] == plan.b_slot[ei[1, e]]:
            out[e] = 1
    return out, plan


def objective(edge_preds, x):
    return float(((1.0 - 2.0 * np.asarray(edge_preds, np.float32).astype(np.float64)) * np.asarray(x, np.float64)).sum())


THREE_EDGES = (np.array([[0, 0, 1], [3, 4, 3]], np.int64), np.array([0.9, 0.8, 0.85], np.float32), 5)


def copies(k):
    """``k`` disjoint copies of the three-edge graph: ``k`` problems of 2 x 2."""
    ei, p, n = THREE_EDGES
    return np.concatenate([ei + n * i for i in range(k)], axis=1), np.tile(p, k), n * k
