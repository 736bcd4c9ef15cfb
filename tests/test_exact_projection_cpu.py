"""The exact projector's device solver, without a device: the restatement of tests/exact_projection_ref.py (the rounding LP as one
dense assignment per connected component of the active edges' bipartite graph) against the reference's LP itself
(``projectors.solve_with_scipy``) on the sub-problem ``ExactProjector`` hands over, for every case of
tests/golden/g19_projection.npz; the new C-ABI symbols and the argument checks of the new entry points."""
import ctypes

import numpy as np
import pytest

from exact_projection_ref import THREE_EDGES, copies, np_cost, np_exact, np_plan, objective
from mpntrackseg_amd import capi
from projection_ref import np_greedy, np_violated
from test_projection_cpu import G19_CASES, MPNHIP_ERR_WORKSPACE, g19_case

UNIQUE = [t for t in G19_CASES if t != "t"]
NEW_SYMBOLS = ["mpnhip_project_exact_workspace_bytes", "mpnhip_project_exact_plan", "mpnhip_project_exact_fill",
               "mpnhip_project_exact_apply"]


def _sub(z, tag):
    ei, p, n = g19_case(z, tag)
    ids = np_violated(ei, p, n)[2]
    return ei, p, n, ids


def _feasible(ei, x, n):
    return np.bincount(ei[0], weights=x, minlength=n).max() <= 1 and np.bincount(ei[1], weights=x, minlength=n).max() <= 1


@pytest.mark.parametrize("tag", G19_CASES)
def test_restatement_solves_the_reference_lp(golden, tag):
    pytest.importorskip("scipy")
    from mpntrackseg_amd import projectors
    z = golden("g19_projection.npz")
    ei, p, n, ids = _sub(z, tag)
    assert ids.size > 0
    got, plan = np_exact(ei, p, n)
    lp = projectors.snap(projectors.solve_with_scipy(ei[:, ids], p[ids]))
    assert np.isin(got, (0.0, 1.0)).all() and np.isin(lp, (0.0, 1.0)).all()
    print("%s: %d problems, sides up to %d, %d cells; objective %.6f" % (tag, plan.n_problems, plan.max_side, plan.cells,
                                                                       objective(p[ids], got[ids])))
    if tag in UNIQUE:
        assert np.array_equal(got[ids], lp.astype(np.float32))
    else:   # 88 scores of exactly 0.5: the optimum is not unique
        assert abs(objective(p[ids], got[ids]) - objective(p[ids], lp)) <= 1e-9
        assert _feasible(ei[:, ids], got[ids].astype(np.float64), n)
    assert _feasible(ei[:, ids], got[ids].astype(np.float64), n)
    # outside the sub-problem: the rounded scores
    outside = np.ones(p.size, bool)
    outside[ids] = False
    assert np.array_equal(got[outside], (p[outside] > 0.5).astype(np.float32))
    # strictly better than the greedy rounding of the same sub-problem
    greedy = np_greedy(ei[:, ids], p[ids], n)[0]
    assert objective(p[ids], got[ids]) < objective(p[ids], greedy)


def test_plan_sizes_of_the_fixture(golden):
    z = golden("g19_projection.npz")
    plan = np_plan(*g19_case(z, "g17_l1"))
    assert plan.n_problems == 3
    plan = np_plan(*g19_case(z, "hub"))
    assert (plan.n_problems, plan.n_a, plan.n_b, plan.max_side, plan.cells) == (1, 548, 537, 548, 548 * 537)
    for tag in G19_CASES:
        assert 0 < np_plan(*g19_case(z, tag)).max_side <= 2048


def test_restatement_on_hand_made_graphs():
    pytest.importorskip("scipy")
    ei, p, n = THREE_EDGES
    assert np_exact(ei, p, n)[0].tolist() == [0, 1, 1]
    assert np_greedy(ei, p, n)[0].tolist() == [1, 0, 0]
    plan = np_plan(ei, p, n)
    assert (plan.n_problems, plan.n_a, plan.n_b, plan.cells) == (1, 2, 2, 4)
    assert plan.a_slot.tolist() == [0, 1, -1, -1, -1] and plan.b_slot.tolist() == [-1, -1, -1, 0, 1]
    cost, winner, cell = np_cost(plan, ei, p)
    assert cost.tolist() == [1.0 - 2.0 * float(np.float32(0.9)), 1.0 - 2.0 * float(np.float32(0.8)), 1.0 - 2.0 * float(np.float32(0.85)), 0.0]
    assert winner.all() and cell.tolist() == [0, 1, 2]
    ei3, p3, n3 = copies(3)
    assert np_exact(ei3, p3, n3)[0].tolist() == [0, 1, 1] * 3 and np_plan(ei3, p3, n3).cell_ptr.tolist() == [0, 4, 8, 12]
    # the chain 0 -> 1 -> 2 with every edge in the mask: node 1 is a column of the first problem and the row of the second
    chain = np.array([[0, 1], [1, 2]])
    plan = np_plan(chain, np.array([0.9, 0.8], np.float32), 3, edges_mask=np.ones(2, bool))
    assert (plan.n_problems, plan.max_side, plan.cells) == (2, 1, 2)
    assert plan.a_slot.tolist() == [0, 1, -1] and plan.b_slot.tolist() == [-1, 0, 1]
    # a duplicate pair: the larger score is the cell's, the lower edge id among equals
    dup = np.array([[0, 0, 0, 1], [3, 3, 4, 3]])
    assert np_exact(dup, np.array([0.9, 0.9, 0.6, 0.55], np.float32), 5)[0].tolist() == [1, 0, 0, 0]
    assert np_exact(dup, np.array([0.9, 0.95, 0.6, 0.55], np.float32), 5)[0].tolist() == [0, 1, 0, 0]
    assert np_exact(dup, np.array([0.9, 0.95, 0.8, 0.85], np.float32), 5)[0].tolist() == [0, 0, 1, 1]
    # a NaN score is not active
    assert np_exact(ei, np.array([0.9, np.nan, 0.85], np.float32), n)[0].tolist() == [1, 0, 0]


def test_new_symbols_are_exported():
    lib = ctypes.CDLL(capi.lib_path())
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.SIGNATURES, name


def test_solver_argument_is_checked_without_gpu():
    import types
    from mpntrackseg_amd import projectors
    fg = types.SimpleNamespace(graph_obj=types.SimpleNamespace(edge_index=None, edge_preds=None, num_nodes=0))
    with pytest.raises(ValueError, match="device"):
        projectors.ExactProjector(fg, solver='gpu')
    assert projectors.ExactProjector(fg, solver_backend='device').solver_backend == 'device'
    assert projectors.ExactProjector(fg, solver='device').solver == 'device'
    with pytest.raises(ValueError):
        projectors.check_solver('host')
    projectors.check_solver(None), projectors.check_solver(len), projectors.check_solver('device')


def test_exact_entry_points_argument_checks_without_gpu():
    """Size queries and argument checks run on the host: null pointers with a non-zero size and bad sizes are refused before any
    launch with the function's name in mpnhip_last_error(), a short workspace is MPNHIP_ERR_WORKSPACE."""
    l = capi.load()
    one = ctypes.c_void_p(256)   # a non-null address that no call below may reach a launch with
    big = 1 << 30
    size = l.mpnhip_project_exact_workspace_bytes
    assert size(0, 0) == 0 and size(-1, 5) == 0 and size(5, -1) == 0 and size(1 << 30, 5) == 0 and size(5, 1 << 30) == 0
    # per node: parent and root of both copies, flags, ranks, counts, products, sort keys and values; one flag per edge
    assert size(1000, 0) >= 1000 * (16 + 2 + 8 + 8 + 8 + 16) and size(1000, 100000) >= size(1000, 0) + 100000
    assert size(100000, 5000) > size(1000, 5000)
    # plan
    plan = l.mpnhip_project_exact_plan
    assert plan(one, -1, 4, one, one, one, one, one, one, one, one, one, big, None) != 0
    assert b"project_exact_plan" in l.mpnhip_last_error()
    assert plan(one, 5, 1 << 30, one, one, one, one, one, one, one, one, one, big, None) != 0
    assert plan(one, 5, 4, one, one, one, one, one, one, one, None, one, big, None) != 0           # sizes are always written
    assert plan(one, 5, 4, one, one, one, one, None, one, one, one, one, big, None) != 0           # ... and the prefix lists
    assert plan(one, 5, 4, one, one, None, one, one, one, one, one, one, big, None) != 0
    assert plan(None, 5, 4, one, one, one, one, one, one, one, one, one, big, None) != 0
    assert plan(one, 5, 4, one, None, one, one, one, one, one, one, one, big, None) != 0
    assert b"project_exact_plan" in l.mpnhip_last_error()
    assert plan(one, 5, 400, one, one, one, one, one, one, one, one, one, size(400, 5) - 1, None) == MPNHIP_ERR_WORKSPACE
    assert plan(one, 5, 400, one, one, one, one, one, one, one, one, None, big, None) == MPNHIP_ERR_WORKSPACE
    assert b"project_exact_plan" in l.mpnhip_last_error()
    # fill
    fill = l.mpnhip_project_exact_fill
    assert fill(None, 0, 0, None, None, None, None, None, None, None, 0, 0, 0, None, 0, None, 0, None) == 0
    assert fill(one, -5, 4, one, one, one, one, one, one, one, 1, 1, 1, one, 1, one, big, None) != 0
    assert b"project_exact_fill" in l.mpnhip_last_error()
    assert fill(None, 5, 4, one, one, one, one, one, one, one, 1, 1, 1, one, 1, one, big, None) != 0
    assert fill(one, 5, 4, one, one, None, one, one, one, one, 1, 1, 1, one, 1, one, big, None) != 0
    assert fill(one, 5, 4, one, one, one, one, one, one, one, 5, 1, 1, one, 1, one, big, None) != 0     # more problems than nodes
    assert fill(one, 5, 4, one, one, one, one, one, one, one, 1, 1, 1, one, -1, one, big, None) != 0
    assert fill(one, 5, 4, one, one, one, one, one, one, one, 1, 1, 1, None, 1, one, big, None) != 0    # cells without a cost buffer
    assert b"project_exact_fill" in l.mpnhip_last_error()
    assert fill(one, 5, 400, one, one, one, one, one, one, one, 1, 1, 1, one, 1, one, size(400, 5) - 1, None) == MPNHIP_ERR_WORKSPACE
    assert b"project_exact_fill" in l.mpnhip_last_error()
    # apply
    apply = l.mpnhip_project_exact_apply
    assert apply(None, 0, 0, None, None, None, None, None, 0, None, None, 0, None) == 0
    assert apply(one, 5, -4, one, one, one, one, one, 1, one, one, big, None) != 0
    assert b"project_exact_apply" in l.mpnhip_last_error()
    assert apply(one, 5, 4, one, one, one, one, one, 1, None, one, big, None) != 0
    assert apply(one, 5, 4, one, one, one, None, one, 1, one, one, big, None) != 0
    assert apply(one, 5, 4, one, one, one, one, None, 1, one, one, big, None) != 0                      # rows without a match list
    assert apply(one, 5, 4, one, one, one, one, one, 5, one, one, big, None) != 0                       # more rows than nodes
    assert b"project_exact_apply" in l.mpnhip_last_error()
    assert apply(one, 5, 400, one, one, one, one, one, 1, one, one, size(400, 5) - 1, None) == MPNHIP_ERR_WORKSPACE
    assert apply(one, 5, 400, one, one, one, one, one, 1, one, None, 0, None) == MPNHIP_ERR_WORKSPACE
    assert b"project_exact_apply" in l.mpnhip_last_error()
