"""From edge scores to track ids on the device: ``projectors.greedy_round`` / ``violated_subproblem`` / the two projector classes,
``tracker.assign_ped_ids``, ``tracker.drop_short_trajectories`` and ``tracker.track_sequence`` against the reference's own outputs
(tests/golden/g19_projection.npz, tools/make_golden.py gen_g19) and the numpy restatement of tests/projection_ref.py.  Everything is
integer or compare-only arithmetic: all comparisons are exact."""
import math
import types

import numpy as np
import pytest
import torch

from mpntrackseg_amd import projectors, tracker
from projection_ref import component_graphs, np_flows, np_greedy, np_keep, np_labels, np_violated
from test_gpu_tracker_tail import _cfg, _inputs, _model
from test_projection_cpu import G19_CASES, SYNTHETIC, g19_case
from test_tracker_tail_cpu import same_bits

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(ei, p):
    return torch.from_numpy(np.ascontiguousarray(ei)).to(dev()), torch.from_numpy(np.ascontiguousarray(p)).to(dev())


def _same_rate(got, want):
    """``got``: a Python float as the reference's ``.item()`` gives; ``want``: the float32 of the fixture / restatement."""
    return (math.isnan(got) and np.isnan(want)) or same_bits(np.float32(got), np.float32(want)) and float(np.float32(got)) == got


def _ordered(z, tag, order):
    ei, p, n = g19_case(z, tag)
    if order == "permuted":
        perm = np.random.default_rng(len(tag) + ei.shape[1]).permutation(ei.shape[1])
        ei, p = np.ascontiguousarray(ei[:, perm]), p[perm]
    return ei, p, n


def _graph(ei, p, n):
    t_ei, t_p = _dev(ei, p)
    return types.SimpleNamespace(graph_obj=types.SimpleNamespace(edge_index=t_ei, edge_preds=t_p, num_nodes=n))


@pytest.mark.parametrize("order", ["stored", "permuted"])
@pytest.mark.parametrize("tag", G19_CASES)
def test_greedy_round_and_both_projectors(golden, tag, order):
    z = golden("g19_projection.npz")
    ei, p, n = _ordered(z, tag, order)
    want, want_rate, info = np_greedy(ei, p, n)     # tie-breaks follow the edge id: the restatement sees the same list
    if order == "stored":
        assert same_bits(want, z[f"{tag}:round_preds"]) and same_bits(want_rate, z[f"{tag}:constr_satisf_rate"])
    got, rate = projectors.greedy_round(*_dev(ei, p), n)
    assert got.dtype == torch.float32 and got.is_cuda and same_bits(_np(got), want)
    assert isinstance(rate, float) and _same_rate(rate, want_rate)
    # the flow counts behind it
    fl = projectors.flow_counts(*_dev(ei, p), n)
    rp0, flow_out, flow_in, v_out, v_in, nc = np_flows(ei, p, n)
    assert same_bits(_np(fl.round_preds), rp0)
    assert np.array_equal(_np(fl.flow_out), flow_out) and np.array_equal(_np(fl.flow_in), flow_in)
    assert (fl.violated_out, fl.violated_in, fl.num_constraints) == (v_out, v_in, nc)
    assert (v_out, v_in) == (info["violated_out"], info["violated_in"])
    # GreedyProjector: the reference's protocol
    fg = _graph(ei, p, n)
    proj = projectors.GreedyProjector(fg)
    proj.project()
    assert same_bits(_np(fg.graph_obj.edge_preds), want) and _same_rate(proj.constr_satisf_rate, want_rate)
    # ExactProjector with the greedy rounding of the sub-problem as its "solver": rounded values outside, the solver's inside
    _, edges_mask, ids = np_violated(ei, p, n)
    seen = []

    def solver(sub_ei, sub_p):
        seen.append((sub_ei.copy(), sub_p.copy()))
        return np_greedy(sub_ei, sub_p, n)[0]
    fg = _graph(ei, p, n)
    proj = projectors.ExactProjector(fg, solver_backend='pulp', solver=solver)
    proj.project()
    expect = rp0.copy()
    expect[ids] = np_greedy(ei[:, ids], p[ids], n)[0]
    assert len(seen) == 1 and np.array_equal(seen[0][0], ei[:, ids]) and same_bits(seen[0][1], p[ids])
    assert same_bits(_np(fg.graph_obj.edge_preds), expect) and _same_rate(proj.constr_satisf_rate, want_rate)


def test_greedy_round_repeats_bitwise(golden):
    z = golden("g19_projection.npz")
    for tag in ("hub", "t"):
        ei, p, n = g19_case(z, tag)
        t = _dev(ei, p)
        first, rate = projectors.greedy_round(*t, n)
        first = _np(first).tobytes()
        for _ in range(3):
            again, rate2 = projectors.greedy_round(*t, n)
            assert _np(again).tobytes() == first and rate2 == rate


def test_greedy_round_large_random_and_degenerate():
    """100,000 edges over 5,000 nodes with scores on a grid of 64 values (many ties, several hundred blocks), then the empty
    shapes and an edge that leaves the graph."""
    rng = np.random.default_rng(31)
    n, K = 5000, 100000
    a, b = rng.integers(0, n, K), rng.integers(0, n, K)
    sel = a != b
    ei = np.stack((np.minimum(a, b)[sel], np.maximum(a, b)[sel])).astype(np.int64)
    p = (rng.integers(0, 65, ei.shape[1]) / 64).astype(np.float32)
    want, want_rate, info = np_greedy(ei, p, n)
    assert info["ties"] > 100 and info["cleared_by_a"] > 100 and info["violated_in"] - info["cleared_by_a"] > 100
    got, rate = projectors.greedy_round(*_dev(ei, p), n)
    assert same_bits(_np(got), want) and _same_rate(rate, want_rate)
    # no edges: nothing rounded, no constraint, 0 / 0
    empty = torch.empty((2, 0), dtype=torch.int64, device=dev()), torch.empty(0, device=dev())
    for nodes in (0, 1, 7):
        got, rate = projectors.greedy_round(*empty, nodes)
        assert got.numel() == 0 and math.isnan(rate)
        sub = projectors.violated_subproblem(*empty, nodes)
        assert sub.nodes_mask.numel() == nodes and not bool(sub.nodes_mask.any()) and sub.edge_ids.numel() == 0
    # one edge, nothing violated
    got, rate = projectors.greedy_round(*_dev(np.array([[0], [1]]), np.array([0.75], np.float32)), 2)
    assert _np(got).tolist() == [1.0] and rate == 1.0
    # an end point outside [0, N) is never followed and is reported
    with pytest.raises(IndexError):
        projectors.greedy_round(*_dev(np.array([[0, 1], [1, 5]]), np.array([0.75, 0.9], np.float32)), 5)


@pytest.mark.parametrize("tag", SYNTHETIC)
def test_violated_subproblem(golden, tag):
    z = golden("g19_projection.npz")
    ei, p, n = g19_case(z, tag)
    nodes, edges, ids = np_violated(ei, p, n)
    assert ids.size > 0 and nodes.any()
    sub = projectors.violated_subproblem(*_dev(ei, p), n)
    assert sub.nodes_mask.dtype == torch.bool and np.array_equal(_np(sub.nodes_mask), nodes)
    assert sub.edges_mask.dtype == torch.bool and np.array_equal(_np(sub.edges_mask), edges)
    assert sub.edge_ids.dtype == torch.int32 and np.array_equal(_np(sub.edge_ids).astype(np.int64), ids)
    assert np.array_equal(_np(sub.edge_index), ei[:, ids]) and same_bits(_np(sub.edge_preds), p[ids])
    assert same_bits(_np(sub.round_preds), np_flows(ei, p, n)[0])
    assert _same_rate(sub.constr_satisf_rate, z[f"{tag}:constr_satisf_rate"])


def test_exact_projector_writes_solver_values_inside_the_mask_only(golden):
    z = golden("g19_projection.npz")
    ei, p, n = g19_case(z, "hub")      # (in the 48-node cases every edge touches a violated node)
    _, edges_mask, ids = np_violated(ei, p, n)
    rp0 = np_flows(ei, p, n)[0]
    assert 0 < ids.size < ei.shape[1]
    fixed = np.linspace(0.0, 1.0, ids.size)        # values the snapping leaves alone, except near the two ends
    fixed[1], fixed[-2] = 5e-7, 1.0 - 5e-7
    fg = _graph(ei, p, n)
    proj = projectors.ExactProjector(fg, solver=lambda sub_ei, sub_p: fixed)
    proj.project()
    got = _np(fg.graph_obj.edge_preds)
    assert same_bits(got[~edges_mask], rp0[~edges_mask])
    want_in = fixed.copy()
    want_in[1], want_in[-2] = 0.0, 1.0
    assert same_bits(got[edges_mask], want_in.astype(np.float32))
    assert _same_rate(proj.constr_satisf_rate, z["hub:constr_satisf_rate"])
    # a star at node 0 next to edges no violated node touches, active and not: those take the rounded values
    ei2, p2 = np.array([[0, 0, 4, 6, 8], [1, 2, 5, 7, 9]]), np.array([0.9, 0.8, 0.7, 0.3, 0.6], np.float32)
    out, rate = projectors.exact_round(*_dev(ei2, p2), 10, solver=lambda sub_ei, sub_p: np.array([0.25, 0.75]))
    assert _np(out).tolist() == [0.25, 0.75, 1.0, 0.0, 1.0] and _same_rate(rate, np.float32(1) - np.float32(1) / np.float32(9))
    # a solver that answers for another number of edges is refused
    with pytest.raises(RuntimeError):
        projectors.exact_round(*_dev(ei, p), n, solver=lambda sub_ei, sub_p: fixed[:-1])
    # nothing violated: the solver is not asked
    chain = np.array([[0, 1, 2], [1, 2, 3]])
    out, rate = projectors.exact_round(*_dev(chain, np.array([0.9, 0.2, 0.8], np.float32)), 4, solver=lambda *a: 1 / 0)
    assert _np(out).tolist() == [1.0, 0.0, 1.0] and rate == 1.0


def test_exact_projector_with_the_default_solver(golden):
    pytest.importorskip("scipy")
    z = golden("g19_projection.npz")
    ei, p, n = g19_case(z, "b")
    fg = _graph(ei, p, n)
    proj = projectors.ExactProjector(fg)
    proj.project()
    x = _np(fg.graph_obj.edge_preds)
    assert np.isin(x, (0.0, 1.0)).all()
    assert np.bincount(ei[0], weights=x, minlength=n).max() <= 1 and np.bincount(ei[1], weights=x, minlength=n).max() <= 1
    cost = lambda v: float(((1.0 - 2.0 * p.astype(np.float64)) * v).sum())
    assert cost(x) <= cost(z["b:round_preds"]) + p.size * 1e-6    # no worse than the greedy rounding
    with pytest.raises(Exception, match="gurobi"):
        projectors.ExactProjector(_graph(ei, p, n), solver_backend='gurobi').project()


@pytest.mark.parametrize("tag", G19_CASES)
def test_ped_ids_and_track_lengths_reproduce_the_reference(golden, tag):
    z = golden("g19_projection.npz")
    ei, _, n = g19_case(z, tag)
    t_ei, t_rp = _dev(ei, z[f"{tag}:round_preds"])
    ids = tracker.assign_ped_ids(t_ei, t_rp, n)
    assert ids.dtype == torch.int64 and ids.is_cuda and np.array_equal(_np(ids), z[f"{tag}:ped_ids"])
    for mtl in (2, 5):
        keep = tracker.drop_short_trajectories(ids, mtl)
        assert keep.dtype == torch.bool and np.array_equal(_np(keep), z[f"{tag}:keep{mtl}"])
    # the components do not depend on the edge order
    perm = np.random.default_rng(7).permutation(ei.shape[1])
    again = tracker.assign_ped_ids(*_dev(ei[:, perm], z[f"{tag}:round_preds"][perm]), n)
    assert torch.equal(again, ids)


@pytest.mark.parametrize("name", sorted(component_graphs()))
def test_components_of_hand_made_graphs(name):
    ei, p, n = component_graphs()[name]
    want = np_labels(ei, p, n)
    ids = tracker.assign_ped_ids(*_dev(ei, p), n)
    assert tuple(ids.shape) == (n,) and np.array_equal(_np(ids), want), name
    flipped = tracker.assign_ped_ids(*_dev(ei[::-1], p), n)      # (col, row): the graph is undirected
    assert torch.equal(flipped, ids)
    for mtl in (1, 2, 3, 200, 302):
        assert np.array_equal(_np(tracker.drop_short_trajectories(ids, mtl)), np_keep(want, mtl)), (name, mtl)


def test_components_degenerate():
    empty = torch.empty((2, 0), dtype=torch.int64, device=dev()), torch.empty(0, device=dev())
    ids = tracker.assign_ped_ids(*empty, 0)
    assert ids.dtype == torch.int64 and ids.numel() == 0
    assert tracker.drop_short_trajectories(ids, 2).numel() == 0
    # ids are not renumbered: a mask over arbitrary labels in [0, N)
    labels = torch.tensor([4, 4, 0, 2, 4, 2], device=dev())
    assert _np(tracker.drop_short_trajectories(labels, 3)).tolist() == [True, True, False, False, True, False]


def test_track_sequence_on_a_g17_sequence(golden):
    z = golden("g17_window_tail.npz")
    args, x_ext = _inputs(z, "s")
    n = args[0].shape[0]
    model = _model()
    cfg = _cfg(z, "s1")
    seq = tracker.evaluate_sequence(model, *args, x_ext=x_ext, **cfg)
    ei, p = _np(seq.edge_index), _np(seq.edge_preds)
    want_rp, want_rate, info = np_greedy(ei, p, n)
    want_ids = np_labels(ei, want_rp, n)
    assert info["violated_out"] > 0 and info["violated_in"] > info["cleared_by_a"]     # the rounding is not vacuous here
    for mtl in (2, 3):
        res = tracker.track_sequence(model, *args, x_ext=x_ext, min_track_len=mtl, **cfg)
        assert torch.equal(res.edge_index, seq.edge_index) and torch.equal(res.final_edge_preds, seq.final_edge_preds)
        assert torch.equal(res.node_preds, seq.node_preds)
        assert same_bits(_np(res.edge_preds), want_rp) and _same_rate(res.constr_satisf_rate, want_rate)
        assert res.ped_ids.dtype == torch.int64 and np.array_equal(_np(res.ped_ids), want_ids)
        assert res.keep.dtype == torch.bool and np.array_equal(_np(res.keep), np_keep(want_ids, mtl))
    assert tracker.track_sequence(model, *args, **cfg).node_preds is None       # defaults: greedy, min_track_len 2, no masks
    # 'exact' with a caller's solver
    res = tracker.track_sequence(model, *args, rounding_method='exact', solver=lambda sub_ei, sub_p: np_greedy(sub_ei, sub_p, n)[0], **cfg)
    _, _, ids = np_violated(ei, p, n)
    expect = np_flows(ei, p, n)[0]
    expect[ids] = np_greedy(ei[:, ids], p[ids], n)[0]
    assert same_bits(_np(res.edge_preds), expect) and np.array_equal(_np(res.ped_ids), np_labels(ei, expect, n))
    with pytest.raises(RuntimeError, match="Rounding type for projector not understood"):
        tracker.track_sequence(model, *args, rounding_method='nearest', **cfg)
