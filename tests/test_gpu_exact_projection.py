"""The exact projector's LP on the device (``projectors.exact_round(solver='device')``, ``exact_plan``, ``ExactProjector`` and
``tracker.track_sequence`` with the device solver; csrc/exact_projection.hip + ``mpnhip_lsa_batched``) against the numpy / scipy
restatement of tests/exact_projection_ref.py, which tests/test_exact_projection_cpu.py pins to the reference's LP.  Plans and edge
values are integers and 0 / 1 flags: every comparison is exact.  On the fixture's case ``t`` (88 scores of exactly 0.5) the
optimum is not unique: there the objective (within 1e-9), feasibility and repeatability are checked instead of the edge vector."""
import math

import numpy as np
import pytest
import torch

import exact_projection_ref as XR
from mpntrackseg_amd import assignment, capi, projectors, tracker
from projection_ref import np_flows, np_violated
from test_exact_projection_cpu import UNIQUE
from test_gpu_projection import _dev, _graph, _np, _ordered, _same_rate, dev
from test_gpu_tracker_tail import _cfg, _inputs, _model
from test_gpu_workspace_exact import exact_call, filled, on
from test_projection_cpu import G19_CASES, g19_case
from test_tracker_tail_cpu import same_bits

pytestmark = pytest.mark.gpu

_REF = {}


def ref(z, tag):
    """the restatement of a fixture case in stored order, computed once"""
    if tag not in _REF:
        ei, p, n = g19_case(z, tag)
        _REF[tag] = XR.np_exact(ei, p, n)
    return _REF[tag]


def _feasible(ei, x, n):
    return np.bincount(ei[0], weights=x, minlength=n).max() <= 1 and np.bincount(ei[1], weights=x, minlength=n).max() <= 1


@pytest.mark.parametrize("order", ["stored", "permuted"])
@pytest.mark.parametrize("tag", G19_CASES)
def test_exact_round_on_the_device(golden, tag, order):
    z = golden("g19_projection.npz")
    ei0, p0, n = g19_case(z, tag)
    ei, p, _ = _ordered(z, tag, order)
    want, _ = ref(z, tag)
    if order == "permuted":    # (the permutation _ordered applied)
        perm = np.random.default_rng(len(tag) + ei0.shape[1]).permutation(ei0.shape[1])
        assert np.array_equal(ei, ei0[:, perm])
        want = want[perm]
    got, rate = projectors.exact_round(*_dev(ei, p), n, solver='device')
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (p.size,)
    assert isinstance(rate, float) and _same_rate(rate, z[f"{tag}:constr_satisf_rate"])
    got = _np(got)
    if tag in UNIQUE:
        assert same_bits(got, want)
    else:
        _, mask, ids = np_violated(ei, p, n)
        print("t (%s): objective %.9f, restatement %.9f" % (order, XR.objective(p[ids], got[ids]), XR.objective(p[ids], want[ids])))
        assert abs(XR.objective(p[ids], got[ids]) - XR.objective(p[ids], want[ids])) <= 1e-9
        assert np.isin(got, (0.0, 1.0)).all() and _feasible(ei[:, ids], got[ids].astype(np.float64), n)
        assert not got[mask & ~(p > 0.5)].any() and same_bits(got[~mask], np_flows(ei, p, n)[0][~mask])
        again, _ = projectors.exact_round(*_dev(ei, p), n, solver='device')
        assert _np(again).tobytes() == got.tobytes()


@pytest.mark.parametrize("tag", ["g17_l1", "hub", "a"])
def test_exact_plan(golden, tag):
    z = golden("g19_projection.npz")
    ei, p, n = g19_case(z, tag)
    want = ref(z, tag)[1]
    for order in ("stored", "permuted"):
        ei_o, p_o, _ = _ordered(z, tag, order)
        plan = projectors.exact_plan(*_dev(ei_o, p_o), n)
        assert (plan.n_problems, plan.n_a, plan.n_b, plan.max_side, plan.cells, plan.skipped_edges) == \
            (want.n_problems, want.n_a, want.n_b, want.max_side, want.cells, 0)
        assert plan.a_slot.dtype == torch.int32 and plan.a_ptr.dtype == torch.int32 and plan.cell_ptr.dtype == torch.int64
        for name in ("a_slot", "b_slot", "a_ptr", "b_ptr", "cell_ptr"):
            assert np.array_equal(_np(getattr(plan, name)), getattr(want, name)), (name, order)
    if tag == "g17_l1":
        assert plan.n_problems == 3
    if tag == "hub":    # one component wider than a wavefront, and than a block
        assert (plan.n_problems, plan.n_a, plan.n_b) == (1, 548, 537)


def test_many_small_problems_and_the_chain():
    ei, p, n = XR.copies(1500)
    perm = np.random.default_rng(5).permutation(p.size)
    got, rate = projectors.exact_round(*_dev(ei[:, perm], p[perm]), n, solver='device')
    out = np.empty(p.size, np.float32)
    out[perm] = _np(got)
    assert out.reshape(1500, 3).tolist() == [[0.0, 1.0, 1.0]] * 1500
    plan = projectors.exact_plan(*_dev(ei, p), n)
    assert (plan.n_problems, plan.n_a, plan.n_b, plan.max_side, plan.cells) == (1500, 3000, 3000, 2, 6000)
    assert np.array_equal(_np(plan.cell_ptr), 4 * np.arange(1501)) and np.array_equal(_np(plan.a_ptr), 2 * np.arange(1501))
    # 0 -> 1 -> 2 with both edges in the mask: node 1 is a column of one problem and the row of another
    chain, cp = np.array([[0, 1], [1, 2]]), np.array([0.9, 0.8], np.float32)
    plan = projectors.exact_plan(*_dev(chain, cp), 3, edges_mask=torch.ones(2, dtype=torch.bool, device=dev()))
    want = XR.np_plan(chain, cp, 3, edges_mask=np.ones(2, bool))
    assert (plan.n_problems, plan.n_a, plan.n_b, plan.max_side, plan.cells) == (2, 2, 2, 1, 2)
    for name in ("a_slot", "b_slot", "a_ptr", "b_ptr", "cell_ptr"):
        assert np.array_equal(_np(getattr(plan, name)), getattr(want, name)), name
    # ... and as the violated sub-problem it is empty: nothing to solve
    assert projectors.exact_plan(*_dev(chain, cp), 3).n_problems == 0


def test_edge_shapes(monkeypatch):
    status_reads = []
    real = assignment.raise_on_status
    monkeypatch.setattr(assignment, "raise_on_status", lambda *a, **k: (status_reads.append(1), real(*a, **k)))
    empty = torch.empty((2, 0), dtype=torch.int64, device=dev()), torch.empty(0, device=dev())
    for nodes in (0, 1, 7):
        got, rate = projectors.exact_round(*empty, nodes, solver='device')
        assert got.numel() == 0 and math.isnan(rate)
        assert projectors.exact_plan(*empty, nodes).n_problems == 0
    # no violated constraint: the rounded scores, and the second read does not happen
    chain = np.array([[0, 1, 2], [1, 2, 3]])
    got, rate = projectors.exact_round(*_dev(chain, np.array([0.9, 0.2, 0.8], np.float32)), 4, solver='device')
    assert _np(got).tolist() == [1.0, 0.0, 1.0] and rate == 1.0 and not status_reads
    # the three-edge graph, then with a NaN score
    ei, p, n = XR.THREE_EDGES
    got, _ = projectors.exact_round(*_dev(ei, p), n, solver='device')
    assert _np(got).tolist() == [0.0, 1.0, 1.0] and len(status_reads) == 1
    assert _np(projectors.greedy_round(*_dev(ei, p), n)[0]).tolist() == [1.0, 0.0, 0.0]
    got, _ = projectors.exact_round(*_dev(ei, np.array([0.9, np.nan, 0.85], np.float32)), n, solver='device')
    assert _np(got).tolist() == [1.0, 0.0, 0.0]
    # a duplicate pair: the larger score is the cell's, the lower edge id among equals; the losers end at 0
    dup = np.array([[0, 0, 0, 1], [3, 3, 4, 3]])
    for scores, want in (([0.9, 0.9, 0.6, 0.55], [1, 0, 0, 0]), ([0.9, 0.95, 0.6, 0.55], [0, 1, 0, 0]), ([0.9, 0.95, 0.8, 0.85], [0, 0, 1, 1])):
        sc = np.array(scores, np.float32)
        assert XR.np_exact(dup, sc, 5)[0].tolist() == want
        got, _ = projectors.exact_round(*_dev(dup, sc), 5, solver='device')
        assert _np(got).tolist() == want, scores
    # an end point outside [0, N) is never followed and is reported
    with pytest.raises(IndexError):
        projectors.exact_round(*_dev(np.array([[0, 0, 1], [1, 2, 5]]), np.array([0.75, 0.9, 0.9], np.float32)), 5, solver='device')
    with pytest.raises(IndexError):
        projectors.exact_plan(*_dev(np.array([[0, 0, 1], [1, 2, 5]]), np.array([0.75, 0.9, 0.9], np.float32)), 5)
    with pytest.raises(IndexError):     # a graph without nodes: every edge leaves it
        projectors.exact_round(*_dev(np.array([[0], [1]]), np.array([0.9], np.float32)), 0, solver='device')


def test_a_component_over_the_assignment_limit_is_refused():
    k = assignment.MAX_SIDE + 1
    ei = np.stack((np.zeros(k, np.int64), np.arange(1, k + 1)))
    t = _dev(ei, np.full(k, 0.9, np.float32))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(capi.MpnhipError, match="host solver"):
        projectors.exact_round(*t, k + 1, solver='device')
    assert torch.cuda.memory_allocated() - before < 1 << 20     # no cost buffer (2049 cells here, but refused before any)
    plan = projectors.exact_plan(*t, k + 1)
    assert (plan.n_problems, plan.n_a, plan.n_b, plan.max_side) == (1, 1, k, k)
    # one edge less is solved: the best-scored edge stays
    p = np.full(k - 1, 0.9, np.float32)
    p[1234] = 0.95
    got, _ = projectors.exact_round(*_dev(ei[:, :k - 1], p), k + 1, solver='device')
    assert np.flatnonzero(_np(got)).tolist() == [1234]


@pytest.mark.parametrize("tag", ["a", "g17_l2"])
def test_exact_projector_class(golden, tag):
    pytest.importorskip("scipy")
    z = golden("g19_projection.npz")
    ei, p, n = g19_case(z, tag)
    host = _graph(ei, p, n)
    proj_host = projectors.ExactProjector(host, solver=projectors.solve_with_scipy)
    proj_host.project()
    for kw in (dict(solver_backend='device'), dict(solver='device')):
        fg = _graph(ei, p, n)
        proj = projectors.ExactProjector(fg, **kw)
        proj.project()
        assert torch.equal(fg.graph_obj.edge_preds, host.graph_obj.edge_preds)
        assert proj.constr_satisf_rate == proj_host.constr_satisf_rate
    with pytest.raises(ValueError):
        projectors.ExactProjector(_graph(ei, p, n), solver='gpu')
    with pytest.raises(ValueError):
        projectors.exact_round(*_dev(ei, p), n, solver='gpu')


def test_track_sequence_with_the_device_solver(golden):
    pytest.importorskip("scipy")
    z = golden("g17_window_tail.npz")
    args, x_ext = _inputs(z, "s")
    model = _model()
    cfg = _cfg(z, "s1")
    host = tracker.track_sequence(model, *args, x_ext=x_ext, rounding_method='exact', solver=projectors.solve_with_scipy, **cfg)
    got = tracker.track_sequence(model, *args, x_ext=x_ext, rounding_method='exact', solver='device', **cfg)
    assert torch.equal(got.edge_index, host.edge_index) and torch.equal(got.edge_preds, host.edge_preds)
    assert torch.equal(got.ped_ids, host.ped_ids) and torch.equal(got.keep, host.keep)
    assert got.constr_satisf_rate == host.constr_satisf_rate
    with pytest.raises(ValueError):
        tracker.track_sequence(model, *args, rounding_method='exact', solver='gpu', **cfg)


@pytest.mark.parametrize("n", [64, 65])
def test_workspace_is_exact(n):
    """In the manner of tests/test_gpu_workspace_exact.py: the three calls through the C ABI with exactly
    ``mpnhip_project_exact_workspace_bytes``; one byte less is refused with MPNHIP_ERR_WORKSPACE before anything is written."""
    lib = capi.load()
    rng = np.random.default_rng(7)
    K = 300
    pairs = {(n - 2, n - 1), (0, n - 1)}
    while len(pairs) < K:
        i, j = rng.integers(0, n, 2)
        if i != j:
            pairs.add((min(i, j), max(i, j)))
    ei = np.ascontiguousarray(np.array(sorted(pairs), np.int64).T[:, rng.permutation(K)])
    preds = rng.random(K).astype(np.float32)
    preds[:2] = 0.75
    mask = np_violated(ei, preds, n)[1]
    want_x, want = XR.np_exact(ei, preds, n)
    want_cost = XR.np_cost(want, ei, preds)[0]
    assert want.n_problems >= 1 and want.max_side > 1 and 0 < mask.sum()
    ei_d, p_d, mask_d, rp_d = on(ei), on(preds), on(mask, np.uint8), on(np_flows(ei, preds, n)[0])
    a_slot, b_slot = filled((n,), torch.int32), filled((n,), torch.int32)
    a_ptr, b_ptr, cell_ptr, sizes = filled((n + 1,), torch.int32), filled((n + 1,), torch.int32), filled((n + 1,), torch.int64), filled((6,), torch.int64)
    need = lib.mpnhip_project_exact_workspace_bytes(n, K)
    s = capi.stream_ptr
    ws = exact_call("project_exact_plan", need,
                    lambda w, b: lib.mpnhip_project_exact_plan(capi.ptr(ei_d), K, n, capi.ptr(p_d), capi.ptr(mask_d), capi.ptr(a_slot), capi.ptr(b_slot),
                                                               capi.ptr(a_ptr), capi.ptr(b_ptr), capi.ptr(cell_ptr), capi.ptr(sizes), w, b, s()),
                    [a_slot, b_slot, a_ptr, b_ptr, cell_ptr, sizes])
    F, n_a, n_b, max_side, cells, skipped = sizes.tolist()
    assert (F, n_a, n_b, max_side, cells, skipped) == (want.n_problems, want.n_a, want.n_b, want.max_side, want.cells, 0)
    assert np.array_equal(_np(a_slot), want.a_slot) and np.array_equal(_np(b_slot), want.b_slot)
    assert np.array_equal(_np(a_ptr)[:F + 1], want.a_ptr) and np.array_equal(_np(cell_ptr)[:F + 1], want.cell_ptr)
    assert (_np(a_ptr)[F:] == n_a).all() and (_np(b_ptr)[F:] == n_b).all() and (_np(cell_ptr)[F:] == cells).all()
    cost = filled((cells,), torch.float64)
    exact_call("project_exact_fill", need,
               lambda w, b: lib.mpnhip_project_exact_fill(capi.ptr(ei_d), K, n, capi.ptr(p_d), capi.ptr(mask_d), capi.ptr(a_slot), capi.ptr(b_slot),
                                                          capi.ptr(a_ptr), capi.ptr(b_ptr), capi.ptr(cell_ptr), F, n_a, n_b, capi.ptr(cost), cells, w, b, s()),
               [cost], ws=ws)
    assert _np(cost).tobytes() == want_cost.tobytes()
    match_b, _, status = assignment.linear_sum_assignment_batched(cost, cell_ptr[:F + 1], a_ptr[:F + 1], b_ptr[:F + 1],
                                                                  a_keep=torch.ones(n_a, dtype=torch.uint8, device=dev()),
                                                                  b_keep=torch.ones(n_b, dtype=torch.uint8, device=dev()))
    assert not status.any()
    out = filled((K,), torch.float32)
    exact_call("project_exact_apply", need,
               lambda w, b: lib.mpnhip_project_exact_apply(capi.ptr(ei_d), K, n, capi.ptr(mask_d), capi.ptr(rp_d), capi.ptr(a_slot), capi.ptr(b_slot),
                                                           capi.ptr(match_b), n_a, capi.ptr(out), w, b, s()), [out], ws=ws)
    got = _np(out)
    ids = np.flatnonzero(mask)
    assert np.isin(got, (0.0, 1.0)).all() and _feasible(ei[:, ids], got[ids].astype(np.float64), n)
    assert abs(XR.objective(preds[ids], got[ids]) - XR.objective(preds[ids], want_x[ids])) <= 1e-9
    assert same_bits(got[~mask], want_x[~mask])
