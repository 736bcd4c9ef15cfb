"""Host mirror of the reference's projectors (``src/mot_neural_solver/tracker/projectors.py``) over the C ABI -- SURVEY.md
section 8 row f-3: the edge scores of a sequence graph are rounded to 0 / 1 so that every node keeps at most one incoming and one
outgoing edge.

``GreedyProjector`` / ``ExactProjector`` have the reference's names, constructor arguments and ``project()`` protocol: they read
``full_graph.graph_obj.{edge_index, edge_preds, num_nodes}``, write ``graph_obj.edge_preds`` and set ``constr_satisf_rate``.
``greedy_round`` / ``violated_subproblem`` are the functional forms.  The edge list is undirected with row < col per edge (what
``tracker.evaluate_sequence`` returns), in any edge order; tensors live on the HIP device (there is no CPU fallback).

The greedy rounding runs on the device (``csrc/projection.hip``: two edge-parallel passes instead of the reference's Python
loop); of the exact one, the flow counts and the violated sub-problem do.  Its linear program runs on the host by default
(``pulp`` or scipy's HiGHS, or a caller's ``solver`` callable) and, with ``solver='device'``, on the device as well: the LP is a
maximum-weight bipartite matching, which ``csrc/exact_projection.hip`` splits into connected components and hands to the batched
linear assignment of ``csrc/assignment.hip`` -- no edge list, score or match leaves the device (``exact_round``)."""
import collections

import numpy as np
import torch

from . import assignment, capi
from .capi import MpnhipError, check, ptr, stream_ptr
from .graph import compact as _compact, gather_edges as _gather_edges, gather_rows as _gather_rows

Flows = collections.namedtuple('Flows', ['round_preds', 'flow_out', 'flow_in', 'violated_out', 'violated_in', 'num_constraints',
                                         'constr_satisf_rate'])


def _edge_inputs(edge_index, edge_preds):
    capi.require_device(edge_index, edge_preds)
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise MpnhipError("edge_index must be [2, K]")
    ei = edge_index.to(torch.int64).contiguous()
    p = capi.f32c(edge_preds).view(-1)
    if p.numel() != ei.shape[1]:
        raise MpnhipError("one score per edge (%d scores, %d edges)" % (p.numel(), ei.shape[1]))
    return ei, p


def _empty(n, dtype, device):
    return torch.empty(max(int(n), 1), dtype=dtype, device=device)[:int(n)]


def _round_and_count(ei, p, num_nodes):
    """Launches ``mpnhip_project_round_count``; returns the device tensors ``(round_preds, flow_out, flow_in, counters)``."""
    lib = capi.load()
    K, N, dev = ei.shape[1], int(num_nodes), p.device
    rp = _empty(K, torch.float32, dev)
    flow_out, flow_in = _empty(N, torch.int32, dev), _empty(N, torch.int32, dev)
    counters = torch.zeros(8, dtype=torch.int32, device=dev)
    ws = capi.workspace(lib.mpnhip_project_round_count_workspace_bytes(N), dev, "project")
    check(lib.mpnhip_project_round_count(ptr(ei), K, N, ptr(p), ptr(rp), ptr(flow_out), ptr(flow_in), ptr(counters), ptr(ws), ws.numel(),
                                         stream_ptr()), "mpnhip_project_round_count")
    return rp, flow_out, flow_in, counters


def _read_counters(counters, num_nodes):
    """The one host read.  ``constr_sat_rate = 1 - violated.float() / num_constraints`` with the reference's own float32
    operations (utils/evaluation.py:406-409); no constraint at all gives 0 / 0 = NaN as there."""
    v_out, v_in, n_constr, bad = counters[:4].tolist()
    if bad:
        raise IndexError("index out of range in edge_index: %d edges have an end point outside [0, %d)" % (bad, int(num_nodes)))
    rate = (1 - torch.tensor(v_out + v_in).float() / n_constr).item()
    return v_out, v_in, n_constr, rate


@capi.on_tensor_device
def flow_counts(edge_index, edge_preds, num_nodes):
    """``compute_constr_satisfaction_rate(graph_obj, (edge_preds > 0.5).float(), undirected_edges=False, return_flow_vals=True)``
    (utils/evaluation.py:370-414) as a ``Flows``: the rounded scores, the per-node counts (int32) and the rate."""
    ei, p = _edge_inputs(edge_index, edge_preds)
    rp, flow_out, flow_in, counters = _round_and_count(ei, p, num_nodes)
    v_out, v_in, n_constr, rate = _read_counters(counters, num_nodes)
    return Flows(rp, flow_out, flow_in, v_out, v_in, n_constr, rate)


@capi.on_tensor_device
def greedy_round(edge_index, edge_preds, num_nodes):
    """``GreedyProjector.project`` (projectors.py:19-67): returns ``(round_preds [K] float32 of 0 / 1, constr_satisf_rate)``.
    Every node with more than one active (> 0.5) outgoing edge keeps the one with the largest score, the lowest edge id on a tie;
    then the same over the incoming edges of the nodes that still have more than one.  One host read (the constraint counters),
    after both passes have been enqueued."""
    lib = capi.load()
    ei, p = _edge_inputs(edge_index, edge_preds)
    K, N = ei.shape[1], int(num_nodes)
    rp, flow_out, flow_in, counters = _round_and_count(ei, p, N)
    ws = capi.workspace(lib.mpnhip_project_greedy_workspace_bytes(N), p.device, "project")
    check(lib.mpnhip_project_greedy(ptr(ei), K, N, ptr(p), ptr(rp), ptr(flow_out), ptr(flow_in), ptr(ws), ws.numel(), stream_ptr()),
          "mpnhip_project_greedy")
    return rp, _read_counters(counters, N)[3]


def _violated_masks(ei, p, num_nodes):
    """``_round_and_count`` and ``mpnhip_project_violated_masks``: ``(round_preds, counters, nodes_mask, edges_mask)`` on the
    device (the masks as uint8)."""
    lib = capi.load()
    K, N, dev = ei.shape[1], int(num_nodes), p.device
    rp, flow_out, flow_in, counters = _round_and_count(ei, p, N)
    nodes_mask, edges_mask = _empty(N, torch.uint8, dev), _empty(K, torch.uint8, dev)
    check(lib.mpnhip_project_violated_masks(ptr(ei), K, N, ptr(flow_out), ptr(flow_in), ptr(nodes_mask), ptr(edges_mask), stream_ptr()),
          "mpnhip_project_violated_masks")
    return rp, counters, nodes_mask, edges_mask


Subproblem = collections.namedtuple('Subproblem', ['nodes_mask', 'edges_mask', 'edge_ids', 'edge_index', 'edge_preds', 'round_preds',
                                                   'constr_satisf_rate'])


@capi.on_tensor_device
def violated_subproblem(edge_index, edge_preds, num_nodes):
    """The graph ``ExactProjector.project`` hands to its solver (projectors.py:83-98), as a ``Subproblem``: ``nodes_mask`` [N] =
    ``flow_in > 1 | flow_out > 1``, ``edges_mask`` [K] = an end point in it (both bool), ``edge_ids`` [M] int32 ascending,
    ``edge_index`` [2, M] / ``edge_preds`` [M] of those edges, plus the rounded scores of ALL edges and the rate."""
    ei, p = _edge_inputs(edge_index, edge_preds)
    K, N, dev = ei.shape[1], int(num_nodes), p.device
    rp, counters, nodes_mask, edges_mask = _violated_masks(ei, p, N)
    rate = _read_counters(counters, N)[3]
    if K == 0:
        return Subproblem(nodes_mask.bool(), edges_mask.bool(), torch.empty(0, dtype=torch.int32, device=dev), ei, p, rp, rate)
    ids, _ = _compact(edges_mask)
    return Subproblem(nodes_mask.bool(), edges_mask.bool(), ids, _gather_edges(ei, ids, 0), _gather_rows(p.view(-1, 1), ids).view(-1),
                      rp, rate)


def _lp_matrices(edge_index, edge_preds):
    """The LP of ``PuLPMinCostFlowSolver`` (projectors.py:129-160): minimise sum x_e (1 - 2 p_e), 0 <= x <= 1, per node in-flow <= 1
    and out-flow <= 1.  Returns ``(c [M], A [2 nodes, M] sparse)``."""
    from scipy import sparse
    ei = np.asarray(edge_index, dtype=np.int64)
    M = ei.shape[1]
    nodes, local = np.unique(ei, return_inverse=True)
    local = local.reshape(2, M)
    rows = np.concatenate((2 * local[1], 2 * local[0] + 1))   # row 2n: in-flow of n, row 2n + 1: its out-flow
    cols = np.concatenate((np.arange(M), np.arange(M)))
    A = sparse.csr_matrix((np.ones(2 * M), (rows, cols)), shape=(2 * nodes.size, M))
    return 1.0 - 2.0 * np.asarray(edge_preds, dtype=np.float64), A


def solve_with_scipy(edge_index, edge_preds):
    """The reference's LP through ``scipy.optimize.linprog(method='highs-ds')``.  The constraint matrix is the incidence matrix
    of a bipartite graph (out-side / in-side copies of the nodes), hence totally unimodular: the simplex vertex is integral."""
    from scipy.optimize import linprog
    c, A = _lp_matrices(edge_index, edge_preds)
    if c.size == 0:
        return np.zeros(0)
    res = linprog(c, A_ub=A, b_ub=np.ones(A.shape[0]), bounds=(0, 1), method='highs-ds')
    if res.status != 0:
        raise MpnhipError("linprog did not solve the rounding LP: %s" % res.message)
    return res.x


def solve_with_pulp(edge_index, edge_preds):
    """``PuLPMinCostFlowSolver`` (projectors.py:116-160) with PuLP's default solver."""
    import pulp as plp
    ei = np.asarray(edge_index, dtype=np.int64)
    assert (ei[0] < ei[1]).all(), "Cannot project a graph with duplicated edges!"
    M = ei.shape[1]
    m = plp.LpProblem(name='MinCostFlowLP')
    xs = [plp.LpVariable(lowBound=0, upBound=1, cat=plp.LpContinuous, name='e%d' % e) for e in range(M)]
    m.sense = plp.LpMinimize
    m.setObjective(plp.lpSum(xs[e] * (1 - 2 * float(edge_preds[e])) for e in range(M)))
    for side in (1, 0):
        order = np.argsort(ei[side], kind='stable')
        for seg in np.split(order, np.flatnonzero(np.diff(ei[side][order])) + 1):
            m.addConstraint(plp.LpConstraint(e=plp.lpSum(xs[e] for e in seg), sense=plp.LpConstraintLE, rhs=1))
    m.solve()
    return np.array([x.varValue for x in xs], dtype=np.float64)


def default_solver():
    """``pulp`` if it imports (the reference's backend), else scipy's HiGHS dual simplex on the same LP."""
    try:
        import pulp  # noqa: F401
        return solve_with_pulp
    except ImportError:
        pass
    try:
        import scipy.optimize  # noqa: F401
        return solve_with_scipy
    except ImportError:
        raise MpnhipError("ExactProjector needs an LP solver on the host: install pulp (the reference's backend) or scipy >= 1.6 "
                          "(scipy.optimize.linprog with HiGHS), or pass solver=callable(edge_index [2, M], edge_preds [M]) -> values [M]")


def snap(values, tol=1e-6):
    """Solver values within ``tol`` of 0 or 1 become exactly 0 or 1 (a simplex vertex of this LP is integral up to the solver's
    feasibility tolerance)."""
    v = np.array(values, dtype=np.float64).reshape(-1)
    v[np.abs(v) <= tol] = 0.0
    v[np.abs(v - 1.0) <= tol] = 1.0
    return v


ExactPlan = collections.namedtuple('ExactPlan', ['a_slot', 'b_slot', 'a_ptr', 'b_ptr', 'cell_ptr', 'n_problems', 'n_a', 'n_b', 'max_side',
                                                 'cells', 'skipped_edges'])

DEVICE_SOLVER = 'device'


def _exact_plan(ei, p, num_nodes, edges_mask):
    """Launches ``mpnhip_project_exact_plan``; returns the device tensors ``(a_slot, b_slot, a_ptr, b_ptr, cell_ptr, sizes)`` (the
    prefix lists at their capacity of ``num_nodes + 1``) and the workspace that the fill and the apply go on with."""
    lib = capi.load()
    K, N, dev = ei.shape[1], int(num_nodes), p.device
    a_slot, b_slot = _empty(N, torch.int32, dev), _empty(N, torch.int32, dev)
    a_ptr, b_ptr = torch.empty(N + 1, dtype=torch.int32, device=dev), torch.empty(N + 1, dtype=torch.int32, device=dev)
    cell_ptr, sizes = torch.empty(N + 1, dtype=torch.int64, device=dev), torch.empty(6, dtype=torch.int64, device=dev)
    need = lib.mpnhip_project_exact_workspace_bytes(N, K)
    if need == 0 and (N or K):
        raise MpnhipError("%d nodes and %d edges are not supported" % (N, K))
    ws = capi.workspace(need, dev, "project_exact")   # (a tag of its own: the winner flags at its head outlive the assignment's launch)
    check(lib.mpnhip_project_exact_plan(ptr(ei), K, N, ptr(p), ptr(edges_mask), ptr(a_slot), ptr(b_slot), ptr(a_ptr), ptr(b_ptr),
                                        ptr(cell_ptr), ptr(sizes), ptr(ws), ws.numel(), stream_ptr()), "mpnhip_project_exact_plan")
    return a_slot, b_slot, a_ptr, b_ptr, cell_ptr, sizes, ws


def _read_counters_and_sizes(counters, sizes, num_nodes):
    """ONE host read of the constraint counters and the plan's sizes: ``(constr_satisf_rate, sizes as six ints)``."""
    both = torch.cat((counters.to(torch.int64), sizes)).tolist()
    v_out, v_in, n_constr, bad = both[:4]
    if bad:
        raise IndexError("index out of range in edge_index: %d edges have an end point outside [0, %d)" % (bad, int(num_nodes)))
    return (1 - torch.tensor(v_out + v_in).float() / n_constr).item(), both[8:]


@capi.on_tensor_device
def exact_plan(edge_index, edge_preds, num_nodes, edges_mask=None):
    """The assignment problems the device solver makes of the violated sub-problem (``mpnhip_project_exact_plan``), as an
    ``ExactPlan``: ``a_slot`` / ``b_slot`` [N] int32 (position of a node's out-copy among all rows / of its in-copy among all
    columns, or -1), ``a_ptr`` / ``b_ptr`` (int32) / ``cell_ptr`` (int64) [n_problems + 1], all on the device, and the sizes as
    Python ints.  ``edges_mask`` [K] (bool or uint8): the edges that take part; None: the violated sub-problem's."""
    ei, p = _edge_inputs(edge_index, edge_preds)
    _, counters, _, mask = _violated_masks(ei, p, num_nodes)
    if edges_mask is not None:
        mask = edges_mask.to(p.device).contiguous().view(-1)
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.ne(0).view(torch.uint8)
        if mask.numel() != ei.shape[1]:
            raise MpnhipError("one mask flag per edge")
    a_slot, b_slot, a_ptr, b_ptr, cell_ptr, sizes, _ = _exact_plan(ei, p, num_nodes, mask)
    _, sz = _read_counters_and_sizes(counters, sizes, num_nodes)
    F = sz[0]
    return ExactPlan(a_slot, b_slot, a_ptr[:F + 1], b_ptr[:F + 1], cell_ptr[:F + 1], *sz)


def _exact_round_device(ei, p, num_nodes):
    """``exact_round`` with the LP as batched assignment on the device.  Two host reads of a few integers: the constraint
    counters with the plan's sizes (the cost buffer's size is among them), and the assignment's status."""
    lib = capi.load()
    K, N, dev = ei.shape[1], int(num_nodes), p.device
    rp, counters, _, edges_mask = _violated_masks(ei, p, N)
    a_slot, b_slot, a_ptr, b_ptr, cell_ptr, sizes, ws = _exact_plan(ei, p, N, edges_mask)
    rate, (F, n_a, n_b, max_side, cells, _) = _read_counters_and_sizes(counters, sizes, N)
    if F == 0:   # nothing violated: the rounded scores
        return rp, rate
    refusal = None
    if max_side > assignment.MAX_SIDE:
        refusal = "a component of %d rows or columns (at most %d)" % (max_side, assignment.MAX_SIDE)
    elif lib.mpnhip_lsa_workspace_bytes(n_a, n_b, F) == 0 or cells >= 1 << 31:
        refusal = "%d components with %d cells (at most 65535 components, fewer than 2^31 cells)" % (F, cells)
    if refusal:
        raise MpnhipError("exact_round(solver='device'): the violated sub-problem has %s; use a host solver (solver=None: pulp or "
                          "scipy, or solver=projectors.solve_with_scipy)" % refusal)
    cost = torch.empty(cells, dtype=torch.float64, device=dev)
    check(lib.mpnhip_project_exact_fill(ptr(ei), K, N, ptr(p), ptr(edges_mask), ptr(a_slot), ptr(b_slot), ptr(a_ptr), ptr(b_ptr),
                                        ptr(cell_ptr), F, n_a, n_b, ptr(cost), cells, ptr(ws), ws.numel(), stream_ptr()),
          "mpnhip_project_exact_fill")
    match_b, status = torch.empty(n_a, dtype=torch.int32, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    lsa_ws = capi.workspace(lib.mpnhip_lsa_workspace_bytes(n_a, n_b, F), dev, "lsa")
    check(lib.mpnhip_lsa_batched(ptr(cost), cells, ptr(cell_ptr), ptr(a_ptr), n_a, ptr(b_ptr), n_b, F, None, None, 0, ptr(match_b), None,
                                 ptr(status), ptr(lsa_ws), lsa_ws.numel(), stream_ptr()), "mpnhip_lsa_batched")
    out = _empty(K, torch.float32, dev)
    check(lib.mpnhip_project_exact_apply(ptr(ei), K, N, ptr(edges_mask), ptr(rp), ptr(a_slot), ptr(b_slot), ptr(match_b), n_a, ptr(out),
                                         ptr(ws), ws.numel(), stream_ptr()), "mpnhip_project_exact_apply")
    assignment.raise_on_status(status, "exact_round(solver='device')")
    return out, rate


def check_solver(solver):
    if isinstance(solver, str) and solver != DEVICE_SOLVER:
        raise ValueError("solver must be None, a callable or %r (got %r)" % (DEVICE_SOLVER, solver))


@capi.on_tensor_device
def exact_round(edge_index, edge_preds, num_nodes, solver=None):
    """``ExactProjector.project``: edges outside the violated sub-problem take the rounded value, the others the solver's
    (snapped).  Returns ``(edge_preds [K] float32 on the device, constr_satisf_rate)``.

    ``solver``: None (``default_solver()`` on the host), a callable (see ``ExactProjector``), or ``'device'``: the LP as batched
    linear assignment without leaving the device (``csrc/exact_projection.hip`` + ``mpnhip_lsa_batched``).  Where the LP's optimum
    is unique both give it; among optima of equal objective they may pick different ones.  A component of the violated
    sub-problem with more than ``assignment.MAX_SIDE`` rows or columns is refused (``MpnhipError``): there is no silent fall-back."""
    check_solver(solver)
    if solver == DEVICE_SOLVER:
        return _exact_round_device(*_edge_inputs(edge_index, edge_preds), num_nodes)
    sub = violated_subproblem(edge_index, edge_preds, num_nodes)
    out = sub.round_preds
    M = sub.edge_ids.numel()
    if M > 0:
        solve = solver if solver is not None else default_solver()
        values = snap(solve(sub.edge_index.cpu().numpy(), sub.edge_preds.cpu().numpy()))
        if values.shape[0] != M:
            raise MpnhipError("the solver returned %d values for %d edges" % (values.shape[0], M))
        out = out.clone()
        out[sub.edge_ids.long()] = torch.from_numpy(values.astype(np.float32)).to(out.device)
    return out, sub.constr_satisf_rate


class GreedyProjector:
    """Applies the greedy rounding scheme described in https://arxiv.org/pdf/1912.07515.pdf, Appendix B.1 (projectors.py:11-67)."""

    def __init__(self, full_graph):
        self.final_graph = full_graph.graph_obj
        self.num_nodes = full_graph.graph_obj.num_nodes

    def project(self):
        g = self.final_graph
        g.edge_preds, self.constr_satisf_rate = greedy_round(g.edge_index, g.edge_preds, self.num_nodes)


class ExactProjector:
    """Rounds the sub-graph of all nodes involved in a violated constraint with a min-cost-flow linear program
    (https://arxiv.org/pdf/1912.07515.pdf, Appendix B.2; projectors.py:69-113).  ``solver``: a callable ``(edge_index_sub [2, M]
    numpy, edge_preds_sub [M] numpy) -> values [M]``; None picks ``default_solver()``; ``'device'`` (or ``solver_backend='device'``)
    solves on the device (``exact_round``)."""

    def __init__(self, full_graph, solver_backend='pulp', solver=None):
        self.final_graph = full_graph.graph_obj
        self.num_nodes = full_graph.graph_obj.num_nodes
        check_solver(solver)
        self.solver_backend = solver_backend
        self.solver = solver

    def project(self):
        if self.solver_backend == 'gurobi':
            raise Exception('Uncomment gurobi code to run gorubi solver')
        g = self.final_graph
        solver = DEVICE_SOLVER if self.solver is None and self.solver_backend == DEVICE_SOLVER else self.solver
        g.edge_preds, self.constr_satisf_rate = exact_round(g.edge_index, g.edge_preds, self.num_nodes, solver=solver)
