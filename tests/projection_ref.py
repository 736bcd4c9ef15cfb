"""Numpy restatement of the path from edge scores to track ids (test infrastructure only): the flow counts and the constraint
satisfaction rate of ``compute_constr_satisfaction_rate(undirected_edges=False)``, the greedy rounding of ``GreedyProjector`` as
two passes, the violated sub-problem of ``ExactProjector``, ``connected_components(directed=False)`` labels by a min-root
union-find, and the track lengths of ``drop_short_trajectories``.  tests/test_projection_cpu.py pins it to the reference's own
outputs (tests/golden/g19_projection.npz); tests/test_gpu_projection.py uses it as the expectation for permuted and hand-made
inputs.  ``component_graphs()`` builds the hand-made graphs of the connected-components tests."""
import numpy as np


def np_flows(edge_index, edge_preds, num_nodes):
    """``(round_preds [K] float32, flow_out [N], flow_in [N], violated_out, violated_in, num_constraints)``."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    p = np.asarray(edge_preds, np.float32)
    with np.errstate(invalid="ignore"):
        active = p > np.float32(0.5)
    flow_out = np.bincount(ei[0][active], minlength=num_nodes).astype(np.int64)
    flow_in = np.bincount(ei[1][active], minlength=num_nodes).astype(np.int64)
    num_constraints = int(np.unique(ei[0]).size + np.unique(ei[1]).size)
    return active.astype(np.float32), flow_out, flow_in, int((flow_out > 1).sum()), int((flow_in > 1).sum()), num_constraints


def np_rate(violated, num_constraints):
    """``1 - violated.float() / num_constraints`` in float32; 0 / 0 is NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(1) - np.float32(violated) / np.float32(num_constraints)


def _pass(ends, p, rp, stats=None):
    """One type of constraint: every node with more than one active edge keeps the one with the largest score (first = lowest
    edge id on a tie).  Returns how many nodes it resolved."""
    resolved = 0
    order = np.argsort(ends, kind="stable")
    bounds = np.flatnonzero(np.diff(ends[order])) + 1
    for seg in np.split(order, bounds):
        act = seg[rp[seg] == 1]          # ascending edge id: argsort is stable
        if act.size > 1:
            key = p[act]
            win = act[int(np.argmax(key))]   # np.argmax returns the first maximum
            if stats is not None and int((key == key.max()).sum()) > 1:
                stats["ties"] = stats.get("ties", 0) + 1
            rp[act] = 0
            rp[win] = 1
            resolved += 1
    return resolved


def np_greedy(edge_index, edge_preds, num_nodes, stats=None):
    """``(round_preds [K] float32 after both passes, constr_satisf_rate float32, info)``; ``info`` holds the numbers of violated
    out- and in-constraints at the start, the in-constraints pass A cleared, and the arg-maxes decided by edge id."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    p = np.asarray(edge_preds, np.float32)
    rp, _, flow_in, v_out, v_in, nc = np_flows(ei, p, num_nodes)
    info = {} if stats is None else stats
    done_out = _pass(ei[0], p, rp, info)
    assert done_out == v_out
    still = np.bincount(ei[1][rp == 1], minlength=num_nodes) > 1
    done_in = _pass(ei[1], p, rp, info)
    assert done_in == int(still.sum()) and not (still & ~(flow_in > 1)).any()
    info.update(violated_out=v_out, violated_in=v_in, cleared_by_a=v_in - done_in, ties=info.get("ties", 0))
    return rp, np_rate(v_out + v_in, nc), info


def np_violated(edge_index, edge_preds, num_nodes):
    """``(nodes_mask [N], edges_mask [K], ids of the masked edges)`` of ``ExactProjector.project``."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    _, flow_out, flow_in, _, _, _ = np_flows(ei, edge_preds, num_nodes)
    nodes = (flow_in > 1) | (flow_out > 1)
    edges = nodes[ei[0]] | nodes[ei[1]]
    return nodes, edges, np.flatnonzero(edges)


def np_labels(edge_index, edge_preds, num_nodes):
    """Component labels over the edges with ``edge_preds == 1``: union-find that links the larger root under the smaller, then the
    rank of every node's root among the roots."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    parent = np.arange(num_nodes, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for e in np.flatnonzero(np.asarray(edge_preds) == 1):
        a, b = find(int(ei[0, e])), find(int(ei[1, e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(v) for v in range(num_nodes)], dtype=np.int64)
    rank = np.cumsum(root == np.arange(num_nodes)) - 1
    return rank[root] if num_nodes else np.zeros(0, np.int64)


def np_keep(labels, min_track_len):
    labels = np.asarray(labels, np.int64)
    return np.bincount(labels, minlength=max(labels.size, 1))[labels] >= min_track_len


def component_graphs():
    """``{name: (edge_index [2, K] with row < col, edge_preds [K] float32 of 0 / 1 values, num_nodes)}``: shapes a projected graph
    never has next to the ones it has."""
    def g(pairs, n, preds=None):
        ei = np.array(pairs, dtype=np.int64).reshape(-1, 2).T.copy()
        return ei, (np.ones(ei.shape[1], np.float32) if preds is None else np.asarray(preds, np.float32)), n
    out = {}
    out["chain_descending"] = g([(i, i + 1) for i in range(198, -1, -1)], 200)
    out["star_300"] = g([(0, i) for i in range(1, 301)], 301)
    out["star_high_centre"] = g([(i, 300) for i in range(300)], 301)
    out["triangle"] = g([(0, 1), (1, 2), (0, 2)], 3)
    out["duplicate_edge"] = g([(2, 5), (2, 5), (0, 1)], 7)
    out["isolated_nodes"] = g([(1, 4), (6, 7)], 10)
    # two chains, an inactive edge between them, joined by the last edge of the list
    out["joined_by_last_edge"] = g([(0, 1), (1, 2), (5, 6), (6, 7), (3, 4), (2, 6), (2, 5)], 8, [1, 1, 1, 1, 1, 0, 1])
    out["inactive_only"] = g([(0, 1), (1, 2)], 3, [0, 0.75])
    out["single_node"] = g([], 1)
    out["no_edges"] = g([], 5)
    rng = np.random.default_rng(19)
    a, b = rng.integers(0, 3000, 2500), rng.integers(0, 3000, 2500)
    sel = a != b
    out["random_3000"] = g(np.stack((np.minimum(a, b)[sel], np.maximum(a, b)[sel]), axis=1), 3000, (rng.random(int(sel.sum())) < 0.8))
    return out
