"""tests/step_metrics_ref.py (the numpy restatement the GPU tests of mpnhip_step_metrics_graphs compare against) pinned on the
reference's own numbers (tests/golden/g9_loss_metrics.npz: compute_perform_metrics of the imported reference, and its per-node
flows) and on a case small enough to check by hand; loss.metrics_from_counts (host code) against the same.  No GPU."""
import numpy as np
import pytest

import step_metrics_ref as R


@pytest.mark.parametrize("tag", ["m1", "m2", "m3"])
def test_restatement_matches_the_reference_metrics(golden, tag):
    z = golden("g9_loss_metrics.npz")
    ei, n = z["edge_index"], 120
    f_out, f_in, _, _ = R.flows(z[f"{tag}:logit"], ei, n)
    assert np.array_equal(f_out.astype(np.float32), z[f"{tag}:flow_out"]) and np.array_equal(f_in.astype(np.float32), z[f"{tag}:flow_in"])
    counts = R.graph_counts(z[f"{tag}:logit"], z[f"{tag}:labels"], ei, n)
    assert counts.shape == (1, 8) and counts[0, :4].sum() == ei.shape[1]
    m = R.metrics(counts)
    for i, k in enumerate(("accuracy", "recall", "precision", "constr_sr")):
        assert abs(m[k][0] - float(z[f"{tag}:metrics"][i])) < 1e-6, k
    # one graph with explicit ids is the same table; the epoch mean of one one-graph step is the step
    same = R.graph_counts(z[f"{tag}:logit"], z[f"{tag}:labels"], ei, n, np.zeros(ei.shape[1], np.int32), np.zeros(n, np.int32), 1)
    assert np.array_equal(same, counts)
    ep = R.epoch_mean([(0.5, 0.25, counts)])
    assert ep["loss"] == 0.75 and all(abs(ep[k] - float(z[f"{tag}:metrics"][i])) < 1e-6
                                      for i, k in enumerate(("accuracy", "recall", "precision", "constr_sr")))


def hand_case():
    """Graph 0: a triangle 0-1-2, both directions stored; the pairs (0,1) and (0,2) are predicted, (0,1) is the one true pair.
    Graph 1: nodes 3 and 4, no edge.  By hand: TP 2, FP 2, TN 2, FN 0; node 0 sends 2 units (a violation), node 1 sends 0, node 2
    has no outgoing edge; nodes 1 and 2 receive 1 unit each (no violation), node 0 has no incoming edge."""
    ei = np.array([[0, 1, 0, 2, 1, 2], [1, 0, 2, 0, 2, 1]], np.int64)
    logits = np.array([2.0, 0.5, 1.0, 3.0, -1.0, 0.0], np.float32)      # (a logit of exactly 0 is "not predicted")
    labels = np.array([1, 1, 0, 0, 0, 0], np.float32)
    return ei, logits, labels, np.zeros(6, np.int32), np.array([0, 0, 0, 1, 1], np.int32)


def test_hand_checked_two_graph_case_and_nan_skipping():
    ei, logits, labels, eg, ng = hand_case()
    counts = R.graph_counts(logits, labels, ei, 5, eg, ng, 2)
    assert counts.tolist() == [[2, 2, 2, 0, 1, 0, 2, 2], [0, 0, 0, 0, 0, 0, 0, 0]]
    m = R.metrics(counts)
    assert m["accuracy"][0] == 4 / 6 and np.isnan(m["accuracy"][1])
    assert m["recall"].tolist() == [1.0, 0.0] and m["precision"].tolist() == [0.5, 0.0]
    assert m["constr_sr"][0] == 0.75 and np.isnan(m["constr_sr"][1])
    # epoch: a two-graph step and a one-graph step (graph 0 again): NaN rows are skipped, losses weighted by the graphs
    ep = R.epoch_mean([(1.0, 0.5, counts), (4.0, 2.0, counts[:1])])
    assert abs(ep["loss_tracking"] - 2.0) < 1e-12 and abs(ep["loss_segmentation"] - 1.0) < 1e-12 and abs(ep["loss"] - 3.0) < 1e-12
    assert abs(ep["accuracy"] - 4 / 6) < 1e-12 and abs(ep["constr_sr"] - 0.75) < 1e-12
    assert abs(ep["recall"] - 2 / 3) < 1e-12 and abs(ep["precision"] - 1 / 3) < 1e-12
    # ids outside [0, n_graphs) are counted nowhere; a label of 0.5 in no confusion cell
    eg2, ng2, lab2 = eg.copy(), ng.copy(), labels.copy()
    eg2[0], ng2[0], lab2[2] = 2, -1, 0.5
    c2 = R.graph_counts(logits, lab2, ei, 5, eg2, ng2, 2)
    assert c2.tolist() == [[1, 1, 2, 0, 0, 0, 1, 2], [0, 0, 0, 0, 0, 0, 0, 0]]


def test_metrics_from_counts_matches_the_restatement():
    from mpntrackseg_amd.loss import METRIC_COUNT_NAMES, metrics_from_counts
    assert METRIC_COUNT_NAMES == R.NAMES
    ei, logits, labels, eg, ng = hand_case()
    counts = R.graph_counts(logits, labels, ei, 5, eg, ng, 2)
    extra = np.array([[0, 0, 3, 2, 0, 0, 1, 0], [5, 0, 0, 0, 2, 1, 2, 1]], np.int64)   # no predicted positive; everything violated
    table = np.concatenate([counts, extra]).astype(np.int32)
    got, want = metrics_from_counts(table), R.metrics(table)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == (4,) and np.array_equal(got[k], want[k], equal_nan=True), k
    assert want["recall"][2] == 0.0 and want["precision"][2] == 0.0 and want["constr_sr"][3] == 0.0
