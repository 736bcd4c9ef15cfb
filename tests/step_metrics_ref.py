"""Numpy restatement of the per-graph step metrics (mpnhip_step_metrics_graphs), of loss.metrics_from_counts and of
train.EpochLog.summary -- written from the reference's definitions (utils/evaluation.py:340-437, pl_module.py:137-147), not from
the kernels: confusion counts of (logit > 0) against the 0 / 1 labels, and the flow-conservation counts of
compute_constr_satisfaction_rate with undirected edges: every stored edge (both directions of a pair are stored) is booked with
weight 1/2 as an OUTGOING edge of its smaller endpoint and as an INCOMING edge of its larger one."""
import numpy as np

NAMES = ("tp", "fp", "tn", "fn", "viol_out", "viol_in", "constr_out", "constr_in")


def flows(logits, edge_index, num_nodes):
    """(flow_out [N], flow_in [N], deg_out [N], deg_in [N]): predicted flow and stored-edge count per node."""
    pred = (np.asarray(logits, np.float32).reshape(-1) > 0).astype(np.float64)
    row, col = np.asarray(edge_index)[0], np.asarray(edge_index)[1]
    lo, hi = np.minimum(row, col), np.maximum(row, col)
    f_out = 0.5 * np.bincount(lo, weights=pred, minlength=num_nodes)
    f_in = 0.5 * np.bincount(hi, weights=pred, minlength=num_nodes)
    return f_out, f_in, np.bincount(lo, minlength=num_nodes), np.bincount(hi, minlength=num_nodes)


def graph_counts(logits, labels, edge_index, num_nodes, edge_graph=None, node_graph=None, n_graphs=1):
    """int64 [n_graphs, 8] (NAMES).  Ids outside [0, n_graphs) are counted nowhere; labels other than 0 / 1 in no confusion cell."""
    z = np.asarray(logits, np.float32).reshape(-1)
    y = np.asarray(labels, np.float32).reshape(-1)
    eg = np.zeros(z.size, np.int64) if edge_graph is None else np.asarray(edge_graph, np.int64)
    ng = np.zeros(num_nodes, np.int64) if node_graph is None else np.asarray(node_graph, np.int64)
    out = np.zeros((n_graphs, 8), np.int64)
    pred = z > 0
    f_out, f_in, d_out, d_in = flows(z, edge_index, num_nodes)
    for g in range(n_graphs):
        e, n = eg == g, ng == g
        out[g, 0] = np.sum(e & pred & (y == 1))
        out[g, 1] = np.sum(e & pred & (y == 0))
        out[g, 2] = np.sum(e & ~pred & (y == 0))
        out[g, 3] = np.sum(e & ~pred & (y == 1))
        out[g, 4] = np.sum(n & (f_out > 1))
        out[g, 5] = np.sum(n & (f_in > 1))
        out[g, 6] = np.sum(n & (d_out > 0))
        out[g, 7] = np.sum(n & (d_in > 0))
    return out


def metrics(counts):
    """Per-graph accuracy / recall / precision / constr_sr (utils/evaluation.py:416-437): accuracy and constr_sr are NaN without
    edges / constraints, recall and precision 0.0 without positives."""
    out = {"accuracy": [], "recall": [], "precision": [], "constr_sr": []}
    for tp, fp, tn, fn, vo, vi, co, ci in np.asarray(counts, np.float64).reshape(-1, 8):
        tot = tp + fp + tn + fn
        out["accuracy"].append((tp + tn) / tot if tot else float("nan"))
        out["recall"].append(tp / (tp + fn) if tp + fn > 0 else 0.0)
        out["precision"].append(tp / (tp + fp) if tp + fp > 0 else 0.0)
        out["constr_sr"].append(1.0 - (vo + vi) / (co + ci) if co + ci > 0 else float("nan"))
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def _nanmean(v):
    v = np.asarray(v, np.float64)
    ok = ~np.isnan(v)
    return float(v[ok].mean()) if ok.any() else float("nan")


def epoch_mean(steps):
    """``steps``: list of (loss_tracking, loss_segmentation, counts [k, 8]) -- one entry per step of k graphs.  The mean over all the
    graphs of the epoch as pd.DataFrame(outputs).mean(axis=0) takes it with one graph per row (NaN skipped); a step's loss is the
    mean of its k graphs' losses, so it stands for k equal rows."""
    lt, ls, rows = [], [], []
    for t, s, c in steps:
        c = np.asarray(c).reshape(-1, 8)
        lt += [float(t)] * c.shape[0]
        ls += [float(s)] * c.shape[0]
        rows.append(c)
    out = {"loss": _nanmean(np.asarray(lt) + np.asarray(ls)), "loss_tracking": _nanmean(lt), "loss_segmentation": _nanmean(ls)}
    for k, v in metrics(np.concatenate(rows)).items():
        out[k] = _nanmean(v)
    return out
