"""mpnhip_step_metrics_graphs (csrc/loss.hip: per-graph confusion and flow-conservation counts of a block-diagonal batch, one LDS
table per block) against the numpy restatement (tests/step_metrics_ref.py, pinned on the reference's numbers by
tests/test_step_metrics_graphs_cpu.py) and against the existing single-graph entry point.  Integer counts: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_metrics_ref as R
from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.loss import step_metric_counts

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")


def single_graph_counts(logits, labels, edge_index, n):
    """The existing mpnhip_step_metrics on one graph (numpy in, numpy [8] out)."""
    lib = capi.load()
    out = torch.full((8,), -7, dtype=torch.int32, device=dev())
    E = int(edge_index.shape[1])
    if E == 0:
        buf = torch.zeros(256, dtype=torch.uint8, device=dev())   # (no edges: the entry point returns behind its memset)
        capi.check(lib.mpnhip_step_metrics(capi.ptr(buf), n, 0, None, None, capi.ptr(out), capi.stream_ptr()), "mpnhip_step_metrics")
        return out.cpu().numpy()
    g = capi.PreparedGraph(torch.from_numpy(edge_index).to(dev()), n)
    lg, y = torch.from_numpy(logits).to(dev()), torch.from_numpy(labels).to(dev())
    capi.check(lib.mpnhip_step_metrics(capi.ptr(g.buf), g.N, g.E, capi.ptr(lg), capi.ptr(y), capi.ptr(out), capi.stream_ptr()),
               "mpnhip_step_metrics")
    return out.cpu().numpy()


def three_graph_batch():
    """Graph 0: 40 nodes, 240 edges and one self loop; graph 1: 5 nodes, no edge; graph 2: 28 nodes, 160 edges.  Logits with exact
    zeros, labels in {0, 1} with one 0.5."""
    a, b = synth.make_graph(40, 240, T=6, seed=3, node_in_dim=4), synth.make_graph(28, 160, T=5, seed=4, node_in_dim=4)
    ei_a = np.concatenate([a["edge_index"], np.array([[7], [7]], np.int64)], axis=1)
    graphs = [(ei_a, 40), (np.zeros((2, 0), np.int64), 5), (b["edge_index"], 28)]
    off, eis, eg, ng = 0, [], [], []
    for i, (ei, n) in enumerate(graphs):
        eis.append(ei + off)
        eg.append(np.full(ei.shape[1], i, np.int32))
        ng.append(np.full(n, i, np.int32))
        off += n
    ei, eg, ng = np.concatenate(eis, axis=1), np.concatenate(eg), np.concatenate(ng)
    E = ei.shape[1]
    logits = synth.normal(21, (E,), stream=0)
    logits[::9] = 0.0
    logits[240] = 1.5                                                # (the self loop is predicted)
    labels = (synth.uniform01(22, E) < 0.25).astype(np.float32)
    labels[5] = 0.5
    return graphs, ei, eg, ng, off, logits, labels


def device_counts(logits, labels, ei, n, eg, ng, k, guard=False):
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev())
    if not guard:
        return step_metric_counts(t(logits), t(labels), t(ei), n, edge_graph=t(eg), node_graph=t(ng), n_graphs=k).cpu().numpy()
    buf = torch.full((8 * k + 32,), 0x5A5A5A5, dtype=torch.int32, device=dev())
    out = buf[16:16 + 8 * k].view(k, 8)
    got = step_metric_counts(t(logits), t(labels), t(ei), n, edge_graph=t(eg), node_graph=t(ng), n_graphs=k, out=out)
    assert got.data_ptr() == out.data_ptr()
    h = buf.cpu().numpy()
    assert (h[:16] == 0x5A5A5A5).all() and (h[16 + 8 * k:] == 0x5A5A5A5).all(), "guard words around counts were written"
    return h[16:16 + 8 * k].reshape(k, 8)


def test_three_graph_batch_is_exact():
    graphs, ei, eg, ng, n, logits, labels = three_graph_batch()
    want = R.graph_counts(logits, labels, ei, n, eg, ng, 3)
    got = device_counts(logits, labels, ei, n, eg, ng, 3, guard=True)
    assert np.array_equal(got, want), (got, want)
    assert want[1].tolist() == [0] * 8 and want[0, 6] > 0 and want[:, 4:6].sum() > 0      # the fixture exercises what it should
    assert want[:, :4].sum() == ei.shape[1] - 1                                           # (the 0.5 label is in no cell)
    # column sums = the existing entry point on the whole batch; each row = the existing entry point on that graph alone
    assert np.array_equal(got.sum(axis=0), single_graph_counts(logits, labels, ei, n))
    e0 = n0 = 0
    for i, (gei, gn) in enumerate(graphs):
        e1 = e0 + gei.shape[1]
        assert np.array_equal(got[i], single_graph_counts(logits[e0:e1], labels[e0:e1], gei, gn)), i
        e0, n0 = e1, n0 + gn
    # one graph, NULL ids: the existing entry point
    one = device_counts(logits, labels, ei, n, None, None, 1, guard=True)
    assert np.array_equal(one[0], single_graph_counts(logits, labels, ei, n))


def test_out_of_range_ids_count_nowhere_and_write_nowhere():
    graphs, ei, eg, ng, n, logits, labels = three_graph_batch()
    eg2, ng2 = eg.copy(), ng.copy()
    eg2[3], ng2[50] = 3, 3          # = n_graphs
    eg2[300], ng2[2] = -1, -5
    want = R.graph_counts(logits, labels, ei, n, eg2, ng2, 3)
    got = device_counts(logits, labels, ei, n, eg2, ng2, 3, guard=True)
    assert np.array_equal(got, want)
    full = R.graph_counts(logits, labels, ei, n, eg, ng, 3)
    assert got[:, :4].sum() == full[:, :4].sum() - 2 and (got <= full).all() and np.array_equal(got[1], full[1])


def test_argument_refusals():
    lib = capi.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev())
    out = torch.zeros(8, dtype=torch.int32, device=dev())
    p = capi.ptr(buf)
    for k in (1025, 0, -1):
        assert lib.mpnhip_step_metrics_graphs(p, 4, 8, p, p, p, p, k, capi.ptr(out), capi.stream_ptr()) == -1, k   # MPNHIP_ERR_ARG
        assert b"step_metrics_graphs" in lib.mpnhip_last_error()
    assert lib.mpnhip_step_metrics_graphs(p, 4, 8, p, p, None, None, 2, capi.ptr(out), capi.stream_ptr()) == -1      # ids needed
    assert lib.mpnhip_step_metrics_graphs(p, 4, 8, p, p, p, p, 2, None, capi.stream_ptr()) == -1
    assert lib.mpnhip_step_metrics_graphs(None, 4, 8, p, p, p, p, 2, capi.ptr(out), capi.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0


def test_1024_graphs_fill_the_whole_lds_table():
    """1024 graphs of 3 nodes and 3 stored pairs each (a triangle): a block of 256 edges spans 43 graphs, the table is the full
    16 KB."""
    K = 1024
    base = np.array([[0, 1, 0, 2, 1, 2], [1, 0, 2, 0, 2, 1]], np.int64)
    ei = np.concatenate([base + 3 * g for g in range(K)], axis=1)
    eg = np.repeat(np.arange(K, dtype=np.int32), 6)
    ng = np.repeat(np.arange(K, dtype=np.int32), 3)
    E, n = ei.shape[1], 3 * K
    logits = synth.normal(31, (E,), stream=0)
    labels = (synth.uniform01(32, E) < 0.4).astype(np.float32)
    want = R.graph_counts(logits, labels, ei, n, eg, ng, K)
    got = device_counts(logits, labels, ei, n, eg, ng, K, guard=True)
    assert np.array_equal(got, want)
    assert np.array_equal(got.sum(axis=0), single_graph_counts(logits, labels, ei, n))
    for g in (0, 511, 1023):
        assert np.array_equal(got[g], single_graph_counts(logits[6 * g:6 * g + 6], labels[6 * g:6 * g + 6], base, 3)), g
    assert (got[:, 6] == 2).all() and (got[:, 7] == 2).all() and got[:, 4:6].sum() > 0
