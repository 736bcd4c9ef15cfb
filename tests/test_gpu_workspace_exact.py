"""Every operator that takes a workspace, called through the C ABI with EXACTLY the size its ``mpnhip_*_workspace_bytes``
function returns: one byte less is refused with MPNHIP_ERR_WORKSPACE before anything is written, the advertised size is
enough, the 4096 bytes behind it (inside the test's own allocation, filled with 0xA5) stay untouched, and the result is the
one of the existing references (tests/segment_ref.py, projection_ref.py, full_masks_ref.py, training_targets_ref.py, ``np_merge``
/ ``np_prune`` of tests/test_tracker_tail_cpu.py, the oracle's dense graph utilities, plain numpy for the tracking loss and the
compaction).  The wrappers of the package are not used: their cached buffers are larger than asked.

A layout function both sizes and carves an operator's workspace (csrc/common.h ``Carver``); a region added to one side only, or
a radix sort over one key bit too few, shows here.  Shapes: 64 and 65 nodes with the largest id present (``key_bits(n - 1)`` and
``key_bits(n)`` differ at a power of two and its successor), about 300 edges (two blocks of 256), 2 frames of 37 x 53 with 5
detections, 3 steps, 2 graphs.  The workspace itself is filled with 0xA5 as well: nothing may rely on zeros it did not write.

``mpnhip_full_masks_workspace_bytes`` is ONE size for three operators (the largest of them plus 256): there the size an
operator refuses below is read from its own refusal message and must not exceed the advertised one."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import full_masks_ref as FM
import projection_ref as PR
import segment_ref as SR
import training_targets_ref as TT
from mpntrackseg_amd import capi
from oracle import tracker_oracle as T
from test_tracker_tail_cpu import np_merge, np_prune, same_bits

pytestmark = pytest.mark.gpu

ERR_WORKSPACE = -3   # include/mpnhip.h
GUARD = 4096
FILL = 0xA5
NODES = [64, 65]
E = 300


def dev():
    return torch.device("cuda:0")


def on(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev())


def filled(shape, dtype):
    """An output no operator result looks like: every byte 0xA5."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(n, 1),), FILL, dtype=torch.uint8, device=dev())[:n].view(dtype).view(shape)


def exact_call(name, advertised, call, outputs, own_threshold=False, ws=None):
    """``call(workspace pointer, workspace_bytes) -> status``.  Returns the workspace (a later call may read what this one left)."""
    lib = capi.load()
    assert advertised > 0, name
    need = advertised
    if ws is None:
        ws = torch.full((advertised + GUARD,), FILL, dtype=torch.uint8, device=dev())
    assert ws.data_ptr() % 256 == 0
    snapshot = [ws.clone()] + [o.clone() for o in outputs]
    if own_threshold:
        assert call(capi.ptr(ws), 0) == ERR_WORKSPACE, name
        need = int(re.search(rb": workspace 0 < (\d+)", lib.mpnhip_last_error()).group(1))
        assert 0 < need <= advertised, (name, need, advertised)
    assert call(capi.ptr(ws), need - 1) == ERR_WORKSPACE, name
    assert ("%s: workspace %d < %d" % (name, need - 1, need)).encode() in lib.mpnhip_last_error()
    torch.cuda.synchronize()
    for t, s in zip([ws] + outputs, snapshot):   # refused before any launch, memset or copy
        assert torch.equal(t.view(torch.uint8), s.view(torch.uint8)), name
    capi.check(call(capi.ptr(ws), need), name)
    torch.cuda.synchronize()
    assert bool((ws[need:] == FILL).all()), name + ": wrote past the advertised size"
    return ws


def edges(n, seed, undirected=False):
    """int64 [2, E]: random end points in [0, n), node n - 1 among them; ``undirected``: row < col, no duplicate pair."""
    rng = np.random.default_rng(seed)
    if undirected:
        pairs = {(n - 2, n - 1), (0, n - 1)}
        while len(pairs) < E:
            i, j = rng.integers(0, n, 2)
            if i != j:
                pairs.add((min(i, j), max(i, j)))
        ei = np.array(sorted(pairs), np.int64).T
        return np.ascontiguousarray(ei[:, rng.permutation(E)])
    ei = rng.integers(0, n, (2, E)).astype(np.int64)
    ei[:, 0], ei[:, 1], ei[:, 2] = (n - 1, 0), (3, n - 1), (n - 1, n - 1)
    return ei


# ------------------------------------------------------------------------------------------------ graph prep
def graph_arrays(buf, n, e):
    """The int32 arrays of the prepared graph buffer: every array starts on the next 256-byte boundary."""
    h = buf.cpu().numpy()
    out, off = {}, 0
    for name, count in (("header", 8), ("perm", e), ("srow", e), ("scol", e), ("seg_ptr", 3 * n + 1), ("cperm", e), ("cseg_ptr", 3 * n + 1),
                        ("rperm", e), ("rseg_ptr", n + 1), ("cperm_all", e), ("cseg_all", n + 1)):
        out[name] = h[off:off + 4 * count].view(np.int32)
        off = (off + 4 * count + 255) // 256 * 256
    return out, off


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("n", NODES)
def test_graph_prep(n, full):
    lib = capi.load()
    ei = edges(n, 1)
    want = SR.graph_csr(ei, n)
    ei_d = on(ei)
    gbytes = lib.mpnhip_graph_bytes(n, E)
    gbuf = filled((gbytes + GUARD,), torch.uint8)
    fn = lib.mpnhip_graph_prep if full else lib.mpnhip_graph_prep_forward
    exact_call("graph_prep", lib.mpnhip_graph_prep_workspace_bytes(n, E),
               lambda w, b: fn(capi.ptr(ei_d), n, E, capi.ptr(gbuf), gbytes, w, b, capi.stream_ptr()), [gbuf])
    got, end = graph_arrays(gbuf, n, E)
    assert end == gbytes and bool((gbuf[gbytes:] == FILL).all())
    d = SR.directions(ei)
    e_out, e_in = int((d == 0).sum()), int((d == 1).sum())
    assert got["header"].tolist() == [0, e_out, e_in, E - e_out - e_in, e_out, e_out + e_in, 0, E]
    for k in ("perm", "srow", "scol", "seg_ptr") + (("cperm", "cseg_ptr", "rperm", "rseg_ptr", "cperm_all", "cseg_all") if full else ()):
        assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------ segment_reduce
def test_segment_reduce():
    """x_size = 64: the parked rows carry the key 64, one bit more than the largest segment id needs."""
    lib = capi.load()
    x_size, dim = 64, 8
    rng = np.random.default_rng(2)
    row = rng.integers(0, x_size, E).astype(np.int64)
    row[row == 17] = 18                                  # segment 17 is empty
    row[:6] = (0, 63, x_size, x_size + 7, -1, x_size)    # the first and the last segment, and four parked rows
    parked = (row < 0) | (row >= x_size)
    src = SR.exact_values(3, (E, dim))
    src[parked] = 8.0    # would win every max and move every sum
    lst, ptr, _ = SR.rows_to_csr(row, x_size)
    src_d, row_d = on(src), on(row)
    for agg in SR.AGGS:
        want, want_arg = SR.seg_reduce_seq(src, ptr, x_size, agg, list=lst)
        out, arg = filled((x_size, dim), torch.float32), filled((x_size, dim), torch.int32)
        exact_call("segment_reduce", lib.mpnhip_segment_reduce_workspace_bytes(E, x_size),
                   lambda w, b: lib.mpnhip_segment_reduce(capi.ptr(src_d), capi.ptr(row_d), E, dim, x_size, capi.AGG_CODE[agg], capi.ptr(out),
                                                          capi.ptr(arg) if agg == "max" else None, w, b, capi.stream_ptr()), [out, arg])
        got = out.cpu().numpy()
        assert np.array_equal(got, want), agg    # (exact inputs: every partial sum is exact in any order)
        assert not got[17].any()
        if agg == "max":
            assert np.array_equal(arg.cpu().numpy(), want_arg)


# ------------------------------------------------------------------------------------------------ graph build, kNN mask
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("n", NODES)
def test_time_valid_conn_count(n, directed):
    lib = capi.load()
    frame = np.sort(np.random.default_rng(4).integers(0, 12, n)).astype(np.int64)
    dist = np.abs(frame[:, None] - frame[None, :])
    ok = (dist > 0) & (dist <= 3)
    if not directed:
        ok &= np.arange(n)[:, None] < np.arange(n)[None, :]
        assert int(ok.sum()) == T.get_time_valid_conn_ixs(frame, 3).shape[1]
    want = np.concatenate(([0], np.cumsum(ok.sum(axis=1))))
    frame_d, offsets = on(frame), filled((n + 1,), torch.int64)
    fn = lib.mpnhip_time_valid_conn_directed_count if directed else lib.mpnhip_time_valid_conn_count
    exact_call("time_valid_conn", lib.mpnhip_time_valid_conn_workspace_bytes(n),
               lambda w, b: fn(capi.ptr(frame_d), n, 3, capi.ptr(offsets), w, b, capi.stream_ptr()), [offsets])
    assert np.array_equal(offsets.cpu().numpy(), want)


@pytest.mark.parametrize("symmetric", [0, 1])
@pytest.mark.parametrize("n", NODES)
def test_knn_mask(n, symmetric):
    lib = capi.load()
    rng = np.random.default_rng(5)
    pairs = edges(n, 5, undirected=True)
    d = (rng.random(E) + 0.01).astype(np.float32)
    if symmetric:
        p = rng.permutation(2 * E)
        ei, dist = np.concatenate((pairs, pairs[::-1]), axis=1)[:, p], np.concatenate((d, d))[p]
    else:
        ei, dist = pairs, d
    m = ei.shape[1]
    ei_d, dist_d = on(ei), on(dist)
    for reciprocal in (0, 1):
        want = T.get_knn_mask(torch.from_numpy(dist), torch.from_numpy(ei), n, 4, bool(reciprocal), symmetric_edges=bool(symmetric))
        mask = filled((m,), torch.uint8)
        exact_call("knn_mask", lib.mpnhip_knn_mask_workspace_bytes(m, symmetric),
                   lambda w, b: lib.mpnhip_knn_mask(capi.ptr(dist_d), capi.ptr(ei_d), n, m, 4, reciprocal, symmetric, capi.ptr(mask), w, b,
                                                    capi.stream_ptr()), [mask])
        assert np.array_equal(mask.cpu().numpy().astype(bool), want.numpy())


# ------------------------------------------------------------------------------------------------ undirected merge, pruning
@pytest.mark.parametrize("id_bits_of", ["n_nodes", "all 32"])
@pytest.mark.parametrize("n", NODES)
def test_undirected_merge_and_prune(n, id_bits_of):
    """The fill reads what the sort left at the head of the SAME workspace; n_nodes = 0 sorts all 32 id bits."""
    lib = capi.load()
    rng = np.random.default_rng(6)
    pairs = edges(n, 6, undirected=True)[:, :E // 2]
    pairs[:, 1] = (n - 2, n - 1)
    ei = np.concatenate((pairs, pairs[::-1]), axis=1)
    ei[:, -1] = ei[:, 0]   # a pair with three copies, another with one
    ei = np.ascontiguousarray(ei[:, rng.permutation(E)])
    attr = rng.random(E).astype(np.float32)
    ei_u, (attr_u,), inv = np_merge(ei, [attr])
    u = ei_u.shape[1]
    ei_d, attr_d = on(ei), on(attr)
    inverse, n_unique = filled((E,), torch.int32), filled((1,), torch.int32)
    need = lib.mpnhip_undirected_merge_workspace_bytes(E)
    ws = exact_call("undirected_merge_sort", need,
                    lambda w, b: lib.mpnhip_undirected_merge_sort(capi.ptr(ei_d), E, n if id_bits_of == "n_nodes" else 0, capi.ptr(inverse),
                                                                  capi.ptr(n_unique), w, b, capi.stream_ptr()), [inverse, n_unique])
    assert int(n_unique[0]) == u and np.array_equal(inverse.cpu().numpy(), inv)
    got_ei, got_attr = filled((2, u), torch.int64), filled((u,), torch.float32)
    exact_call("undirected_merge_fill", need,
               lambda w, b: lib.mpnhip_undirected_merge_fill(E, u, w, b, capi.ptr(got_ei), capi.ptr(attr_d), capi.ptr(got_attr), capi.stream_ptr()),
               [got_ei, got_attr], ws=ws)
    assert np.array_equal(got_ei.cpu().numpy(), ei_u) and same_bits(got_attr.cpu().numpy(), attr_u)
    # to_lightweight_graph: threshold (no workspace), then the compaction
    _, _, kept = np_prune(ei_u, attr_u, 0.5)
    flags, ids, count = filled((u,), torch.uint8), filled((u,), torch.int32), filled((1,), torch.int32)
    capi.check(lib.mpnhip_threshold_flags(capi.ptr(got_attr), u, 0.5, capi.ptr(flags), capi.stream_ptr()), "threshold_flags")
    exact_call("compact", lib.mpnhip_compact_workspace_bytes(u),
               lambda w, b: lib.mpnhip_compact(capi.ptr(flags), u, capi.ptr(ids), capi.ptr(count), w, b, capi.stream_ptr()), [ids, count])
    assert 0 < kept.size < u and int(count[0]) == kept.size and np.array_equal(ids.cpu().numpy()[:kept.size], kept)


# ------------------------------------------------------------------------------------------------ projection
@pytest.mark.parametrize("n", NODES)
def test_projection(n):
    lib = capi.load()
    ei = edges(n, 7, undirected=True)
    preds = np.random.default_rng(7).random(E).astype(np.float32)
    preds[:40] = np.float32(0.99)   # ties: the lowest edge id wins
    ei_d, preds_d = on(ei), on(preds)
    rp_want, fo, fi, v_out, v_in, nc = PR.np_flows(ei, preds, n)
    rp, flow_out, flow_in, counters = filled((E,), torch.float32), filled((n,), torch.int32), filled((n,), torch.int32), filled((8,), torch.int32)
    exact_call("project_round_count", lib.mpnhip_project_round_count_workspace_bytes(n),
               lambda w, b: lib.mpnhip_project_round_count(capi.ptr(ei_d), E, n, capi.ptr(preds_d), capi.ptr(rp), capi.ptr(flow_out),
                                                           capi.ptr(flow_in), capi.ptr(counters), w, b, capi.stream_ptr()),
               [rp, flow_out, flow_in, counters])
    assert np.array_equal(rp.cpu().numpy(), rp_want)
    assert np.array_equal(flow_out.cpu().numpy(), fo) and np.array_equal(flow_in.cpu().numpy(), fi)
    assert counters.cpu().numpy()[:4].tolist() == [v_out, v_in, nc, 0] and v_out > 0 and v_in > 0
    greedy_want, _, info = PR.np_greedy(ei, preds, n)
    assert info["ties"] > 0
    exact_call("project_greedy", lib.mpnhip_project_greedy_workspace_bytes(n),
               lambda w, b: lib.mpnhip_project_greedy(capi.ptr(ei_d), E, n, capi.ptr(preds_d), capi.ptr(rp), capi.ptr(flow_out), capi.ptr(flow_in),
                                                      w, b, capi.stream_ptr()), [rp])
    assert np.array_equal(rp.cpu().numpy(), greedy_want)
    want = PR.np_labels(ei, greedy_want, n)
    labels, n_comp = filled((n,), torch.int64), filled((1,), torch.int32)
    exact_call("connected_components", lib.mpnhip_connected_components_workspace_bytes(n),
               lambda w, b: lib.mpnhip_connected_components(capi.ptr(ei_d), E, n, capi.ptr(rp), capi.ptr(labels), capi.ptr(n_comp), w, b,
                                                            capi.stream_ptr()), [labels, n_comp])
    assert np.array_equal(labels.cpu().numpy(), want) and int(n_comp[0]) == int(want.max()) + 1 and 1 < int(n_comp[0]) < n


# ------------------------------------------------------------------------------------------------ full-frame masks
def test_full_masks():
    lib = capi.load()
    h, w, thr, frame_ptr = 37, 53, 0.5, [0, 3, 5]
    nd, nf = 5, 2
    rng = np.random.default_rng(8)
    masks = FM.blob_masks(rng, nd, 28, 28)
    boxes = FM.random_boxes(rng, nd, h, w, lo=8.0, hi=40.0)
    lab_want, pos_want, cnt_want = [], [], []
    for f in range(nf):
        a, b = frame_ptr[f], frame_ptr[f + 1]
        lab, _ = FM.np_frame(masks[a:b], boxes[a:b], h, w, thr)
        p, c = FM.np_events(lab, b - a)
        lab_want.append(np.where(lab >= 0, lab + a, -1).astype(np.int32))
        pos_want.append(p)
        cnt_want.append(c)
    lab_want, pos_want, cnt_want = np.stack(lab_want), np.concatenate(pos_want), np.concatenate(cnt_want)
    total = int(cnt_want.sum())
    assert total > 0 and (cnt_want > 0).sum() >= 3
    masks_d, boxes_d, fp_d = on(masks), on(boxes, np.float64), on(frame_ptr, np.int32)
    labels = filled((nf, w, h), torch.int32)
    exact_call("paste_unique_masks", lib.mpnhip_full_masks_workspace_bytes(nd, nf, h * w, 0),
               lambda ws, b: lib.mpnhip_paste_unique_masks(capi.ptr(masks_d), nd, 28, 28, capi.ptr(boxes_d), None, nd, capi.ptr(fp_d), nf, h, w, thr,
                                                           capi.ptr(labels), None, ws, b, capi.stream_ptr()), [labels], own_threshold=True)
    assert np.array_equal(labels.cpu().numpy().transpose(0, 2, 1), lab_want)
    det_counts, n_events = filled((nd,), torch.int32), filled((1,), torch.int32)
    exact_call("mask_run_events_count", lib.mpnhip_full_masks_workspace_bytes(nd, nf, h * w, 0),
               lambda ws, b: lib.mpnhip_mask_run_events_count(capi.ptr(labels), nf, h * w, nd, capi.ptr(det_counts), capi.ptr(n_events), ws, b,
                                                              capi.stream_ptr()), [det_counts, n_events], own_threshold=True)
    assert int(n_events[0]) == total and np.array_equal(det_counts.cpu().numpy(), cnt_want)
    pos = filled((total,), torch.int32)
    exact_call("mask_run_events", lib.mpnhip_full_masks_workspace_bytes(nd, nf, h * w, total),
               lambda ws, b: lib.mpnhip_mask_run_events(capi.ptr(labels), nf, h * w, nd, total, capi.ptr(pos), ws, b, capi.stream_ptr()),
               [pos], own_threshold=True)
    assert np.array_equal(pos.cpu().numpy(), pos_want)


# ------------------------------------------------------------------------------------------------ training targets
@pytest.mark.parametrize("n", NODES)
def test_edge_labels_closest(n):
    lib = capi.load()
    ei = edges(n, 9)
    ids = np.random.default_rng(9).integers(-1, 6, n).astype(np.int64)
    ids[n - 1] = ids[0] = 2
    want = TT.edge_labels(ei, ids, "closest")
    assert 0 < want.sum() < (TT.edge_labels(ei, ids, "all")).sum()
    ei_d, ids_d = on(ei), on(ids)
    labels, status = filled((E,), torch.float32), filled((1,), torch.int32)
    exact_call("edge_labels", lib.mpnhip_edge_labels_workspace_bytes(n),
               lambda w, b: lib.mpnhip_edge_labels(capi.ptr(ei_d), E, capi.ptr(ids_d), n, 1, capi.ptr(labels), capi.ptr(status), w, b,
                                                   capi.stream_ptr()), [labels, status])
    assert labels.cpu().numpy().tobytes() == want.tobytes() and int(status[0]) == 0


@pytest.mark.parametrize("shape", [(3, 171), (8, 320)], ids=["scalar, 2 chunks per row", "vector, 2 chunks per row"])
def test_mask_loss(shape):
    """3 steps, 2 graphs; bounds of tests/test_gpu_training_targets.py (float32 terms against float64: 1e-5 of the loss, 1e-6 of
    the largest gradient element)."""
    lib = capi.load()
    k, n, ng, weight = 3, 9, 2, 1.5
    rng = np.random.default_rng(10)
    preds = (rng.standard_normal((k, n) + shape) * 1.5).astype(np.float32)
    y = (rng.random((n,) + shape) < 0.4).astype(np.float32)
    valid = np.array([1, 0, 1, 1, 0, 1, 1, 0, 1], np.uint8)
    node_graph = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1], np.int32)
    want_lv, want_g = TT.mask_loss(list(preds), y, valid, weight, node_graph, ng)
    p = int(np.prod(shape))
    pt = [on(preds[s]) for s in range(k)]
    gt = [filled((n,) + shape, torch.float32) for _ in range(k)]
    y_d, valid_d, ng_d, loss = on(y), on(valid), on(node_graph), filled((1 + k,), torch.float32)
    pa, ga = (C.c_void_p * k)(*[t.data_ptr() for t in pt]), (C.c_void_p * k)(*[t.data_ptr() for t in gt])
    exact_call("mask_loss", lib.mpnhip_mask_loss_workspace_bytes(k, n, p, ng),
               lambda w, b: lib.mpnhip_mask_loss(pa, k, capi.ptr(y_d), capi.ptr(valid_d), capi.ptr(ng_d), ng, n, p, weight, capi.ptr(loss), ga, w, b,
                                                 capi.stream_ptr()), [loss] + gt)
    got = loss.cpu().numpy()
    for i in range(1 + k):
        assert abs(got[i] - want_lv[i]) <= 1e-5 * max(1.0, abs(want_lv[i])), (i, got[i], want_lv[i])
    for s in range(k):
        g = gt[s].cpu().numpy()
        assert np.abs(g - want_g[s]).max() <= 1e-6 * max(1.0, float(np.abs(want_g[s]).max()))
        assert not g[valid == 0].any()


def np_tracking_loss(logits, y, first_step, weight, edge_graph, n_graphs):
    """float64: per graph its own pos_weight and its own mean, the graph losses averaged (pl_module.py:88-107)."""
    z, y = logits.astype(np.float64), y.astype(np.float64)
    lv, grad = np.zeros(1 + z.shape[0]), np.zeros_like(z)
    for g in range(n_graphs):
        m = edge_graph == g
        eg, pos = float(m.sum()), float(y[m].sum())
        pw = (eg - pos) / pos if pos > 0 else 0.0
        lw = 1.0 + (pw - 1.0) * y[m]
        for s in range(first_step, z.shape[0]):
            zs = z[s, m]
            lv[1 + s] += weight * ((1.0 - y[m]) * zs + lw * (np.log1p(np.exp(-np.abs(zs))) + np.maximum(-zs, 0.0))).sum() / eg / n_graphs
            grad[s, m] = (lw / (1.0 + np.exp(-zs)) - pw * y[m]) * weight / (eg * n_graphs)
    lv[0] = lv[1:].sum()
    return lv, grad


@pytest.mark.parametrize("n_graphs", [1, 2], ids=["tracking_loss", "tracking_loss_graphs"])
def test_tracking_loss(n_graphs):
    """3 steps (the first unclassified), 2 graphs; bounds of tests/test_gpu_loss.py."""
    lib = capi.load()
    k, first, weight = 3, 1, 0.75
    rng = np.random.default_rng(11)
    logits = (rng.standard_normal((k, E)) * 2.0).astype(np.float32)
    y = (rng.random(E) < 0.2).astype(np.float32)
    edge_graph = (np.arange(E) >= 130).astype(np.int32) if n_graphs == 2 else np.zeros(E, np.int32)
    want_lv, want_g = np_tracking_loss(logits, y, first, weight, edge_graph, n_graphs)
    logits_d, y_d, eg_d = on(logits), on(y), on(edge_graph)
    loss, grad = filled((1 + k,), torch.float32), filled((k, E), torch.float32)
    if n_graphs == 1:
        exact_call("tracking_loss", lib.mpnhip_tracking_loss_workspace_bytes(k, E),
                   lambda w, b: lib.mpnhip_tracking_loss(capi.ptr(logits_d), capi.ptr(y_d), k, E, first, weight, capi.ptr(loss), capi.ptr(grad), w, b,
                                                         capi.stream_ptr()), [loss, grad])
    else:
        exact_call("tracking_loss_graphs", lib.mpnhip_tracking_loss_graphs_workspace_bytes(k, E, n_graphs),
                   lambda w, b: lib.mpnhip_tracking_loss_graphs(capi.ptr(logits_d), capi.ptr(y_d), capi.ptr(eg_d), n_graphs, k, E, first, weight,
                                                                capi.ptr(loss), capi.ptr(grad), w, b, capi.stream_ptr()), [loss, grad])
    got, g = loss.cpu().numpy(), grad.cpu().numpy()
    for i in range(1 + k):
        assert abs(got[i] - want_lv[i]) <= 1e-5 * max(1.0, abs(want_lv[i])), (i, got[i], want_lv[i])
    assert np.abs(g - want_g).max() <= 1e-6 * max(1.0, float(np.abs(want_g).max()))
    assert not g[:first].any() and got[1] == 0.0
