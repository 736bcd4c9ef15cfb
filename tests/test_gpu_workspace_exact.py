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
operator refuses below is read from its own refusal message and must not exceed the advertised one.

The message-passing core (csrc/plan.h, backward_plan.h: ``mpnhip_forward`` / ``mpnhip_backward``) under the same discipline, at the
smallest shapes at which each class of region exists -- fp32 / 32-d / max / 3 steps (ARG, the unfused-width slabs), fp32_split / 64-d /
mean / 4 steps (four steps fork the side stream: slab_side, slab_wp, slab_tail, the node-chain images) and bf16 / 64-d / sum / 4
steps (the bf16 dZ blocks, dEpp, dP16 / dZn16 / AGG16 / enc16, wt_keep16, the backward pair images).  The layout is a function of
the dims, not of the buffer, and the kernels sum in a fixed order: logits and EVERY gradient must be BITWISE those of the package's
own path (``model.hot_path`` + autograd, roomy cached buffers) on the same inputs.  Two cases reuse inputs the suite checks against
the CPU oracle (tests/test_gpu_backward.py::test_structure_graph, tests/test_gpu_split.py::test_split_gradients_match_oracle)
and are held to the same bounds.  The small operators with a workspace (meta layer, MLP, weight gradients, BatchNorm / dropout)
follow, against plain numpy / float64 torch at the bounds of tests/test_gpu_wgrad.py and tests/test_gpu_modular.py."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import full_masks_ref as FM
import projection_ref as PR
import segment_ref as SR
import training_targets_ref as TT
from mpntrackseg_amd import capi, synth
from oracle import tracker_oracle as T
from pinned import forward_decisions
from test_gpu_backward import check_against_oracle, make_model, native_grads
from test_gpu_split import small_batch
from test_tracker_tail_cpu import np_merge, np_prune, same_bits

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WORKSPACE = -1, -3   # include/mpnhip.h
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


def exact_call(name, advertised, call, outputs, own_threshold=False, ws=None, refusal=None, offset=0):
    """``call(workspace pointer, workspace_bytes) -> status``.  Returns the workspace (a later call may read what this one left).
    ``refusal``: (status, message) of an operator that does not answer a short workspace with MPNHIP_ERR_WORKSPACE and the two
    numbers; ``offset``: hand the operator ``workspace + offset`` (one that accepts unaligned buffers) -- still ``advertised`` bytes."""
    lib = capi.load()
    assert advertised > 0, name
    need = advertised
    if ws is None:
        ws = torch.full((offset + advertised + GUARD,), FILL, dtype=torch.uint8, device=dev())
    assert ws.data_ptr() % 256 == 0
    ws = ws[offset:]
    snapshot = [ws.clone()] + [o.clone() for o in outputs]
    if own_threshold:
        assert call(capi.ptr(ws), 0) == ERR_WORKSPACE, name
        need = int(re.search(rb": workspace 0 < (\d+)", lib.mpnhip_last_error()).group(1))
        assert 0 < need <= advertised, (name, need, advertised)
    status, message = refusal or (ERR_WORKSPACE, "%s: workspace %d < %d" % (name, need - 1, need))
    assert call(capi.ptr(ws), need - 1) == status, name
    assert message.encode() in lib.mpnhip_last_error()
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


# ------------------------------------------------------------------------------------------------ the message-passing core
CORE = {"fp32": (32, 3, "max", "fp32"), "fp32_split": (64, 4, "mean", "fp32_split"), "bf16": (64, 4, "sum", "bf16")}


def core_case(case, n, steps=None):
    d, L, agg, precision = CORE[case]
    params = synth.model_params(d, L if steps is None else steps, agg, node_in_dim=48)
    model = make_model(params, synth.make_weights(params, seed=14))
    model.gemm_precision = precision
    return model, synth.make_graph(n, E, T=6, seed=30 + n, node_in_dim=48)


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), "%s differs from the package's path" % what


def core_exact_run(model, g, r, device=None, decisions=True):
    """Training forward and backward through the C ABI, each in exactly its advertised workspace, and the same through the
    package's own path: bitwise equal.  Signature and results of pinned.hip_run.
    What this can NOT show: an interior region running into the next one (say slab_wp into slab_tail) corrupts both paths alike,
    since they share the layout -- that is caught by the guard behind the last region, by the oracle cases (fp32 and split; the
    bf16 case has none here) and by tools/diag/workspace_sizes.py against a known-good build, not by the bitwise comparison."""
    lib = capi.load()
    x, ei, ea, gl = on(g["x"]), on(g["edge_index"]), on(g["edge_attr"]), on(r)
    n, e, L = x.shape[0], ea.shape[0], max(int(model.num_enc_steps), 1)
    pg = capi.PreparedGraph(ei, n, validate=True)
    params = model.hot_path_parameters()
    grads = {id(p): torch.zeros_like(p) for p in params}   # (the backward adds into them)
    keep = []
    m = model.c_model(keep, grads=grads, n_edges=e)
    logits, gx, gea = filled((L, e), torch.float32), filled(tuple(x.shape), torch.float32), filled(tuple(ea.shape), torch.float32)
    capi.path_counters(reset=True)
    fneed, bneed = lib.mpnhip_forward_workspace_bytes(m, n, e, 1), lib.mpnhip_backward_workspace_bytes(m, n, e)
    fws = exact_call("forward", fneed,
                     lambda w, b: lib.mpnhip_forward(m, capi.ptr(pg.buf), n, e, capi.ptr(x), capi.ptr(ea), capi.ptr(logits), None, None, w, b, 1,
                                                     capi.stream_ptr()), [logits])
    given = forward_decisions(model, pg, fws[:fneed]) if decisions else None
    outputs = [gx, gea] + list(grads.values())

    def backward(w, b, fwd_bytes=fneed):
        return lib.mpnhip_backward(m, capi.ptr(pg.buf), n, e, capi.ptr(x), capi.ptr(ea), capi.ptr(gl), None, None, capi.ptr(gx), capi.ptr(gea),
                                   capi.ptr(fws), fwd_bytes, w, b, capi.stream_ptr())
    # a forward workspace one byte short is refused first, whatever the backward's own buffer
    bws = torch.full((bneed + GUARD,), FILL, dtype=torch.uint8, device=dev())
    snapshot = [t.clone() for t in [fws, bws] + outputs]
    assert backward(capi.ptr(bws), bneed, fwd_bytes=fneed - 1) == ERR_WORKSPACE
    assert lib.mpnhip_last_error() == b"backward: forward workspace %d < %d (must be the save_for_backward buffer)" % (fneed - 1, fneed)
    torch.cuda.synchronize()
    for t, s in zip([fws, bws] + outputs, snapshot):
        assert torch.equal(t.view(torch.uint8), s.view(torch.uint8))
    exact_call("backward", bneed, backward, outputs, ws=bws)
    assert bool((fws[fneed:] == FILL).all()), "backward: wrote past the forward workspace"
    counts = capi.path_counters(reset=True)
    names = {id(p): k for k, p in model.named_parameters()}
    out = {names[i]: t.double().cpu().numpy() for i, t in grads.items()}
    out["grad_x"], out["grad_edge_attr"] = gx.double().cpu().numpy(), gea.double().cpu().numpy()
    lo, px, pea, ppg = native_grads(model, g["x"], g["edge_index"], g["edge_attr"], r)
    same_bytes(logits.cpu().numpy(), lo, "logits")
    same_bytes(gx.cpu().numpy(), px, "grad_x")
    same_bytes(gea.cpu().numpy(), pea, "grad_edge_attr")
    for i, t in grads.items():
        same_bytes(t.cpu().numpy(), ppg[names[i]], names[i])
    return logits.double().cpu().numpy(), out, given, counts


@pytest.mark.parametrize("n", NODES)
@pytest.mark.parametrize("case", list(CORE))
def test_core_forward_backward(case, n):
    model, g = core_case(case, n)
    L = int(model.num_enc_steps)
    _, grads, _, counts = core_exact_run(model, g, synth.normal(12, (L, E)), decisions=False)
    assert all(np.isfinite(v).all() for v in grads.values()) and all(np.abs(v).max() > 0 for v in grads.values())
    keep = []
    assert capi.load().mpnhip_backward_uses_side_stream(model.c_model(keep)) == (1 if L >= 4 else 0)
    print({k: v for k, v in counts.items() if v})
    # the kernels whose regions the case is here for ran
    if case == "fp32_split":
        assert counts["edge_chain_bwd_split"] == L and counts["gemm_tn_panel"] > 0 and counts["node_chain"] == L, counts
    elif case == "bf16":   # (chain_bf16_train_ok: the fused bf16 kernels in both directions)
        assert counts["edge_chain_fwd_bf16"] == L and counts["edge_chain_bwd_bf16"] == L, counts


def test_core_structure_graph_matches_oracle(golden):
    """The inputs of tests/test_gpu_backward.py::test_structure_graph[max], at its bound; and, max being piecewise, the decision-pinned
    comparison of tests/test_gpu_pinned.py."""
    z = golden("g4_structure.npz")
    params = synth.model_params(32, 3, "max", node_in_dim=64)
    g = {"x": z["x"], "edge_index": z["edge_index"], "edge_attr": z["edge_attr"]}
    W = synth.make_weights(params, seed=8)
    check_against_oracle(params, W, g, run=core_exact_run)
    check_against_oracle(params, W, g, robust=True, run=core_exact_run)


def test_core_split_batch_matches_oracle():
    """The inputs of tests/test_gpu_split.py::test_split_gradients_match_oracle[64-True-mean], at its bound."""
    g = small_batch(170)
    params = synth.model_params(64, 3, "mean", node_in_dim=48)
    check_against_oracle(params, synth.make_weights(params, seed=13), g, precision="fp32_split", run=core_exact_run)


@pytest.mark.parametrize("n", NODES)
@pytest.mark.parametrize("case", list(CORE))
def test_core_forward_only(case, n):
    """Inference (save 0) at the model's steps, and a model of zero steps with and without saving: logits and final features bitwise
    those of the package's inference path."""
    lib = capi.load()
    for steps, save in ((None, 0), (0, 0), (0, 1)):
        model, g = core_case(case, n, steps)
        model.eval()
        x, ei, ea = on(g["x"]), on(g["edge_index"]), on(g["edge_attr"])
        L = max(int(model.num_enc_steps), 1)
        pg = capi.PreparedGraph(ei, n, validate=True, full=bool(save))
        keep = []
        m = model.c_model(keep, n_edges=E)
        logits, xo, eo = filled((L, E), torch.float32), filled((n, m.dn), torch.float32), filled((E, m.de), torch.float32)
        exact_call("forward", lib.mpnhip_forward_workspace_bytes(m, n, E, save),
                   lambda w, b: lib.mpnhip_forward(m, capi.ptr(pg.buf), n, E, capi.ptr(x), capi.ptr(ea), capi.ptr(logits), capi.ptr(xo), capi.ptr(eo),
                                                   w, b, save, capi.stream_ptr()), [logits, xo, eo])
        with torch.no_grad():
            want = model.hot_path(x, ei, ea, return_state=True)   # (the inference path; saving changes no value)
        for got, ref, what in zip((logits, xo, eo), want, ("logits", "x_out", "e_out")):
            same_bytes(got.cpu().numpy(), ref.cpu().numpy(), "%s (steps %s, save %d)" % (what, steps, save))


# ------------------------------------------------------------------------------------------------ the small operators
@pytest.mark.parametrize("n", NODES)
def test_meta_layer(n):
    """One MetaLayer step (mpn.py:33-54) against the float64 oracle at the activations' bound of tests/test_gpu_modular.py (1e-4)."""
    from oracle import mpn_oracle as O
    lib = capi.load()
    params = synth.model_params(32, 1, "mean", node_in_dim=48)
    W = synth.make_weights(params, seed=15)
    model = make_model(params, W).eval()
    ei = synth.make_graph(n, E, T=6, seed=40 + n, node_in_dim=48)["edge_index"]
    x, e = synth.normal(16, (n, 64)), synth.normal(17, (E, 32))   # [initial | current] features: both re-attached
    keep = []
    m = model.MPNet.core_struct(keep)
    m.reattach_nodes = m.reattach_edges = 1
    pg = capi.PreparedGraph(on(ei), n, validate=True)
    x_d, e_d, x_new, e_new = on(x), on(e), filled((n, 32), torch.float32), filled((E, 16), torch.float32)
    exact_call("meta_layer", lib.mpnhip_meta_layer_workspace_bytes(m, n, E),
               lambda w, b: lib.mpnhip_meta_layer_forward(m, capi.ptr(pg.buf), n, E, capi.ptr(x_d), capi.ptr(e_d), capi.ptr(x_new), capi.ptr(e_new), w, b,
                                                          capi.stream_ptr()), [x_new, e_new])
    W64 = {k: torch.from_numpy(v).double() for k, v in W.items()}
    xr, er = O.meta_layer(torch.from_numpy(x).double(), torch.from_numpy(ei), torch.from_numpy(e).double(), W64, "mean")
    for got, ref in ((x_new, xr), (e_new, er)):
        assert float((got.double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max())) < 1e-4


def test_mlp_forward():
    """Three layers (two hidden activations ping-pong through the workspace), 65 rows; a single layer needs no workspace at all."""
    lib = capi.load()
    rows, dims = 65, [6, 18, 18, 16]
    ws_ = [synth.normal(18, (dims[i + 1], dims[i]), stream=i, std=(2.0 / dims[i]) ** 0.5) for i in range(3)]
    bs_ = [synth.normal(19, (dims[i + 1],), stream=i, std=0.1) for i in range(3)]
    x = synth.normal(20, (rows, dims[0]))
    tensors = [(on(w), on(b)) for w, b in zip(ws_, bs_)]
    mlp = capi.fill_mlp(capi.Mlp(), tensors)
    x_d, y = on(x), filled((rows, dims[-1]), torch.float32)
    exact_call("mlp_forward", lib.mpnhip_mlp_workspace_bytes(mlp, rows),
               lambda w, b: lib.mpnhip_mlp_forward(mlp, capi.ptr(x_d), capi.ptr(y), rows, w, b, capi.stream_ptr()), [y])
    ref = x.astype(np.float64)
    for w, b in zip(ws_, bs_):
        ref = np.maximum(ref @ w.astype(np.float64).T + b, 0.0)
    assert np.abs(y.cpu().numpy() - ref).max() / max(1.0, np.abs(ref).max()) < 1e-4
    one = capi.fill_mlp(capi.Mlp(), tensors[:1])
    y1 = filled((rows, dims[1]), torch.float32)
    capi.check(lib.mpnhip_mlp_forward(one, capi.ptr(x_d), capi.ptr(y1), rows, None, 0, capi.stream_ptr()), "mlp_forward")
    torch.cuda.synchronize()
    ref1 = np.maximum(x.astype(np.float64) @ ws_[0].astype(np.float64).T + bs_[0], 0.0)
    assert np.abs(y1.cpu().numpy() - ref1).max() / max(1.0, np.abs(ref1).max()) < 1e-4


@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("rows16", [False, True], ids=["weight_grad", "weight_grad_bf16_rows"])
def test_weight_grad(rows16, offset):
    """300 rows, [64 x 48], two batches; the operator rounds its workspace pointer up to 256 itself (offset 16); bound of
    tests/test_gpu_wgrad.py (3e-6 of the largest entry).  No rows: nothing to do, no workspace asked for."""
    lib = capi.load()
    rows, n_out, k_in, nb = 300, 64, 48, 2
    dz, h = on(synth.normal(21, (nb, rows, n_out))), on(synth.normal(22, (nb, rows, k_in)))
    if rows16:
        dz, h = dz.bfloat16(), h.bfloat16()
    gw, gb = torch.full((n_out, k_in), 0.25, device=dev()), torch.full((n_out,), -0.5, device=dev())   # "+=" into existing values
    name = "weight_grad_bf16_rows" if rows16 else "weight_grad"
    fn, size = getattr(lib, "mpnhip_" + name), getattr(lib, "mpnhip_%s_workspace_bytes" % name)
    assert fn(None, None, 0, n_out, k_in, nb, capi.ptr(gw), capi.ptr(gb), None, 0, capi.stream_ptr()) == 0
    exact_call(name, size(n_out, k_in, rows, nb),
               lambda w, b: fn(capi.ptr(dz), capi.ptr(h), rows, n_out, k_in, nb, capi.ptr(gw), capi.ptr(gb), w, b, capi.stream_ptr()), [gw, gb],
               offset=offset)
    ref, refb = torch.einsum("bmo,bmc->oc", dz.double(), h.double()), dz.double().sum((0, 1))
    assert float((gw.double() - 0.25 - ref).abs().max()) / float(ref.abs().max()) < 3e-6
    assert float((gb.double() + 0.5 - refb).abs().max()) / float(refb.abs().max()) < 3e-6


def test_bn_relu_dropout():
    """300 x 20, BatchNorm1d (training) + ReLU against float64 torch at the bounds of tests/test_gpu_modular.py: activations 1e-4,
    gradients 2e-4, running statistics 1e-5.  A short workspace is a bad ARGUMENT to these two (MPNHIP_ERR_ARG)."""
    lib = capi.load()
    m, n, eps, momentum = 300, 20, 1e-5, 0.1
    z, dy = synth.normal(23, (m, n)), synth.normal(24, (m, n))
    gamma, beta = 1.0 + 0.3 * synth.normal(25, (n,)), 0.2 * synth.normal(26, (n,))
    bn = torch.nn.BatchNorm1d(n, eps=eps, momentum=momentum).double().train()
    bn.weight.data, bn.bias.data = torch.from_numpy(gamma).double(), torch.from_numpy(beta).double()
    zr = torch.from_numpy(z).double().requires_grad_(True)
    yr = torch.relu(bn(zr))
    (yr * torch.from_numpy(dy).double()).sum().backward()
    z_d, dy_d, g_d, b_d = on(z), on(dy), on(gamma), on(beta)
    rm, rv = torch.zeros(n, device=dev()), torch.ones(n, device=dev())
    y, mean, invstd = filled((m, n), torch.float32), filled((n,), torch.float32), filled((n,), torch.float32)
    need = lib.mpnhip_bn_dropout_workspace_bytes(m, n)

    def rel(a, b):
        return float((a.double().cpu() - b.detach()).abs().max()) / max(1.0, float(b.detach().abs().max()))
    exact_call("bn_relu_dropout_forward", need,
               lambda w, b: lib.mpnhip_bn_relu_dropout_forward(capi.ptr(z_d), m, n, 1, capi.ptr(g_d), capi.ptr(b_d), capi.ptr(rm), capi.ptr(rv), momentum,
                                                               eps, 1, 0.0, 0, capi.ptr(y), capi.ptr(mean), capi.ptr(invstd), w, b, capi.stream_ptr()),
               [y, mean, invstd, rm, rv], refusal=(ERR_ARG, "bn_relu_dropout_forward: workspace too small"))
    assert rel(y, yr) < 1e-4 and rel(rm, bn.running_mean) < 1e-5 and rel(rv, bn.running_var) < 1e-5
    dz, dg, db = filled((m, n), torch.float32), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    exact_call("bn_relu_dropout_backward", need,
               lambda w, b: lib.mpnhip_bn_relu_dropout_backward(capi.ptr(dy_d), capi.ptr(z_d), m, n, 1, capi.ptr(g_d), capi.ptr(b_d), capi.ptr(mean),
                                                                capi.ptr(invstd), 1, 0.0, 0, capi.ptr(dz), capi.ptr(dg), capi.ptr(db), w, b,
                                                                capi.stream_ptr()),
               [dz, dg, db], refusal=(ERR_ARG, "bn_relu_dropout_backward: workspace too small"))
    assert rel(dz, zr.grad) < 2e-4 and rel(dg, bn.weight.grad) < 2e-4 and rel(db, bn.bias.grad) < 2e-4
