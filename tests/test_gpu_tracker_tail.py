"""The tail of the sliding-window inference on the device: node masks, undirected merge, edge pruning, directed time-valid pairs and
``tracker.evaluate_sequence`` against the reference's ``MPNTracker._evaluate_graph_in_batches`` run to its end
(tests/golden/g17_window_tail.npz, tools/make_golden.py gen_g17) and against the numpy restatement of
tests/test_tracker_tail_cpu.py."""
import types

import numpy as np
import pytest
import torch

from mpntrackseg_amd import capi, graph as G, synth, tracker
from mpntrackseg_amd.capi import MpnhipError
from mpntrackseg_amd.mpn import MOTMPNet
from pyg_standin import Graph
from test_tracker_tail_cpu import SEQ_CASES, np_merge, np_prune, same_bits

pytestmark = pytest.mark.gpu

TOL = 2e-5   # the bound of test_gpu_tracker.py::test_sliding_window_against_reference_tracker


def dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("tag", SEQ_CASES)
def test_merge_and_prune_reproduce_the_reference_bit_for_bit(golden, tag):
    z = golden("g17_window_tail.npz")
    sq = tag[0]
    n = z[f"{sq}:frame"].shape[0]
    ei = torch.from_numpy(z[f"{sq}:edge_index"]).to(dev())
    labels = (synth.uniform01(23, ei.shape[1]) < 0.3).astype(np.float32)
    go = Graph(x=torch.from_numpy(z[f"{sq}:x"]).to(dev()), edge_index=ei, edge_attr=torch.from_numpy(z[f"{sq}:edge_attr"]).to(dev()),
               reid_emb_dists=torch.from_numpy(z[f"{sq}:reid_emb_dists"]).to(dev()),
               edge_preds=torch.from_numpy(z[f"{tag}:final_edge_preds"]).to(dev()))
    if tag.endswith("1"):
        go.edge_labels = torch.from_numpy(labels).to(dev())
    mot_graph = types.SimpleNamespace(graph_obj=go)
    inverse = G.to_undirected_graph(mot_graph)
    assert go.edge_index.dtype == torch.int64 and np.array_equal(_np(go.edge_index), z[f"{tag}:edge_index_u"])
    assert same_bits(_np(go.edge_preds), z[f"{tag}:edge_preds_u"])
    assert np.array_equal(_np(inverse).astype(np.int64), z[f"{tag}:orig_indices"])
    if tag.endswith("1"):
        assert same_bits(_np(go.edge_labels), np_merge(z[f"{sq}:edge_index"], [labels])[1][0])
    G.to_lightweight_graph(mot_graph)
    assert np.array_equal(_np(go.edge_index), z[f"{tag}:edge_index"])
    assert same_bits(_np(go.edge_preds), z[f"{tag}:edge_preds"])
    assert np.array_equal(_np(go.node_names), np.arange(n)) and go.node_names.is_cuda
    for name in ("reid_emb_dists", "x", "edge_attr", "edge_labels"):
        assert not hasattr(go, name), name


def _symmetric_list(rng, n_pairs, n_nodes, base=0):
    pairs = set()
    while len(pairs) < n_pairs:
        i, j = (int(v) for v in rng.integers(0, n_nodes, 2))
        if i != j:
            pairs.add((min(i, j) + base, max(i, j) + base))
    pr = np.array(sorted(pairs), dtype=np.int64).T.reshape(2, -1)
    ei = np.concatenate((pr, pr[::-1]), axis=1)
    return ei[:, rng.permutation(ei.shape[1])]


def _check_merge(ei, attrs, **kw):
    want_ei, want_attrs, want_inv = np_merge(ei, attrs)
    got_ei, got_attrs, got_inv = G.merge_undirected(torch.from_numpy(ei).to(dev()), [torch.from_numpy(a).to(dev()) for a in attrs], **kw)
    assert got_ei.dtype == torch.int64 and got_inv.dtype == torch.int32
    assert np.array_equal(_np(got_ei), want_ei)
    assert np.array_equal(_np(got_inv).astype(np.int64), want_inv)
    assert len(got_attrs) == len(attrs)
    for g, w in zip(got_attrs, want_attrs):
        assert same_bits(_np(g), w)
    return got_ei, got_attrs


@pytest.mark.parametrize("n_pairs,n_nodes,base", [(1, 2, 0), (500, 120, 0), (50000, 3000, 0), (700, 5000, 2 ** 31 - 1 - 5000)])
def test_merge_and_prune_random_lists(n_pairs, n_nodes, base):
    rng = np.random.default_rng(n_pairs)
    ei = _symmetric_list(rng, n_pairs, n_nodes, base)
    attrs = [rng.random(ei.shape[1]).astype(np.float32), rng.standard_normal(ei.shape[1]).astype(np.float32)]
    got_ei, got_attrs = _check_merge(ei, attrs)
    if base == 0:   # the node count as a hint: fewer sorted bits, the same result
        _check_merge(ei, attrs, num_nodes=n_nodes)
        _check_merge(ei, [], num_nodes=n_nodes)
    p = _np(got_attrs[0]).copy()
    p[::7] = np.nan
    p[1::7] = 0.5
    want = np_prune(_np(got_ei), p)
    got = G.prune_edges(got_ei, torch.from_numpy(p).to(dev()))
    assert np.array_equal(_np(got[0]), want[0]) and same_bits(_np(got[1]), want[1])
    assert np.array_equal(_np(got[2]).astype(np.int64), want[2])
    got = G.prune_edges(got_ei, torch.from_numpy(p).to(dev()), threshold=0.25)
    assert np.array_equal(_np(got[0]), np_prune(_np(got_ei), p, 0.25)[0])


def test_merge_and_prune_degenerate_lists():
    empty = torch.empty((2, 0), dtype=torch.int64, device=dev())
    ei_u, attrs, inv = G.merge_undirected(empty, [torch.empty(0, device=dev())])
    assert tuple(ei_u.shape) == (2, 0) and attrs[0].numel() == 0 and inv.numel() == 0
    ek, pk, ids = G.prune_edges(ei_u, attrs[0])
    assert tuple(ek.shape) == (2, 0) and pk.numel() == 0 and ids.numel() == 0
    rng = np.random.default_rng(3)
    ei = _symmetric_list(rng, 40, 30)
    # an unpaired edge: E is odd, or even with one pair listed in one direction only
    for bad in (ei[:, :-1], np.concatenate((ei, [[100], [101]], [[200], [201]]), axis=1)):
        with pytest.raises(MpnhipError, match="Some edges were not duplicated"):
            G.merge_undirected(torch.from_numpy(np.ascontiguousarray(bad)).to(dev()))
    # every pair listed four times: E = 4 U
    with pytest.raises(MpnhipError, match="Some edges were not duplicated"):
        G.merge_undirected(torch.from_numpy(np.concatenate((ei, ei), axis=1)).to(dev()))
    # one pair three times, another once: E = 2 U holds and the means run over the real numbers of copies, as scatter_mean's do
    odd = np.concatenate((ei, [[7, 7], [100, 100]], [[100], [7]], [[200], [201]]), axis=1)
    odd = odd[:, rng.permutation(odd.shape[1])]
    a = rng.random(odd.shape[1]).astype(np.float32)
    _, (m,) = _check_merge(odd, [a])
    want_ei, (want_m,), inv = np_merge(odd, [a])
    assert sorted(np.bincount(inv).tolist())[-1] == 3 and sorted(np.bincount(inv).tolist())[0] == 1


def test_node_mask_kernels_both_paths():
    """accumulate / average on the 16-byte path (row length 3136) and the scalar one (row length 7, odd offsets), overlapping
    windows, a node no window covers."""
    lib = capi.load()
    rng = np.random.default_rng(5)
    for row_len, n_nodes, windows in ((3136, 12, [(0, 5), (3, 9), (3, 9), (10, 12)]), (7, 9, [(0, 4), (1, 6), (5, 8)]), (8, 6, [(1, 4)])):
        overall = torch.zeros((n_nodes, row_len), device=dev())
        count = torch.zeros(n_nodes, device=dev())
        want, want_n = np.zeros((n_nodes, row_len), np.float32), np.zeros(n_nodes, np.float32)
        for (n0, n1) in windows:
            lg = (4.0 * rng.standard_normal((n1 - n0, row_len))).astype(np.float32)
            t = torch.from_numpy(lg).to(dev())
            capi.check(lib.mpnhip_node_mask_accumulate(capi.ptr(t), n1 - n0, row_len, n0, n_nodes, capi.ptr(overall), capi.ptr(count),
                                                       capi.stream_ptr()), "mpnhip_node_mask_accumulate")
            want[n0:n1] += (1.0 / (1.0 + np.exp(-lg.astype(np.float64)))).astype(np.float32)
            want_n[n0:n1] += 1
        out = torch.empty_like(overall)
        capi.check(lib.mpnhip_node_mask_average(capi.ptr(overall), capi.ptr(count), n_nodes, row_len, capi.ptr(out), capi.stream_ptr()),
                   "mpnhip_node_mask_average")
        torch.cuda.synchronize()
        assert np.array_equal(_np(count), want_n)
        # a float32 sigmoid is within a few ulp of the float64 one: 1e-6 per window
        assert float(np.abs(_np(overall) - want).max()) <= 1e-6 * len(windows)
        got = _np(out)
        seen = want_n > 0
        assert same_bits(got[seen], _np(overall)[seen] / want_n[seen, None])
        assert np.isnan(got[~seen]).all() and (~seen).any()
    # rows that would leave the accumulators are refused before any launch
    t = torch.zeros((3, 8), device=dev())
    assert lib.mpnhip_node_mask_accumulate(capi.ptr(t), 3, 8, 4, 6, capi.ptr(overall), capi.ptr(count), capi.stream_ptr()) != 0


def test_directed_time_valid_pairs(golden):
    z = golden("g17_window_tail.npz")
    f = torch.from_numpy(z["l:frame"]).to(dev())
    for name in ("tv_max", "tv_3"):
        mfd = int(z[f"{name}:max_frame_dist"])
        row, col = G.get_time_valid_conn_ixs(f, 'max' if mfd < 0 else mfd, return_undirected=False)
        assert row.dtype == torch.int64 and np.array_equal(_np(row), z[f"{name}:row"]) and np.array_equal(_np(col), z[f"{name}:col"])
    rng = np.random.default_rng(7)
    fr = rng.integers(0, 40, 700)
    for mfd in (0, 1, 7, 'max'):
        d = np.abs(fr[:, None] - fr[None, :])
        want = np.nonzero((d > 0) if mfd == 'max' else ((d > 0) & (d <= mfd)))
        row, col = G.get_time_valid_conn_ixs(torch.from_numpy(fr).to(dev()), mfd, return_undirected=False)
        assert np.array_equal(_np(row), want[0]) and np.array_equal(_np(col), want[1]), mfd
    row, col = G.get_time_valid_conn_ixs(torch.zeros(0, dtype=torch.int64, device=dev()), 'max', return_undirected=False)
    assert row.numel() == 0 and col.numel() == 0
    # the undirected form is unchanged: the directed pairs with row < col
    und = G.get_time_valid_conn_ixs(torch.from_numpy(fr).to(dev()), 7)
    row, col = G.get_time_valid_conn_ixs(torch.from_numpy(fr).to(dev()), 7, return_undirected=False)
    assert np.array_equal(_np(und), np.stack((_np(row), _np(col)))[:, _np(row) < _np(col)])


# ---------------------------------------------------------------------------------------------- end to end
def _model(mask_branch=True):
    params = synth.model_params(32, 4, "sum", num_class_steps=2, node_in_dim=64)
    W = synth.make_weights(params, seed=7, gain=0.6)
    if mask_branch:
        params = dict(params)
        params.update(synth.MASK_PARAMS)
        W.update(synth.make_mask_weights(seed=17))
    model = MOTMPNet(params)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    return model.to(dev()).eval()


def _inputs(z, sq, with_x_ext=True):
    t = {k: torch.from_numpy(z[f"{sq}:{k}"]).to(dev()) for k in ("x", "edge_index", "edge_attr", "reid_emb_dists")}
    n = z[f"{sq}:frame"].shape[0]
    x_ext = torch.from_numpy(synth.normal(9, (n, 256, 14, 14), stream=1, std=0.5)).to(dev()) if with_x_ext else None
    return (t["x"], t["edge_index"], t["edge_attr"], t["reid_emb_dists"], z[f"{sq}:frame"]), x_ext


def _cfg(z, tag):
    inactive, recip, fpg, top_k = [int(v) for v in z[f"{tag}:cfg"]]
    return dict(frames_per_graph=fpg, top_k_nns=top_k, reciprocal_k_nns=bool(recip), set_pruned_edges_to_inactive=bool(inactive))


def _pair_keys(ei):
    return (np.asarray(ei[0]).astype(np.int64) << 32) | np.asarray(ei[1]).astype(np.int64)


@pytest.mark.parametrize("windows_per_launch", [1, 3])
@pytest.mark.parametrize("tag", SEQ_CASES)
def test_evaluate_sequence_against_the_reference_tracker(golden, tag, windows_per_launch):
    """Bounds: 2e-5 on the directed, undirected and kept scores (the bound of the g10 test; a mean of two values inside it is
    inside it); the kept set up to the pairs whose REFERENCE score is within 2e-5 of 0.5, the only ones the tolerance allows to
    flip, and at most 1 % of a case's pairs (0, 0, 0 and 1 of 5,044 here); node masks within 5e-5 * max |mask logit| (the mask-branch
    test allows 2e-4 of the largest logit, sigmoid has slope <= 1/4), per-node sums within 3136 times that.
    Measured on an MI355X, all eight cases alike: scores 6e-8 .. 1.2e-7, node masks 3.3e-7 (bound 9.3e-5 .. 9.7e-5), per-node sums
    <= 5e-5; the kept sets equal the reference's (56, 74, 158, 189 pairs).  Every figure is printed before the assertions."""
    z = golden("g17_window_tail.npz")
    sq = tag[0]
    args, x_ext = _inputs(z, sq)
    n = args[0].shape[0]
    res = tracker.evaluate_sequence(_model(), *args, windows_per_launch=windows_per_launch, x_ext=x_ext, **_cfg(z, tag))
    final = _np(res.final_edge_preds)
    err_final = float(np.abs(final - z[f"{tag}:final_edge_preds"]).max())
    # undirected scores before pruning: the merge of the directed scores this call produced
    ei_u, (pu,), _ = G.merge_undirected(args[1], [res.final_edge_preds])
    ref_u = z[f"{tag}:edge_preds_u"]
    assert np.array_equal(_np(ei_u), z[f"{tag}:edge_index_u"])
    err_u = float(np.abs(_np(pu) - ref_u).max())
    # kept set: equal to the reference's once the pairs the tolerance allows to flip are left out
    near = np.abs(ref_u - 0.5) <= TOL
    near_keys = _pair_keys(z[f"{tag}:edge_index_u"])[near]
    got_keys, ref_keys = _pair_keys(_np(res.edge_index)), _pair_keys(z[f"{tag}:edge_index"])
    got_sel, ref_sel = ~np.isin(got_keys, near_keys), ~np.isin(ref_keys, near_keys)
    same_set = np.array_equal(got_keys[got_sel], ref_keys[ref_sel])
    common = np.intersect1d(got_keys, ref_keys)
    got_p = _np(res.edge_preds)[np.searchsorted(got_keys, common)]
    ref_p = z[f"{tag}:edge_preds"][np.searchsorted(ref_keys, common)]
    err_kept = float(np.abs(got_p - ref_p).max())
    # node masks
    node_preds = _np(res.node_preds)
    bound_mask = 5e-5 * float(z[f"{tag}:max_abs_mask_logit"])
    if sq == "s":
        err_mask = float(np.abs(node_preds - golden("g17_window_tail_masks.npz")[f"{tag}:node_preds"]).max())
        err_sum = 0.0
    else:
        err_mask = float(np.abs(node_preds[:16] - z[f"{tag}:node_preds_head"]).max())
        err_sum = float(np.abs(node_preds.astype(np.float64).sum(axis=(1, 2, 3)) - z[f"{tag}:node_preds_sum"]).max())
    print("g17 %s wpl=%d: final %.3g undirected %.3g kept %.3g (bound %.1g); left out %d of %d pairs; kept %d (reference %d); "
          "node masks %.3g (bound %.3g), per-node sums %.3g (bound %.3g)"
          % (tag, windows_per_launch, err_final, err_u, err_kept, TOL, int(near.sum()), near.size, got_keys.size, ref_keys.size,
             err_mask, bound_mask, err_sum, 3136 * bound_mask))
    assert err_final < TOL
    assert err_u < TOL
    assert int(near.sum()) <= 0.01 * near.size
    assert same_set
    assert common.size > 0 and err_kept < TOL
    assert np.array_equal(got_keys, np.sort(got_keys)) and res.edge_index.dtype == torch.int64
    assert bool((_np(res.edge_index)[0] < _np(res.edge_index)[1]).all())
    assert tuple(res.node_preds.shape) == (n, 1, 56, 56) and not np.isnan(node_preds).any()
    assert err_mask <= bound_mask
    assert err_sum <= 3136 * bound_mask   # a sum of 3136 entries each inside the bound


def test_evaluate_sequence_properties(golden):
    z = golden("g17_window_tail.npz")
    args, x_ext = _inputs(z, "l")
    model = _model()
    cfg = _cfg(z, "l1")
    one = tracker.evaluate_sequence(model, *args, x_ext=x_ext, **cfg)
    # the directed scores are evaluate_graph_in_batches's, bit for bit
    assert torch.equal(one.final_edge_preds, tracker.evaluate_graph_in_batches(model, *args, **cfg))
    # the undirected list is the merge + pruning of those scores
    ei_u, (pu,), _ = G.merge_undirected(args[1], [one.final_edge_preds])
    ek, pk, _ = G.prune_edges(ei_u, pu)
    assert torch.equal(ek, one.edge_index) and torch.equal(pk, one.edge_preds)
    # several windows per launch change nothing
    three = tracker.evaluate_sequence(model, *args, x_ext=x_ext, windows_per_launch=3, **cfg)
    assert float((three.final_edge_preds - one.final_edge_preds).abs().max()) <= 1e-6
    assert float((three.node_preds - one.node_preds).abs().max()) <= 1e-6
    # two "ranks": the four accumulators of each, captured through reduce_fn and summed as all_reduce(sum) would
    acc = []
    for r in range(2):
        tracker.evaluate_sequence(model, *args, x_ext=x_ext, rank=r, world_size=2, reduce_fn=lambda t: acc.append(t.clone()), **cfg)
    assert len(acc) == 8
    preds, num, node, node_num = (acc[i] + acc[4 + i] for i in range(4))
    both = torch.where(num > 0, preds / num, torch.zeros_like(preds))
    assert float((both - one.final_edge_preds).abs().max()) <= 1e-6
    assert tuple(node.shape) == tuple(one.node_preds.shape) and bool((node_num > 0).all())
    assert float((node / node_num.view(-1, 1, 1, 1) - one.node_preds).abs().max()) <= 1e-6


def test_last_step_only_mask_evaluation_is_bitwise_the_full_forward(golden):
    """``last_only`` skips the earlier class steps' mask heads and nothing else: its one prediction is bit for bit the last of
    ``model(data)['mask_predictions']`` on one window.  The hot path, the attention kernel and the stock convolutions repeat
    bitwise within a process (0 mismatches in 190 repetitions on an MI355X); the comparison does rely on the convolution library
    running the same solver in both evaluations, so the per-stage differences are printed before the assertions."""
    z = golden("g17_window_tail.npz")
    (x, ei, ea, dist, frame), x_ext = _inputs(z, "s")
    model = _model()
    n0, n1 = tracker.frame_windows(frame, 5)[1]
    sub_ei, sub_attr, _, _ = tracker.window_subgraph(ei, ea, dist, n0, n1, 6, True)
    data = Graph(x=x[n0:n1].contiguous(), x_ext=x_ext[n0:n1].contiguous(), edge_index=sub_ei, edge_attr=sub_attr)
    with torch.no_grad():
        out = model(data)
        logits = model.hot_path(data.x, sub_ei, sub_attr)
        last = model.mask_predictions(data.x_ext, sub_ei, logits, last_only=True)
        every = model.mask_predictions(data.x_ext, sub_ei, logits)
    print("last-step-only: logits %.3g; all steps vs forward %s; last only vs forward %.3g"
          % (float((logits - model.last_logits).abs().max()), [float((a - b).abs().max()) for a, b in zip(every, out["mask_predictions"])],
             float((last[0] - out["mask_predictions"][-1]).abs().max())))
    assert len(out["mask_predictions"]) == 2 and len(every) == 2 and len(last) == 1
    assert tuple(last[0].shape) == (n1 - n0, 1, 56, 56)
    assert torch.equal(last[0], out["mask_predictions"][-1])
    for a, b in zip(every, out["mask_predictions"]):
        assert torch.equal(a, b)


def test_evaluate_sequence_degenerate(golden):
    z = golden("g17_window_tail.npz")
    args, x_ext = _inputs(z, "s")
    n, E = args[0].shape[0], args[1].shape[1]
    model = _model()
    # more frames per window than the sequence has: no window -- all scores 0, nothing kept, every node 0 / 0 (as the reference)
    res = tracker.evaluate_sequence(model, *args, frames_per_graph=40, top_k_nns=5, x_ext=x_ext)
    assert res.final_edge_preds.shape[0] == E and float(res.final_edge_preds.abs().max()) == 0.0
    assert tuple(res.edge_index.shape) == (2, 0) and res.edge_preds.numel() == 0
    assert tuple(res.node_preds.shape) == (n, 1, 56, 56) and bool(torch.isnan(res.node_preds).all())
    # no x_ext, or a model without the mask branch: no node_preds, the same edges
    cfg = _cfg(z, "s1")
    full = tracker.evaluate_sequence(model, *args, x_ext=x_ext, **cfg)
    for res in (tracker.evaluate_sequence(model, *args, **cfg), tracker.evaluate_sequence(_model(mask_branch=False), *args, x_ext=x_ext, **cfg)):
        assert res.node_preds is None
        assert torch.equal(res.final_edge_preds, full.final_edge_preds)
        assert torch.equal(res.edge_index, full.edge_index) and torch.equal(res.edge_preds, full.edge_preds)
    # top_k = 0 prunes every edge of every window: nothing predicted, nothing kept
    res = tracker.evaluate_sequence(model, *args, frames_per_graph=3, top_k_nns=0)
    assert float(res.final_edge_preds.abs().max()) == 0.0 and tuple(res.edge_index.shape) == (2, 0) and res.node_preds is None
    # ... while the mask branch still runs, on windows without edges
    res = tracker.evaluate_sequence(model, *args, frames_per_graph=3, top_k_nns=0, x_ext=x_ext, windows_per_launch=2)
    assert tuple(res.edge_index.shape) == (2, 0) and tuple(res.node_preds.shape) == (n, 1, 56, 56)
    assert not bool(torch.isnan(res.node_preds).any()) and 0.0 < float(res.node_preds.min()) and float(res.node_preds.max()) < 1.0
    # a lower threshold keeps more
    low = tracker.evaluate_sequence(model, *args, prune_threshold=0.1, **cfg)
    assert low.edge_index.shape[1] > full.edge_index.shape[1] and float(low.edge_preds.min()) >= 0.1
