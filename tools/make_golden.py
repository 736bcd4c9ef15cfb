#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE implementation (authoring container only).

The reference's Python never travels to the GPU box; this script imports
``/root/reference/src/mot_neural_solver/models/mpn.py`` here, drives it on inputs from the
repo's own deterministic generator (``mpntrackseg_amd/synth.py``) and stores the outputs as
small fixtures.  The only thing injected is a stand-in for the un-vendored third-party
``torch_scatter`` 2.0.4 package (``environment.yml:146``), restating its documented semantics with
stock torch ops (scatter_add_ / clamp / scatter_reduce amax, empty segments -> 0).

Fixtures:
  g1_tiny_{sum,mean,max}.npz   full ``MOTMPNet.forward`` (mask branch included) on N=60/E=800, default
                               dims with node_in_dim=64; inputs, weights, logits of every step, final
                               x/e, and autograd gradients of loss = sum_steps sum_edges logit*r.
  g4_structure.npz             isolated nodes, only-past / only-future nodes, 3 batched sub-graphs
                               (interleaved halves), self loops, ties at 0 under max.
  g5_modules.npz               MetaLayer.forward single step and node_agg_fn alone.
  g2_cfgA_{agg}.npz            cfg-A (500/4000/d32/L6): logits [6,4000]; inputs regenerated (checksums).
  g3_cfgB_{agg}.npz            cfg-B (5000/50000/d128/L12): logits at 4096 fixed edges x 12 steps +
                               per-step sum / abs-sum / max checksums.
  g0_l0.npz                    num_enc_steps == 0 special case (mpn.py:387-389).
  g11_cfgB_sum_o1.npz          cfg-B, sum aggregation, 12 steps, weights scaled to O(1) logits: sampled logits, checksums and the
                               reference's autograd gradients (the headline training workload).
  g12_dense_knn_{agg}.npz      dense reciprocal-kNN graph (E / N = 64, d = 32, 12 steps): sampled logits + reference autograd.
  g9_loss_metrics.npz          MOTNeuralSolver._compute_loss (+ autograd) and compute_perform_metrics / compute_constr_satisfaction_rate.
  g10_windows.npz              MPNTracker._evaluate_graph_in_batches on a synthetic sequence with the reference model.
  g17_window_tail.npz          the same call to its END: the undirected merge, the pruned edge list and the averaged node masks, on g10's
  (+ g17_window_tail_masks)    sequence and a longer one; get_time_valid_conn_ixs(return_undirected=False).  Only with --only g17.
  g7_graph_utils.npz           the reference's utils/graph.py on a synthetic detection table (synth.make_detections):
                               get_time_valid_conn_ixs ('max' and 3 frames), compute_edge_feats_dict, F.pairwise_distance,
                               get_knn_mask (reciprocal on/off; one direction per pair and both directions).
  g15_batchnorm_train.npz      MLPs with BatchNorm1d in TRAINING mode: the reference's forward, autograd (incl. BatchNorm weights) and
                               running statistics in float64 (three aggregations).
  g6_mask_branch.npz           full forward WITH the attention / mask branch (deterministic weights for all 54
                               tensors): mask predictions + reference-autograd gradients through both branches.
  g18_attention.npz            TimeAwareAttentionModel.forward alone (identity node_model, given logits) on a 40-node / 400-edge graph
                               with self loops, duplicate edges and empty segments: flow_in / flow_out + reference autograd.  Only
                               with --only g18.
  g19_projection.npz           GreedyProjector.project, MPNTracker._assign_ped_ids and Postprocessor.drop_short_trajectories (min_track_len
                               2 and 5) on three 48-node score graphs (one with tied scores), a 650-node graph with a hub of > 256 active
                               edges on each side, and the pruned undirected outputs of g17.  Only with --only g19.
  g20_full_masks.npz           MPNTracker._to_full_masks on 3 frames of at most 6 RoI masks (56 x 56, image 96 x 128): the binary masks of
                               the reference's ensure_unique_masks over the literal paste (tests/full_masks_ref.py literal_paste: torch's
                               own CPU resize), bit-packed, their COCO strings, and the sample line of the MOTS evaluation kit's README.
                               Only with --only g20.
  g21_training_targets.npz     MOTGraph.assign_edge_labels ('all' and 'closest') on seven graphs (gaps, unmatched nodes, stored duplicates,
                               self loops, a batch, several blocks of edges) and MOTNeuralSolver._compute_loss WITH its segmentation term
                               (+ autograd w.r.t. the logits and the mask predictions) on six cases incl. a batch of three graphs, and end
                               to end through g6's model.  Inputs come from tests/training_targets_ref.py.  Only with --only g21.
  g22_mots_metrics.npz         MOTSMetrics.compute_metrics_per_sequence + compute_clearmot of the vendored MOTS evaluation kit on two scenes
                               of id images: "cases" (12 frames of 37 x 29 with an id switch, a fragment, ignore regions, a pair at IoU
                               exactly 0.5, ...) and "crowded" (3 frames of 64 x 48 with 110 objects a side).  pycocotools is not
                               installed: the kit runs over a numpy stand-in built on the project's RLE codec.  Only with --only g22.
  g23_hota.npz                 TrackEval's KittiMOTS preprocessing and HOTA.eval_sequence (class pedestrian) on g22's two scenes (read from
                               g22_mots_metrics.npz, not stored again) and on "association" (12 frames of 37 x 29: a track covered by two
                               prediction ids in turn, a swap, a prediction the global alignment assigns against the frame's IoU, IoUs at
                               every twentieth, removals by the ignore region), and HOTA.combine_sequences over the three: every result
                               field, the four counts and per frame the kept prediction ids.  Only with --only g23.

  g24_clear_identity.npz       TrackEval's CLEAR, Identity, Count and HOTA .eval_sequence for the classes car and pedestrian on g22's and
                               g23's scenes (not stored again) and on "clear" (12 frames of 30 x 40: a row star and a column star decided by
                               continuity, a frame without predictions, a frame without ground truth, objects matched in exactly 4 of 5
                               and 1 of 5 frames, a car with an absence, an id switch and a removed prediction), and the three combine
                               methods of every metric: every field per scene and class, the COMBINED_SEQ rows.  Only with --only g24.

Usage:  python tools/make_golden.py [--only g1,g2,...]
"""
import sys
sys.dont_write_bytecode = True  # never leave __pycache__ inside the read-only reference tree
import argparse
import os
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mpntrackseg_amd import synth  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")


# ------------------------------------------------------------------ torch_scatter 2.0.4 stand-in
def _bcast(index, src, dim):
    if index.dim() == 1:
        shape = [1] * src.dim()
        shape[dim] = -1
        index = index.view(shape)
    return index.expand_as(src)


def _scatter_add(src, index, dim=-1, out=None, dim_size=None):
    dim = dim % src.dim()
    size = list(src.size())
    size[dim] = dim_size if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
    out = torch.zeros(size, dtype=src.dtype, device=src.device)
    return out.scatter_add_(dim, _bcast(index, src, dim), src)


def _scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    dim = dim % src.dim()
    out = _scatter_add(src, index, dim, None, dim_size)
    ones = torch.ones(index.size(), dtype=src.dtype, device=src.device)
    count = _scatter_add(ones, index, 0, None, out.size(dim)).clamp_(1)
    shape = [1] * out.dim()
    shape[dim] = -1
    return out / count.view(shape)


def _scatter_max(src, index, dim=-1, out=None, dim_size=None):
    dim = dim % src.dim()
    size = list(src.size())
    size[dim] = dim_size if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
    out = torch.zeros(size, dtype=src.dtype, device=src.device)
    if src.numel():
        out = out.scatter_reduce(dim, _bcast(index, src, dim), src, reduce="amax", include_self=False)
    return out, None


def _scatter_min(src, index, dim=-1, out=None, dim_size=None):
    raise NotImplementedError   # (imported by data/mot_graph.py at module level; no function under test calls it)


def _scatter_softmax(src, index, dim=-1, eps=1e-12):
    dim = dim % src.dim()
    n = int(index.max()) + 1 if index.numel() else 0
    idx = _bcast(index, src, dim)
    mx = torch.zeros([n] + list(src.shape[1:]), dtype=src.dtype).scatter_reduce(
        dim, idx, src, reduce="amax", include_self=False)
    ex = (src - mx.gather(dim, idx)).exp()
    sm = _scatter_add(ex, index, dim, None, n)
    return ex / (sm.gather(dim, idx) + eps)


def install_shim():
    ts = types.ModuleType("torch_scatter")
    ts.scatter_add, ts.scatter_mean, ts.scatter_max, ts.scatter_min = (
        _scatter_add, _scatter_mean, _scatter_max, _scatter_min)
    comp = types.ModuleType("torch_scatter.composite")
    comp.scatter_softmax = _scatter_softmax
    ts.composite = comp
    sys.modules["torch_scatter"] = ts
    sys.modules["torch_scatter.composite"] = comp


def import_reference():
    install_shim()
    sys.path.insert(0, "/root/reference/src")
    from mot_neural_solver.models import mpn  # noqa
    return mpn


MASK_PARAMS = synth.MASK_PARAMS  # mask-branch dicts of configs/tracking_cfg.yaml:168-218


def build_reference_model(mpn, params, weights):
    full = dict(params)
    full.update(MASK_PARAMS)
    torch.manual_seed(0)
    model = mpn.MOTMPNet(full)
    sd = {k: torch.from_numpy(v) for k, v in weights.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(not any(m.startswith(p) for p in ("encoder.", "MPNet.", "classifier.")) for m in missing), missing
    return model


def ref_hot_path(model, x, edge_index, edge_attr, want_all=True):
    """Drive the REFERENCE modules (encoder / MPNet / classifier) with the loop of mpn.py:355-381,
    leaving out the x_ext lines.  Verified equal to the full forward in g1 below."""
    e, xn = model.encoder(edge_attr, x)
    e0, x0 = e, xn
    logits = []
    for _ in range(model.num_enc_steps):
        e = torch.cat((e0, e), dim=1)
        xn = torch.cat((x0, xn), dim=1)
        xn, e = model.MPNet(xn, edge_index, e)
        dec, _ = model.classifier(e)
        logits.append(dec)
    if model.num_enc_steps == 0:
        dec, _ = model.classifier(e)
        logits.append(dec)
    return logits, xn, e


class Data:
    pass


def gen_g1(mpn):
    for agg in ("sum", "mean", "max"):
        N, E, L, nin = 60, 800, 4, 64
        params = synth.model_params(32, L, agg, num_class_steps=3, node_in_dim=nin)
        W = synth.make_weights(params, seed=7)
        g = synth.make_graph(N, E, T=10, seed=1, node_in_dim=nin)
        model = build_reference_model(mpn, params, W)
        d = Data()
        # reference input layout: x is [N, C, 8, 4] before the avg-pool (seq_processor.py:445)
        x4 = synth.normal(3, (N, nin, 8, 4), stream=9)
        d.x = torch.from_numpy(x4)
        d.x_ext = torch.from_numpy(synth.normal(3, (N, 256, 14, 14), stream=10, std=0.5))
        d.edge_index = torch.from_numpy(g["edge_index"])
        d.edge_attr = torch.from_numpy(g["edge_attr"])
        with torch.no_grad():
            out = model(d)
        full_logits = [t.numpy() for t in out["classified_edges"]]
        assert len(full_logits) == 3 and full_logits[0].shape == (E, 1)

        # hot-path driver on the pooled input, with autograd
        xp = d.x.mean(dim=(2, 3)).clone().requires_grad_(True)
        ea = d.edge_attr.clone().requires_grad_(True)
        logits, xL, eL = ref_hot_path(model, xp, d.edge_index, ea)
        for a, b in zip(full_logits, logits[-3:]):
            assert np.array_equal(a, b.detach().numpy()), "driver loop != MOTMPNet.forward"
        r = torch.from_numpy(synth.normal(11, (L, E), stream=0))
        loss = sum((logits[s].view(-1) * r[s]).sum() for s in range(L))
        hot = {k: p for k, p in model.named_parameters() if k in W}
        grads = torch.autograd.grad(loss, [xp, ea] + list(hot.values()))
        rec = {
            "agg": agg, "N": N, "E": E, "L": L, "d": 32, "node_in_dim": nin,
            "x4": x4, "x_pooled": xp.detach().numpy(), "edge_index": g["edge_index"], "edge_attr": g["edge_attr"],
            "logits": np.stack([t.detach().numpy().reshape(-1) for t in logits]),
            "x_final": xL.detach().numpy(), "e_final": eL.detach().numpy(),
            "r": r.numpy(), "grad_x": grads[0].numpy(), "grad_edge_attr": grads[1].numpy(),
        }
        for k, v in W.items():
            rec["W:" + k] = v
        for k, gr in zip(hot.keys(), grads[2:]):
            rec["G:" + k] = gr.numpy()
        np.savez_compressed(os.path.join(GOLD, f"g1_tiny_{agg}.npz"), **rec)
        print("g1", agg, "max|logit|", float(np.abs(rec["logits"]).max()))


def gen_g6(mpn):
    """Full MOTMPNet.forward INCLUDING the attention / mask branch with deterministic weights for every parameter:
    mask_predictions of the classified steps (12 nodes + checksums of all), and reference-autograd gradients of
    loss = sum logits*r + sum mask_preds*r2 (hot-path parameters, the first attention conv, x_ext)."""
    N, E, L, nin = 40, 360, 3, 64
    params = synth.model_params(32, L, "sum", num_class_steps=2, node_in_dim=nin)
    W = synth.make_weights(params, seed=7)
    W.update(synth.make_mask_weights(seed=17))
    full = dict(params)
    full.update(MASK_PARAMS)
    model = mpn.MOTMPNet(full)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    g = synth.make_graph(N, E, T=8, seed=4, node_in_dim=nin)
    d = Data()
    d.x = torch.from_numpy(g["x"]).view(N, nin, 1, 1)
    d.x_ext = torch.from_numpy(synth.normal(5, (N, 256, 14, 14), stream=1, std=0.5)).requires_grad_(True)
    d.edge_index = torch.from_numpy(g["edge_index"])
    d.edge_attr = torch.from_numpy(g["edge_attr"])
    out = model(d)
    masks = out["mask_predictions"]
    assert len(masks) == 2 and masks[0].shape == (N, 1, 56, 56)
    r = torch.from_numpy(synth.normal(11, (2, E), stream=0))
    r2 = torch.from_numpy(synth.normal(12, (2, N, 1, 56, 56), stream=0, std=0.05))
    loss = sum((out["classified_edges"][s].view(-1) * r[s]).sum() for s in range(2)) + \
        sum((masks[s] * r2[s]).sum() for s in range(2))
    names = [k for k in W if k.startswith(("encoder.", "MPNet.", "classifier."))] + ["MPAttentionNet.node_model.layers.0.weight",
                                                                                    "mask_predictor.mask_head.layers.0.bias"]
    pd = dict(model.named_parameters())
    grads = torch.autograd.grad(loss, [pd[k] for k in names] + [d.x_ext])
    rec = {"N": N, "E": E, "L": L, "node_in_dim": nin,
           "logits": np.stack([t.detach().numpy().reshape(-1) for t in out["classified_edges"]]),
           "mask_rows": np.stack([m.detach().numpy()[:12] for m in masks]),
           "mask_sum": np.array([float(m.detach().double().sum()) for m in masks]),
           "mask_abssum": np.array([float(m.detach().double().abs().sum()) for m in masks]),
           "grad_x_ext_rows": grads[-1].numpy()[:4, :8],
           "grad_x_ext_abssum": np.float64(grads[-1].double().abs().sum())}
    for k, gr in zip(names, grads[:-1]):
        a = gr.numpy()
        rec["G:" + k] = a if a.size < 20000 else a.reshape(-1)[:20000]
        rec["Gn:" + k] = np.float64(np.sqrt((a.astype(np.float64) ** 2).sum()))
    np.savez_compressed(os.path.join(GOLD, "g6_mask_branch.npz"), **rec)
    print("g6 ok; |mask| per step", rec["mask_abssum"])


def g18_graph():
    """The small operator-level graph of g18: 40 nodes, 400 edges.  Node 0 is isolated; node 1 is only ever a neighbour
    (``col``), never a ``row``: both its segments are empty while its features are gathered; the last node has only past
    neighbours.  380 random (row, col) pairs with row in [2, N) and col in [1, N) (self loops occur), 14 of them stored a
    second time at the end, and 6 forced self loops."""
    N = 40
    row = 2 + (synth.uniform01(18, 380, stream=0) * (N - 2)).astype(np.int64)
    col = 1 + (synth.uniform01(18, 380, stream=1) * (N - 1)).astype(np.int64)
    dup = (synth.uniform01(18, 14, stream=2) * 380).astype(np.int64)
    loops = np.array([2, 5, 5, 17, 38, 39], dtype=np.int64)
    ei = np.stack([np.concatenate([row, row[dup], loops]), np.concatenate([col, col[dup], loops])]).astype(np.int64)
    assert ei.shape == (2, 400) and 0 not in ei and 1 not in ei[0] and 1 in ei[1]
    assert (ei[0] == ei[1]).sum() >= 6 and (ei[0] == N - 1).any()
    return N, ei


def gen_g18(mpn):
    """TimeAwareAttentionModel.forward (mpn.py:111-137) ALONE, on the CPU: identity ``node_model``, a ``cls_net`` that returns
    the given logits -- the operator ``mpnhip_attention_aggregate`` computes, without any convolution behind it.  Recorded: the
    inputs, the concatenated output split back into flow_in / flow_out, and the reference's autograd gradients of x (total:
    the concatenation passes x through as well) and of the logits under a fixed random upstream gradient."""
    N, ei = g18_graph()
    E = ei.shape[1]
    x = torch.from_numpy(synth.normal(18, (N, 4, 2, 2), stream=3)).requires_grad_(True)
    logits = torch.from_numpy(synth.normal(18, (E, 1), stream=4, std=2.0)).requires_grad_(True)
    up = torch.from_numpy(synth.normal(18, (N, 12, 2, 2), stream=5))
    model = mpn.TimeAwareAttentionModel(torch.nn.Identity(), None, None)
    flow, dec = model(x, torch.from_numpy(ei), logits, lambda edge_attr: (edge_attr, None))
    assert flow.shape == (N, 12, 2, 2) and dec is logits and torch.equal(flow[:, :4], x)
    gx, gl = torch.autograd.grad((flow * up).sum(), [x, logits])
    rec = {"edge_index": ei, "x": x.detach().numpy(), "logits": logits.detach().numpy(), "upstream": up.numpy(),
           "flow_in": flow[:, 4:8].detach().numpy(), "flow_out": flow[:, 8:12].detach().numpy(),
           "grad_x_total": gx.numpy(), "grad_logits": gl.numpy()}
    np.savez_compressed(os.path.join(GOLD, "g18_attention.npz"), **rec)
    print("g18 ok: N", N, "E", E, "self loops", int((ei[0] == ei[1]).sum()), "max|flow|", float(flow[:, 4:].detach().abs().max()))


def structure_graph():
    """Hand-built corner cases.  Sub-graph 0 (nodes 0..7): node 0 isolated, node 1 only future
    neighbours, node 7 only past neighbours, one self loop (3,3) -- contributes to the edge update but
    to neither aggregate (mpn.py:85,91).  Sub-graphs 1 and 2 are generated and batched behind it so
    the (i<j) / (j<i) halves interleave."""
    lo = np.array([1, 1, 2, 2, 4, 5, 6, 2], dtype=np.int64)
    hi = np.array([2, 4, 5, 7, 7, 6, 7, 6], dtype=np.int64)
    ei = np.stack([np.concatenate([lo, hi, [3]]), np.concatenate([hi, lo, [3]])]).astype(np.int64)
    nin = 64
    g0 = {"x": synth.normal(21, (8, nin), stream=0), "edge_index": ei,
          "edge_attr": synth.normal(21, (ei.shape[1], 6), stream=1), "frame": np.arange(8)}
    g1 = synth.make_graph(20, 60, T=5, seed=22, node_in_dim=nin)
    g2 = synth.make_graph(12, 30, T=4, seed=23, node_in_dim=nin)
    return synth.batch_graphs([g0, g1, g2])


def gen_g4(mpn):
    g = structure_graph()
    rec = {"x": g["x"], "edge_index": g["edge_index"], "edge_attr": g["edge_attr"]}
    for agg in ("sum", "mean", "max"):
        params = synth.model_params(32, 3, agg, node_in_dim=64)
        W = synth.make_weights(params, seed=8)
        model = build_reference_model(mpn, params, W)
        with torch.no_grad():
            logits, xL, eL = ref_hot_path(model, torch.from_numpy(g["x"]), torch.from_numpy(g["edge_index"]),
                                          torch.from_numpy(g["edge_attr"]))
        rec[f"logits_{agg}"] = np.stack([t.numpy().reshape(-1) for t in logits])
        rec[f"x_final_{agg}"] = xL.numpy()
        rec[f"e_final_{agg}"] = eL.numpy()
    # empty graph (E = 0)
    params = synth.model_params(32, 2, "sum", node_in_dim=64)
    model = build_reference_model(mpn, params, synth.make_weights(params, seed=8))
    with torch.no_grad():
        logits, xL, eL = ref_hot_path(model, torch.from_numpy(g["x"][:5]), torch.zeros((2, 0), dtype=torch.int64),
                                      torch.zeros((0, 6)))
    rec["empty_x_final"] = xL.numpy()
    assert logits[0].shape == (0, 1)
    np.savez_compressed(os.path.join(GOLD, "g4_structure.npz"), **rec)
    print("g4 ok, E =", g["edge_index"].shape[1])


def gen_g5(mpn):
    rec = {}
    g = synth.make_graph(40, 300, T=6, seed=31, node_in_dim=64)
    ei = torch.from_numpy(g["edge_index"])
    for agg in ("sum", "mean", "max"):
        params = synth.model_params(32, 1, agg, node_in_dim=64)
        W = synth.make_weights(params, seed=9)
        model = build_reference_model(mpn, params, W)
        x = torch.from_numpy(synth.normal(32, (40, 64), stream=0))   # [N, 2dn]
        e = torch.from_numpy(synth.normal(32, (300, 32), stream=1))  # [E, 2de]
        with torch.no_grad():
            xo, eo = model.MPNet(x, ei, e)                           # MetaLayer.forward mpn.py:33-54
            m = torch.from_numpy(np.maximum(synth.normal(33, (300, 32), stream=2), 0))  # post-ReLU: ties at 0
            row = ei[0]
            ao = model.MPNet.node_model.node_agg_fn(m, row, 40)      # mpn.py:266-273
        rec.update({f"meta_x_{agg}": xo.numpy(), f"meta_e_{agg}": eo.numpy(), f"agg_{agg}": ao.numpy()})
    rec.update({"x_in": x.numpy(), "e_in": e.numpy(), "edge_index": g["edge_index"], "msg": m.numpy()})
    np.savez_compressed(os.path.join(GOLD, "g5_modules.npz"), **rec)
    print("g5 ok")


def gen_g0(mpn):
    params = synth.model_params(32, 0, "sum", num_class_steps=0, node_in_dim=64)
    W = synth.make_weights(params, seed=7)
    g = synth.make_graph(30, 100, T=5, seed=2, node_in_dim=64)
    model = build_reference_model(mpn, params, W)
    d = Data()
    d.x = torch.from_numpy(g["x"]).view(30, 64, 1, 1)
    d.x_ext = torch.from_numpy(synth.normal(3, (30, 256, 14, 14), stream=10, std=0.5))
    d.edge_index = torch.from_numpy(g["edge_index"])
    d.edge_attr = torch.from_numpy(g["edge_attr"])
    with torch.no_grad():
        out = model(d)
    assert len(out["classified_edges"]) == 1
    np.savez_compressed(os.path.join(GOLD, "g0_l0.npz"), logits=out["classified_edges"][0].numpy().reshape(-1))
    print("g0 ok")


def gen_cfg(mpn, name, tag, sample=None):
    c = synth.CONFIGS[name]
    g = synth.make_graph(c["N"], c["E"], seed=1)
    for agg in ("sum", "mean", "max"):
        params = synth.model_params(c["d"], c["L"], agg)
        W = synth.make_weights(params, seed=7)
        model = build_reference_model(mpn, params, W)
        with torch.no_grad():
            logits, xL, eL = ref_hot_path(model, torch.from_numpy(g["x"]), torch.from_numpy(g["edge_index"]),
                                          torch.from_numpy(g["edge_attr"]))
        lg = np.stack([t.numpy().reshape(-1) for t in logits])          # [L, E]
        rec = {"N": c["N"], "E": c["E"], "d": c["d"], "L": c["L"], "agg": agg,
               "cs_x": np.uint64(synth.checksum(g["x"])), "cs_edge_index": np.uint64(synth.checksum(g["edge_index"])),
               "cs_edge_attr": np.uint64(synth.checksum(g["edge_attr"])),
               "cs_weights": np.uint64(synth.checksum(np.concatenate([v.ravel() for v in W.values()]))),
               "step_sum": lg.astype(np.float64).sum(1), "step_abssum": np.abs(lg).astype(np.float64).sum(1),
               "step_max": np.abs(lg).max(1)}
        if sample is None:
            rec["logits"] = lg
        else:
            ids = (synth.uniform01(99, sample, stream=0) * c["E"]).astype(np.int64)
            rec["edge_ids"] = ids
            rec["logits"] = lg[:, ids]
            rec["x_final_rows"] = xL.numpy()[:64]
        np.savez_compressed(os.path.join(GOLD, f"{tag}_{agg}.npz"), **rec)
        print(tag, agg, "max|logit| per step", rec["step_max"][[0, -1]])


def gen_g13(mpn):
    """BASELINE.json configs[4] at FULL size (20,000 nodes / 400,000 edges / 256-d), two message-passing steps: the reference's
    forward (fp32, CPU) -- 4,096 sampled logits per step + whole-tensor checksums.  'mean' has O(1) logits; 'sum' with gain-0.8
    weights keeps them O(10)."""
    c = synth.CONFIGS["E"]
    g = synth.make_graph(c["N"], c["E"], seed=1)
    L = 2
    for agg, gain in (("mean", 1.0), ("sum", 0.8)):
        params = synth.model_params(c["d"], L, agg)
        W = synth.make_weights(params, seed=7, gain=gain)
        model = build_reference_model(mpn, params, W)
        with torch.no_grad():
            logits, xL, eL = ref_hot_path(model, torch.from_numpy(g["x"]), torch.from_numpy(g["edge_index"]),
                                          torch.from_numpy(g["edge_attr"]))
        lg = np.stack([t.numpy().reshape(-1) for t in logits])
        ids = (synth.uniform01(113, 4096, stream=0) * c["E"]).astype(np.int64)
        rec = {"N": c["N"], "E": c["E"], "d": c["d"], "L": L, "agg": agg, "gain": gain,
               "cs_x": np.uint64(synth.checksum(g["x"])), "cs_edge_index": np.uint64(synth.checksum(g["edge_index"])),
               "cs_edge_attr": np.uint64(synth.checksum(g["edge_attr"])),
               "cs_weights": np.uint64(synth.checksum(np.concatenate([v.ravel() for v in W.values()]))),
               "step_sum": lg.astype(np.float64).sum(1), "step_abssum": np.abs(lg).astype(np.float64).sum(1), "step_max": np.abs(lg).max(1),
               "edge_ids": ids, "logits": lg[:, ids], "x_final_rows": xL.numpy()[:32], "e_final_rows": eL.numpy()[:32]}
        np.savez_compressed(os.path.join(GOLD, f"g13_cfgE_{agg}.npz"), **rec)
        print("g13", agg, "max|logit| per step", rec["step_max"])


def _grad_record(rec, names, grads, gx, gea, ids_e):
    """Gradient fixtures: small tensors whole, large ones as their first 20,000 elements + the Euclidean norm of all."""
    for k, gr in zip(names, grads):
        a = gr.numpy()
        rec["G:" + k] = a if a.size <= 20000 else a.reshape(-1)[:20000].copy()
        rec["Gn:" + k] = np.float64(np.sqrt((a.astype(np.float64) ** 2).sum()))
    a = gx.numpy()
    rec["grad_x"] = a if a.size <= 40000 else a[:16].copy()
    rec["grad_x_norm"] = np.float64(np.sqrt((a.astype(np.float64) ** 2).sum()))
    rec["grad_x_rownorm"] = np.sqrt((a.astype(np.float64) ** 2).sum(1))
    b = gea.numpy()
    rec["grad_edge_attr"] = b[ids_e]
    rec["grad_edge_attr_norm"] = np.float64(np.sqrt((b.astype(np.float64) ** 2).sum()))


def _ref_fwd_bwd(mpn, params, W, g, r):
    model = build_reference_model(mpn, params, W)
    xp = torch.from_numpy(g["x"]).clone().requires_grad_(True)
    ea = torch.from_numpy(g["edge_attr"]).clone().requires_grad_(True)
    logits, xL, eL = ref_hot_path(model, xp, torch.from_numpy(g["edge_index"]), ea)
    L = len(logits)
    loss = sum((logits[s].view(-1) * torch.from_numpy(r[s])).sum() for s in range(L))
    hot = {k: p for k, p in model.named_parameters() if k in W}
    grads = torch.autograd.grad(loss, [xp, ea] + list(hot.values()))
    lg = np.stack([t.detach().numpy().reshape(-1) for t in logits])
    return lg, xL.detach(), eL.detach(), list(hot.keys()), grads


def gen_g15(mpn):
    """MLPs with BatchNorm1d in TRAINING mode (models/mlp.py:14; `use_batchnorm: True` in every feats dict, dropout 0): the
    reference's own forward (batch statistics), its autograd incl. the BatchNorm weights / biases, and the running statistics it
    leaves behind, in float64 -- the fixture of the layer-by-layer path (mpntrackseg_amd/modular.py, tests/test_gpu_modular.py)."""
    rec = {}
    for agg in ("sum", "mean", "max"):
        N, E, L, nin = 90, 700, 2, 48
        params = synth.model_params(32, L, agg, node_in_dim=nin)
        for k in ("encoder_feats_dict", "edge_model_feats_dict", "node_model_feats_dict", "classifier_feats_dict"):
            params[k] = dict(params[k], use_batchnorm=True, dropout_p=0)
        g = synth.make_graph(N, E, seed=4, node_in_dim=nin)
        full = dict(params)
        full.update(MASK_PARAMS)
        torch.manual_seed(5)
        model = mpn.MOTMPNet(full)
        hot = ("encoder.", "MPNet.", "classifier.")
        for name, mod in model.named_modules():      # non-trivial BatchNorm state (float32-representable)
            if isinstance(mod, torch.nn.BatchNorm1d) and name.startswith(hot):
                mod.weight.data.uniform_(0.6, 1.4)
                mod.bias.data.normal_(0, 0.2)
                mod.running_mean.normal_(0, 0.3)
                mod.running_var.uniform_(0.5, 1.5)
        state = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith(hot)}
        model = model.double().train()
        xp = torch.from_numpy(g["x"]).double().requires_grad_(True)
        ea = torch.from_numpy(g["edge_attr"]).double().requires_grad_(True)
        logits, _, _ = ref_hot_path(model, xp, torch.from_numpy(g["edge_index"]), ea)
        r = synth.normal(12, (L, E))
        loss = sum((logits[s].view(-1) * torch.from_numpy(r[s]).double()).sum() for s in range(L))
        named = [(k, p) for k, p in model.named_parameters() if k.startswith(hot)]
        grads = torch.autograd.grad(loss, [xp, ea] + [p for _, p in named])
        rec["%s:logits" % agg] = np.stack([t.detach().numpy().reshape(-1) for t in logits])
        rec["%s:grad_x" % agg] = grads[0].numpy()
        rec["%s:grad_edge_attr" % agg] = grads[1].numpy()
        for (k, _), gr in zip(named, grads[2:]):
            rec["%s:grad:%s" % (agg, k)] = gr.numpy()
        for k, v in state.items():
            rec["%s:state:%s" % (agg, k)] = v.numpy()
        for k, v in model.state_dict().items():       # buffers AFTER the training-mode forward
            if k.startswith(hot) and ("running_" in k or "num_batches" in k):
                rec["%s:after:%s" % (agg, k)] = v.detach().numpy()
        print("g15", agg, "max|logit|", float(np.abs(rec["%s:logits" % agg]).max()))
    np.savez_compressed(os.path.join(GOLD, "g15_batchnorm_train.npz"), **rec)


def gen_g11(mpn):
    """The HEADLINE workload with O(1) logits: cfg-B (5k nodes / 50k edges / 128-d / 12 steps), node_agg_fn = 'sum' (the shipped
    default), He weights scaled by 0.7 so that the sum-aggregated magnitudes stay O(1) over 12 steps (max |logit| 9.4 at step
    12) -- per-element logit parity means something there -- plus the REFERENCE's autograd of loss = sum logits * r."""
    c = synth.CONFIGS["B"]
    g = synth.make_graph(c["N"], c["E"], seed=1)
    params = synth.model_params(c["d"], c["L"], "sum")
    W = synth.make_weights(params, seed=7, gain=0.7)
    r = synth.normal(11, (c["L"], c["E"]))
    lg, xL, eL, names, grads = _ref_fwd_bwd(mpn, params, W, g, r)
    ids = (synth.uniform01(99, 4096, stream=0) * c["E"]).astype(np.int64)
    rec = {"gain": np.float64(0.7), "cs_x": np.uint64(synth.checksum(g["x"])),
           "cs_weights": np.uint64(synth.checksum(np.concatenate([v.ravel() for v in W.values()]))),
           "edge_ids": ids, "logits": lg[:, ids], "step_sum": lg.astype(np.float64).sum(1),
           "step_abssum": np.abs(lg).astype(np.float64).sum(1), "step_max": np.abs(lg).max(1),
           "x_final_rows": xL.numpy()[:64], "e_final_rows": eL.numpy()[ids[:256]]}
    _grad_record(rec, names, grads[2:], grads[0], grads[1], ids)
    np.savez_compressed(os.path.join(GOLD, "g11_cfgB_sum_o1.npz"), **rec)
    print("g11 max|logit| per step", rec["step_max"])


def gen_g12(mpn):
    """BASELINE.json configs[2] stand-in (SURVEY.md section 8d cfg-C): dense reciprocal-kNN graph, 20 frames x 25 detections,
    top-60 (E / N = 64: long segments -- the block-per-segment reductions of the HIP backward), reference dims d = 32, 12 steps,
    all three aggregations, weights scaled so that the logits stay O(1); reference forward AND reference autograd."""
    g = synth.make_knn_graph(frames=20, dets=25, top_k=60, seed=3, node_in_dim=64)
    E = g["edge_index"].shape[1]
    ids = (synth.uniform01(98, 8192, stream=0) * E).astype(np.int64)
    for agg, gain in (("sum", 0.45), ("mean", 1.0), ("max", 1.0)):
        params = synth.model_params(32, 12, agg, node_in_dim=64)
        W = synth.make_weights(params, seed=7, gain=gain)
        r = synth.normal(11, (12, E))
        lg, xL, eL, names, grads = _ref_fwd_bwd(mpn, params, W, g, r)
        rec = {"gain": np.float64(gain), "E": E, "cs_edge_index": np.uint64(synth.checksum(g["edge_index"])),
               "edge_ids": ids, "logits": lg[:, ids], "step_sum": lg.astype(np.float64).sum(1),
               "step_abssum": np.abs(lg).astype(np.float64).sum(1), "step_max": np.abs(lg).max(1),
               "x_final": xL.numpy(), "e_final_rows": eL.numpy()[ids[:1024]]}
        _grad_record(rec, names, grads[2:], grads[0], grads[1], ids)
        np.savez_compressed(os.path.join(GOLD, f"g12_dense_knn_{agg}.npz"), **rec)
        print("g12", agg, "E", E, "max|logit|", rec["step_max"][[0, -1]])


def gen_g7():
    """utils/graph.py of the reference (graph construction / kNN pruning helpers)."""
    import pandas as pd
    import torch.nn.functional as F
    from mot_neural_solver.utils import graph as G
    det = synth.make_detections()
    df = pd.DataFrame({k: det[k] for k in ("frame", "bb_height", "bb_width", "feet_x", "feet_y")})
    emb = torch.from_numpy(det["reid"])
    fps = 25.0
    out = dict(fps=np.float32(fps), **{"det:" + k: det[k] for k in ("frame", "bb_height", "bb_width", "feet_x", "feet_y", "reid")})
    for tag, mfd in (("max", "max"), ("d3", 3)):
        ei = G.get_time_valid_conn_ixs(torch.from_numpy(det["frame"]), mfd, use_cuda=False)
        out[f"{tag}:edge_ixs"] = ei.numpy()
        feats = G.compute_edge_feats_dict(ei, df, fps, use_cuda=False)
        out[f"{tag}:feats"] = torch.stack([feats[k] for k in ("secs_time_dists", "norm_feet_x_dists", "norm_feet_y_dists",
                                                              "bb_height_dists", "bb_width_dists")]).T.numpy()
        d = F.pairwise_distance(emb[ei[0]], emb[ei[1]])
        out[f"{tag}:emb_dist"] = d.numpy()
        for k in (3, 8):
            for rec in (0, 1):
                m = G.get_knn_mask(d, ei, len(df), k, use_cuda=False, reciprocal_k_nns=bool(rec), symmetric_edges=False)
                out[f"{tag}:knn_k{k}_r{rec}_pairs"] = m.numpy()
                ei2 = torch.cat((ei, torch.stack((ei[1], ei[0]))), dim=1)
                m2 = G.get_knn_mask(torch.cat((d, d)), ei2, len(df), k, use_cuda=False, reciprocal_k_nns=bool(rec),
                                    symmetric_edges=True)
                out[f"{tag}:knn_k{k}_r{rec}_sym"] = m2.numpy()
    np.savez_compressed(os.path.join(GOLD, "g7_graph_utils.npz"), **out)
    print("g7_graph_utils.npz", {k: v.shape for k, v in out.items() if k.startswith("max:")})


def gen_g8():
    """load_precomputed_embeddings (utils/rgb.py:150-188): per-frame ``.pt`` files whose column / channel 0 carries the
    detection id.  utils/rgb.py imports skimage / torchvision / pycocotools / matplotlib at module level for its OTHER
    functions (image cropping, mask decoding, plotting); none is installed here and none is touched by the function under
    test, so empty placeholder modules are registered for the import only."""
    import tempfile
    import types
    import pandas as pd
    for name, attrs in (("skimage", ()), ("skimage.io", ("imread",)), ("torchvision", ()),
                        ("torchvision.transforms", ("Compose", "Resize", "ToTensor", "Normalize")),
                        ("pycocotools", ()), ("pycocotools.mask", ()), ("matplotlib", ()), ("matplotlib.pyplot", ())):
        if name not in sys.modules:
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, None)
            sys.modules[name] = m
    from mot_neural_solver.utils import rgb as R
    rng = np.random.RandomState(8)
    frames = [3, 4, 6, 7, 9, 10]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        next_id, stored1, stored3, fr_of, keep_ids, keep_frames = 0, [], [], [], [], []
        os.makedirs(os.path.join(tmp, "processed_data", "emb1d"))
        os.makedirs(os.path.join(tmp, "processed_data", "emb3d"))
        for f in frames:
            n = int(rng.randint(2, 7))
            ids = np.arange(next_id, next_id + n)
            next_id += n
            e1 = np.concatenate([ids[:, None].astype(np.float32), rng.randn(n, 16).astype(np.float32)], axis=1)
            e3 = rng.randn(n, 5, 3, 2).astype(np.float32)
            e3[:, 0] = ids[:, None, None]
            torch.save(torch.from_numpy(e1), os.path.join(tmp, "processed_data", "emb1d", f"{f}.pt"))
            torch.save(torch.from_numpy(e3), os.path.join(tmp, "processed_data", "emb3d", f"{f}.pt"))
            stored1.append(e1); stored3.append(e3); fr_of += [f] * n
            kept = ids[rng.rand(n) < 0.7]           # the detections that survived the reference's filtering steps
            keep_ids += kept.tolist(); keep_frames += [f] * len(kept)
        # a frame none of whose detections survives is not opened at all (frames_to_retrieve = det_df.frame.unique())
        det_df = pd.DataFrame({"frame": keep_frames, "detection_id": keep_ids})
        info = {"seq_path": tmp}
        o1 = R.load_precomputed_embeddings(det_df, info, "emb1d", use_cuda=False, embedding_dim='1D')
        o3 = R.load_precomputed_embeddings(det_df, info, "emb3d", use_cuda=False, embedding_dim='3D')
    out.update(stored_1d=np.concatenate(stored1), stored_3d=np.concatenate(stored3), stored_frame=np.asarray(fr_of, np.int64),
               det_frame=np.asarray(keep_frames, np.int64), det_id=np.asarray(keep_ids, np.int64),
               out_1d=o1.numpy(), out_3d=o3.numpy())
    np.savez_compressed(os.path.join(GOLD, "g8_embedding_files.npz"), **out)
    print("g8_embedding_files.npz", {k: v.shape for k, v in out.items()})


def _placeholder_modules(specs):
    """Empty stand-ins for third-party / unrelated packages a reference module imports at MODULE level for its OTHER functions
    (nothing of them is touched by the function under test); attributes are set to None unless a value is given."""
    for name, attrs in specs:
        if name in sys.modules:
            m = sys.modules[name]
        else:
            m = types.ModuleType(name)
            sys.modules[name] = m
        for a in attrs:
            if isinstance(a, tuple):
                setattr(m, a[0], a[1])
            elif not hasattr(m, a):
                setattr(m, a, None)
        if "." in name:   # make `import a.b` find b as an attribute of a
            parent, child = name.rsplit(".", 1)
            if parent in sys.modules:
                setattr(sys.modules[parent], child, m)


class _GeoData:
    """Stand-in for torch_geometric.data.Data (third party, not installed): an attribute container with the two derived
    properties the reference code reads -- num_nodes (settable, else rows of x) and num_edges (columns of edge_index)."""
    def __init__(self, **kwargs):
        self._num_nodes = None
        for k, v in kwargs.items():
            setattr(self, k, v)

    @property
    def num_nodes(self):
        return self._num_nodes if self._num_nodes is not None else self.x.shape[0]

    @num_nodes.setter
    def num_nodes(self, v):
        self._num_nodes = v

    @property
    def num_edges(self):
        return self.edge_index.shape[1]


def _import_tracking_stack():
    """utils/evaluation.py, pl_module/pl_module.py and tracker/mpn_tracker.py of the reference.  Their module-level imports pull in
    pytorch_lightning, torch_geometric, motmetrics, the MOTS / KITTI evaluation kits, pulp, pycocotools, torchvision, skimage,
    matplotlib, tracktor -- none installed here and none used by the functions under test (_compute_loss,
    compute_perform_metrics, compute_constr_satisfaction_rate, _predict_edges_and_masks, _evaluate_graph_in_batches)."""
    install_shim()
    sys.modules["torch_scatter"].scatter_min = _scatter_min
    if "/root/reference/src" not in sys.path:
        sys.path.insert(0, "/root/reference/src")

    class _Base:
        def __init__(self, *a, **k):
            pass
    _placeholder_modules([
        ("pytorch_lightning", [("LightningModule", _Base), ("Callback", _Base)]),
        ("torch_geometric", []), ("torch_geometric.data", [("Data", _GeoData), ("DataLoader", None)]),
        # (evaluation.py builds its MOT-metric report formatters at import time: mm.metrics.create().formatters, mm.io.*_names)
        ("motmetrics", [("metrics", types.SimpleNamespace(create=lambda: types.SimpleNamespace(formatters={"mota": None}))),
                        ("io", types.SimpleNamespace(motchallenge_metric_names={"mota": "MOTA"}))]),
        ("MOTChallengeEvalKit", []), ("MOTChallengeEvalKit.MOTS", []),
        ("MOTChallengeEvalKit.MOTS.evalMOTS", ["MOTS_evaluator"]),
        ("TrackEval", []), ("TrackEval.scripts", []), ("TrackEval.scripts.run_kitti_mots", ["eval_kitti_mots"]),
        ("pulp", []), ("pycocotools", []), ("pycocotools.mask", []),
        ("skimage", []), ("skimage.io", ["imread"]),
        ("matplotlib", []), ("matplotlib.pyplot", []),
        ("torchvision", []), ("torchvision.ops", ["roi_align"]), ("torchvision.transforms", ["Compose", "Resize", "ToTensor", "Normalize"]),
        ("torchvision.models", []), ("torchvision.models.detection", []), ("torchvision.models.detection.roi_heads", ["paste_masks_in_image"]),
        ("torchvision.models.utils", ["load_state_dict_from_url"]),
        ("tracktor_masked", []), ("tracktor_masked.maskrcnn_fpn", ["MaskRCNN_FPN"]),
        # reference modules that are unrelated to the functions under test and need yet more packages
        ("mot_neural_solver.data.augmentation", ["MOTGraphAugmentor"]),
        ("mot_neural_solver.data.mot_graph_dataset", ["MOTGraphDataset"]),
        ("mot_neural_solver.models.resnet", ["resnet50_fc256", "load_pretrained_weights"]),
    ])
    import mot_neural_solver.data  # noqa: F401  (package first, so that the placeholders above hang off it)
    from mot_neural_solver.utils import evaluation as EV
    from mot_neural_solver.tracker import mpn_tracker as TR
    from mot_neural_solver.pl_module import pl_module as PL
    return EV, TR, PL


def gen_g9():
    """MOTNeuralSolver._compute_loss (pl_module/pl_module.py:88-120; tracking term: no matched masks) with its autograd gradient
    w.r.t. every classified step's logits, and compute_perform_metrics / compute_constr_satisfaction_rate
    (utils/evaluation.py:340-437), on seeded inputs incl. the no-positive-label and single-edge cases."""
    EV, TR, PL = _import_tracking_stack()
    rec = {}
    cases = [("a", 1000, 3, 0.2), ("b", 6000, 12, 0.02), ("c", 777, 4, 0.0), ("d", 1, 1, 1.0)]
    for tag, E, k, frac in cases:
        logits = synth.normal(3, (k, E), std=3.0)
        labels = (synth.uniform01(4, E) < frac).astype(np.float32)
        lg = torch.from_numpy(logits).clone().requires_grad_(True)
        outputs = {"classified_edges": [lg[s].view(E, 1) for s in range(k)],
                   "mask_predictions": [torch.zeros((2, 1, 4, 4)) for _ in range(k)]}
        batch = types.SimpleNamespace(edge_labels=torch.from_numpy(labels), mask_labels=torch.zeros((2, 1, 4, 4)),
                                      mask_gt_ixs=torch.zeros(0, dtype=torch.long))
        solver = types.SimpleNamespace(hparams={"train_params": {"loss_weights": {"tracking": 0.75, "segmentation": 1.0}}})
        loss = PL.MOTNeuralSolver._compute_loss(solver, outputs, batch)
        loss.backward()
        rec.update({f"{tag}:logits": logits, f"{tag}:labels": labels, f"{tag}:loss": np.float64(float(loss)),
                    f"{tag}:grad": lg.grad.numpy(), f"{tag}:weight": np.float64(0.75)})
    # metrics: two batched tracking graphs (both edge directions present), one self loop, thresholded logits
    g = synth.batch_graphs([synth.make_graph(60, 400, T=6, seed=sd, node_in_dim=4) for sd in (1, 2)])
    ei = g["edge_index"].copy()
    ei[:, 3] = [7, 7]
    for tag, seed, frac in (("m1", 8, 0.25), ("m2", 18, 0.6), ("m3", 28, 0.0)):
        E = ei.shape[1]
        logit = synth.normal(seed, (E, 1))
        labels = (synth.uniform01(seed + 1, E) < frac).astype(np.float32)
        go = types.SimpleNamespace(edge_index=torch.from_numpy(ei), edge_labels=torch.from_numpy(labels), num_nodes=120)
        m = EV.compute_perform_metrics({"classified_edges": [torch.from_numpy(logit)]}, go)
        sr, flow_in, flow_out = EV.compute_constr_satisfaction_rate(go, (torch.from_numpy(logit).view(-1) > 0).float(), return_flow_vals=True)
        rec.update({f"{tag}:logit": logit, f"{tag}:labels": labels,
                    f"{tag}:metrics": np.array([m["accuracy"], m["recall"], m["precision"], m["constr_sr"]], np.float64),
                    f"{tag}:flow_in": flow_in.numpy(), f"{tag}:flow_out": flow_out.numpy()})
    rec["edge_index"] = ei
    np.savez_compressed(os.path.join(GOLD, "g9_loss_metrics.npz"), **rec)
    print("g9 ok:", {k: float(v) for k, v in rec.items() if k.endswith(":loss")}, rec["m1:metrics"])


def gen_g16():
    """accumulate_grad_batches (configs/tracking_cfg.yaml:3-4) executed in space on ONE device: K graphs as one block-diagonal batch.
    The reference calls MOTNeuralSolver._compute_loss (pl_module/pl_module.py:88-107) once per graph -- its own pos_weight, its own
    mean -- and Lightning averages the K backward passes: expected loss = mean over the graphs of the reference's loss on the graph's
    slice of the logits, gradient = its autograd.  Cases: 3 graphs of different sizes, one of them without a positive label; 8 equal
    graphs (the shipped accumulate_grad_batches)."""
    EV, TR, PL = _import_tracking_stack()
    rec = {}
    for tag, sizes, k, fracs in (("g3", [700, 1900, 333], 3, [0.15, 0.0, 0.4]), ("g8", [500] * 8, 4, [0.05 * (i + 1) for i in range(8)])):
        E = sum(sizes)
        logits = synth.normal(7, (k, E), std=2.5)
        labels = np.concatenate([(synth.uniform01(11 + i, n) < f).astype(np.float32) for i, (n, f) in enumerate(zip(sizes, fracs))])
        ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        lg = torch.from_numpy(logits).clone().requires_grad_(True)
        solver = types.SimpleNamespace(hparams={"train_params": {"loss_weights": {"tracking": 0.75, "segmentation": 1.0}}})
        total = 0
        per_graph = []
        for i in range(len(sizes)):
            a, b = int(ptr[i]), int(ptr[i + 1])
            outputs = {"classified_edges": [lg[s, a:b].view(b - a, 1) for s in range(k)],
                       "mask_predictions": [torch.zeros((2, 1, 4, 4)) for _ in range(k)]}
            batch = types.SimpleNamespace(edge_labels=torch.from_numpy(labels[a:b]), mask_labels=torch.zeros((2, 1, 4, 4)),
                                          mask_gt_ixs=torch.zeros(0, dtype=torch.long))
            li = PL.MOTNeuralSolver._compute_loss(solver, outputs, batch)
            per_graph.append(float(li))
            total = total + li
        loss = total / len(sizes)
        loss.backward()
        rec.update({f"{tag}:logits": logits, f"{tag}:labels": labels, f"{tag}:edge_ptr": ptr, f"{tag}:loss": np.float64(float(loss)),
                    f"{tag}:per_graph": np.array(per_graph, np.float64), f"{tag}:grad": lg.grad.numpy(), f"{tag}:weight": np.float64(0.75)})
    np.savez_compressed(os.path.join(GOLD, "g16_loss_graphs.npz"), **rec)
    print("g16 ok:", {k: float(v) for k, v in rec.items() if k.endswith(":loss")})


def _tracker_redirections():
    """The reference's tracker module with the two redirections its hard-coded device needs on a CPU: the module's
    `torch.device('cuda')` resolves to the CPU and get_knn_mask is called with use_cuda=False.  ``captured["final_edge_preds"]`` is
    the directed average just before to_undirected_graph."""
    EV, TR, PL = _import_tracking_stack()
    from mot_neural_solver.utils import graph as G
    mpn = import_reference()

    class _TorchProxy:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def device(*a, **k):
            return torch.device("cpu")
    TR.torch = _TorchProxy()
    real_knn = G.get_knn_mask
    TR.get_knn_mask = lambda **kw: real_knn(**dict(kw, use_cuda=False))
    captured = {}
    real_undirected = G.to_undirected_graph

    def capture_then_undirected(mot_graph, attrs_to_update=("edge_preds", "edge_labels")):
        captured["final_edge_preds"] = mot_graph.graph_obj.edge_preds.clone()
        return real_undirected(mot_graph, attrs_to_update=attrs_to_update)
    TR.to_undirected_graph = capture_then_undirected
    return TR, G, mpn, captured


def _tracker_sequence(TR, G, mpn, det, inactive, recip, fpg, top_k, wrap_model=None):
    """One synthetic sequence through MPNTracker._evaluate_graph_in_batches with the reference model (mask branch included).
    Returns ``(full_graph, inputs)``: the MOTGraph stand-in after the call, and the arrays that went in."""
    import pandas as pd
    import torch.nn.functional as F
    n = det["frame"].shape[0]
    df = pd.DataFrame({k: det[k] for k in ("frame", "bb_height", "bb_width", "feet_x", "feet_y")})
    ei = G.get_time_valid_conn_ixs(torch.from_numpy(det["frame"]), "max", use_cuda=False)
    feats = G.compute_edge_feats_dict(ei, df, 25.0, use_cuda=False)
    ef = torch.stack([feats[k] for k in ("secs_time_dists", "norm_feet_x_dists", "norm_feet_y_dists", "bb_height_dists",
                                         "bb_width_dists")]).T
    emb = torch.from_numpy(det["reid"])
    dist = F.pairwise_distance(emb[ei[0]], emb[ei[1]]).view(-1, 1)
    ef = torch.cat((ef, dist), dim=1)
    edge_index = torch.cat((ei, torch.stack((ei[1], ei[0]))), dim=1)
    edge_attr = torch.cat((ef, ef), dim=0)
    emb_dists = torch.cat((dist, dist))
    params = synth.model_params(32, 4, "sum", num_class_steps=2, node_in_dim=64)
    W = synth.make_weights(params, seed=7, gain=0.6)
    W.update(synth.make_mask_weights(seed=17))
    full = dict(params)
    full.update(MASK_PARAMS)
    model = mpn.MOTMPNet(full)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    x = torch.from_numpy(det["x"]).view(n, 64, 1, 1)
    x_ext = torch.from_numpy(synth.normal(9, (n, 256, 14, 14), stream=1, std=0.5))
    from mot_neural_solver.data.mot_graph import Graph
    graph_obj = Graph(x=x, x_ext=x_ext, edge_attr=edge_attr, reid_emb_dists=emb_dists, edge_index=edge_index)
    full_graph = types.SimpleNamespace(frames=sorted(set(det["frame"].tolist())), graph_df=df, graph_obj=graph_obj,
                                       frames_per_graph=fpg)
    tracker = TR.MPNTracker(dataset=None, graph_model=model if wrap_model is None else wrap_model(model), use_gt=False,
                            eval_params={"set_pruned_edges_to_inactive": inactive},
                            dataset_params={"top_k_nns": top_k, "reciprocal_k_nns": recip, "gt_mask_spatial_size": [56, 56]})
    tracker.full_graph = full_graph
    tracker._evaluate_graph_in_batches()
    inputs = {"frame": det["frame"], "x": det["x"], "edge_index": edge_index.numpy(), "edge_attr": edge_attr.numpy(),
              "reid_emb_dists": emb_dists.numpy()}
    return full_graph, inputs


def gen_g10():
    """MPNTracker._evaluate_graph_in_batches + _predict_edges_and_masks (tracker/mpn_tracker.py:96-210) on a synthetic sequence,
    driven with the REFERENCE model (mask branch included) on CPU (redirections: _tracker_redirections)."""
    TR, G, mpn, captured = _tracker_redirections()
    rec = {}
    for tag, inactive, recip, fpg, top_k in (("w1", False, True, 5, 6), ("w2", True, False, 4, 4)):
        det = synth.make_detections(frames=9, dets_lo=3, dets_hi=6, seed=5, emb_dim=32, node_in_dim=64, frame_stride=2)
        full_graph, inputs = _tracker_sequence(TR, G, mpn, det, inactive, recip, fpg, top_k)
        rec.update({f"{tag}:{k}": v for k, v in inputs.items()})
        rec.update({f"{tag}:final_edge_preds": captured["final_edge_preds"].numpy(),
                    f"{tag}:cfg": np.array([int(inactive), int(recip), fpg, top_k], np.int64)})
        print("g10", tag, "nodes", det["frame"].shape[0], "edges", inputs["edge_index"].shape[1], "mean pred",
              float(captured["final_edge_preds"].mean()), "windows", len(full_graph.frames) - fpg + 1)
    np.savez_compressed(os.path.join(GOLD, "g10_windows.npz"), **rec)


G17_TOL = 2e-5          # the tolerance of the end-to-end edge scores (tests/test_gpu_tracker.py): pairs whose reference score is
G17_MAX_NEAR = 0.01     # this close to 0.5 may flip in the kept set; at most this fraction of a case's pairs may be that close


def gen_g17():
    """MPNTracker._evaluate_graph_in_batches to its END (tracker/mpn_tracker.py:143-210): the directed scores as g10 captures them,
    the graph after to_undirected_graph (edge_index, edge_preds and the inverse map scatter_mean receives), after
    to_lightweight_graph (the edges with edge_preds >= 0.5), the averaged node masks and the largest |mask_predictions[-1]| any
    window saw.  g10's two configurations on g10's sequence (s*) and on a longer one (l*: 16 frames, 104 nodes, 10,088 directed
    edges; node_preds for the first 16 nodes plus a float64 sum per node).  The inputs of a sequence are stored once.  The full
    node_preds of the short cases go into a file of their own (g17_window_tail_masks.npz) to keep every file under 1 MiB.  Also get_time_valid_conn_ixs(return_undirected=False) for 'max' and a bounded distance."""
    TR, G, mpn, captured = _tracker_redirections()
    real_light, real_mean = G.to_lightweight_graph, G.scatter_mean

    def capture_mean(src, index, *a, **k):
        captured["orig_indices"] = index.clone()
        return real_mean(src, index, *a, **k)
    G.scatter_mean = capture_mean

    def capture_then_light(mot_graph, *a, **k):
        captured["edge_index_u"] = mot_graph.graph_obj.edge_index.clone()
        captured["edge_preds_u"] = mot_graph.graph_obj.edge_preds.clone()
        return real_light(mot_graph, *a, **k)
    TR.to_lightweight_graph = capture_then_light

    class wrap_model:
        """The model as MPNTracker sees it, recording the largest |mask_predictions[-1]| of the windows."""
        def __init__(self, model):
            self.model = model

        def eval(self):
            self.model.eval()
            return self

        def __call__(self, subgraph):
            out = self.model(subgraph)
            captured["max_abs_mask_logit"] = max(captured.get("max_abs_mask_logit", 0.0), float(out["mask_predictions"][-1].abs().max()))
            return out

    rec, masks = {}, {}
    seqs = {"s": dict(frames=9, dets_lo=3, dets_hi=6, seed=5), "l": dict(frames=16, dets_lo=4, dets_hi=9, seed=11)}
    for sq, kw in seqs.items():
        det = synth.make_detections(emb_dim=32, node_in_dim=64, frame_stride=2, **kw)
        rec[f"{sq}:seq"] = np.array([kw["frames"], kw["dets_lo"], kw["dets_hi"], kw["seed"]], np.int64)
        for i, (inactive, recip, fpg, top_k) in enumerate(((False, True, 5, 6), (True, False, 4, 4))):
            tag = f"{sq}{i + 1}"
            captured.pop("max_abs_mask_logit", None)
            full_graph, inputs = _tracker_sequence(TR, G, mpn, det, inactive, recip, fpg, top_k, wrap_model=wrap_model)
            go = full_graph.graph_obj
            rec.update({f"{sq}:{k}": v for k, v in inputs.items()})
            pu = captured["edge_preds_u"].numpy()
            near = int((np.abs(pu - 0.5) <= G17_TOL).sum())
            assert near <= G17_MAX_NEAR * pu.size, (tag, near, pu.size)
            node_preds = go.node_preds.numpy()
            rec.update({f"{tag}:cfg": np.array([int(inactive), int(recip), fpg, top_k], np.int64),
                        f"{tag}:final_edge_preds": captured["final_edge_preds"].numpy(),
                        f"{tag}:edge_index_u": captured["edge_index_u"].numpy(), f"{tag}:edge_preds_u": pu,
                        f"{tag}:orig_indices": captured["orig_indices"].numpy(),
                        f"{tag}:edge_index": go.edge_index.numpy(), f"{tag}:edge_preds": go.edge_preds.numpy(),
                        f"{tag}:max_abs_mask_logit": np.float64(captured["max_abs_mask_logit"])})
            if sq == "s":
                masks[tag] = node_preds
            else:
                rec[f"{tag}:node_preds_head"] = node_preds[:16]
                rec[f"{tag}:node_preds_sum"] = node_preds.astype(np.float64).sum(axis=(1, 2, 3))
            gap = np.abs(pu - 0.5)
            print("g17", tag, "nodes", node_preds.shape[0], "edges", inputs["edge_index"].shape[1], "kept", go.edge_index.shape[1],
                  "pairs within tol of 0.5:", near, "smallest gaps", np.sort(gap)[:2], "node preds", float(node_preds.min()),
                  float(node_preds.max()), "max |mask logit|", captured["max_abs_mask_logit"])
        if sq == "l":
            for name, mfd in (("tv_max", "max"), ("tv_3", 3)):
                row, col = G.get_time_valid_conn_ixs(torch.from_numpy(det["frame"]), mfd, use_cuda=False, return_undirected=False)
                rec[f"{name}:row"], rec[f"{name}:col"] = row.numpy(), col.numpy()
                rec[f"{name}:max_frame_dist"] = np.int64(-1 if mfd == "max" else mfd)
    np.savez_compressed(os.path.join(GOLD, "g17_window_tail.npz"), **rec)
    np.savez_compressed(os.path.join(GOLD, "g17_window_tail_masks.npz"), **{f"{tag}:node_preds": arr for tag, arr in masks.items()})


def _g19_score_graph(rng, frames, dets, p_edge, max_dist=None, tied=False):
    """Cross-frame pairs (row < col, detections ordered by frame) kept with probability p_edge; 35 % of the scores in (0.5, 1], the
    rest in [0, 0.5]; ``tied``: scores rounded to multiples of 1/8."""
    n = frames * dets
    frame = np.arange(n) // dets
    i, j = np.triu_indices(n, 1)
    ok = frame[i] != frame[j]
    if max_dist is not None:
        ok &= (frame[j] - frame[i]) <= max_dist
    ok &= rng.random(i.size) < p_edge
    ei = np.stack((i[ok], j[ok])).astype(np.int64)
    K = ei.shape[1]
    u = rng.random(K)
    p = np.where(rng.random(K) < 0.35, 0.5 + 0.5 * (1.0 - u), 0.5 * u).astype(np.float32)
    if tied:
        p = (np.round(p * 8) / 8).astype(np.float32)
    return ei, p, n


def _g19_stats(ei, p, n):
    """Violated out- / in-constraints of the thresholded scores, the in-constraints that the out-pass alone clears, and the
    arg-maxes (of either pass) that several edges attain -- plain numpy, for the generator's assertions."""
    rp = (p > np.float32(0.5)).astype(np.float32)
    v_out = int((np.bincount(ei[0][rp == 1], minlength=n) > 1).sum())
    v_in = int((np.bincount(ei[1][rp == 1], minlength=n) > 1).sum())
    ties = 0
    for side in (0, 1):
        if side == 1:
            still = int((np.bincount(ei[1][rp == 1], minlength=n) > 1).sum())
        for node in range(n):
            act = np.flatnonzero((ei[side] == node) & (rp == 1))
            if act.size > 1:
                ties += int((p[act] == p[act].max()).sum() > 1)
                rp[act] = 0
                rp[act[np.argmax(p[act])]] = 1
    return v_out, v_in, v_in - still, ties


def gen_g19():
    """GreedyProjector.project (tracker/projectors.py:19-67), MPNTracker._assign_ped_ids (tracker/mpn_tracker.py:231-248, called
    unbound on a namespace carrying full_graph) and Postprocessor.drop_short_trajectories (tracker/postprocessing.py:14-18,
    min_track_len 2 and 5) of the reference itself.  Inputs and outputs are stored per case, with the numbers of violated out- and
    in-constraints, of in-constraints the out-pass clears and of arg-maxes decided by edge id."""
    import pandas as pd
    EV, TR, PL = _import_tracking_stack()
    from mot_neural_solver.tracker import projectors as PJ
    from mot_neural_solver.tracker.postprocessing import Postprocessor
    rng = np.random.default_rng(19)
    cases = {}
    for tag, tied in (("a", False), ("b", False), ("t", True)):
        cases[tag] = _g19_score_graph(rng, 8, 6, 0.6, tied=tied)
    # the hub: a sparse background, one mid-sequence node joined to every node of every other frame with scores above 0.5
    ei, p, n = _g19_score_graph(rng, 130, 5, 0.3, max_dist=2)
    hub = 65 * 5 + 2
    others = np.array([v for v in range(n) if v // 5 != hub // 5], dtype=np.int64)
    hub_ei = np.stack((np.minimum(others, hub), np.maximum(others, hub)))
    background = ~((ei[0] == hub) | (ei[1] == hub))
    ei = np.concatenate((ei[:, background], hub_ei), axis=1)
    p = np.concatenate((p[background], (0.55 + 0.4 * rng.random(others.size)).astype(np.float32)))
    order = rng.permutation(ei.shape[1])
    cases["hub"] = (np.ascontiguousarray(ei[:, order]), p[order], n)
    z = np.load(os.path.join(GOLD, "g17_window_tail.npz"))
    for tag in ("s1", "s2", "l1", "l2"):
        cases["g17_" + tag] = (z[f"{tag}:edge_index"], z[f"{tag}:edge_preds"], int(z[f"{tag[0]}:frame"].shape[0]))
    rec = {"cases": np.array(list(cases))}
    for tag, (ei, p, n) in cases.items():
        assert (ei[0] < ei[1]).all() and p.dtype == np.float32
        graph_obj = _GeoData(edge_index=torch.from_numpy(ei), edge_preds=torch.from_numpy(p).clone())
        graph_obj.num_nodes = n
        df = pd.DataFrame({"frame": np.arange(n) // 5})
        full_graph = types.SimpleNamespace(graph_obj=graph_obj, graph_df=df)
        proj = PJ.GreedyProjector(full_graph)
        proj.project()
        round_preds = graph_obj.edge_preds.numpy().copy()
        rate = np.float32(proj.constr_satisf_rate)
        assert float(rate) == proj.constr_satisf_rate or np.isnan(rate)
        graph_obj.edge_preds, graph_obj.edge_index = round_preds, ei     # (graph_obj.numpy() of _project_graph_model_output)
        me = types.SimpleNamespace(full_graph=full_graph)
        TR.MPNTracker._assign_ped_ids(me)
        labels = np.asarray(me.final_projected_output["ped_id"], dtype=np.int64)
        rec.update({f"{tag}:edge_index": ei, f"{tag}:edge_preds": p, f"{tag}:num_nodes": np.int64(n), f"{tag}:round_preds": round_preds,
                    f"{tag}:constr_satisf_rate": rate, f"{tag}:ped_ids": labels})
        for mtl in (2, 5):
            pp = Postprocessor(me.final_projected_output.copy(), None, {"min_track_len": mtl})
            pp.drop_short_trajectories()
            keep = np.zeros(n, dtype=bool)
            keep[pp.traj_df.index.to_numpy()] = True
            rec[f"{tag}:keep{mtl}"] = keep
        stats = _g19_stats(ei, p, n)
        rec[f"{tag}:stats"] = np.array(stats, np.int64)
        if not tag.startswith("g17"):
            assert min(stats[:3]) >= 10, (tag, stats)
        if tag == "t":
            assert stats[3] >= 1 and (p == 0.5).any(), (tag, stats)
        if tag == "hub":
            act = p > 0.5
            assert int((act & (ei[0] == hub)).sum()) > 256 and int((act & (ei[1] == hub)).sum()) > 256
        print("g19", tag, "nodes", n, "edges", ei.shape[1], "violated out / in, cleared by the out-pass, ties:", stats, "rate", float(rate),
              "active after", int(round_preds.sum()), "tracks", int(labels.max()) + 1, "kept (2, 5)", int(rec[f"{tag}:keep2"].sum()),
              int(rec[f"{tag}:keep5"].sum()))
    np.savez_compressed(os.path.join(GOLD, "g19_projection.npz"), **rec)


def gen_g14():
    """MOTGraph._get_edge_ixs + construct_graph_object (data/mot_graph.py:195-218, 283-317) of the reference itself, on synthetic
    detections with the appearance data supplied directly (``_load_appearance_data`` replaced: it reads image crops / .pt files,
    the rows before and after this path): training mode (kNN pruning inside, reciprocal and not) and inference mode (all
    time-valid pairs + reid_emb_dists), 'max' and bounded frame distances.  The MOTGraph is built without its __init__ (which
    slices a sequence data frame): the attributes construct_graph_object reads are set by hand."""
    _import_tracking_stack()
    import pandas as pd
    from mot_neural_solver.data import mot_graph as MG
    from mot_neural_solver.utils import graph as G
    # (the reference moves the index computation to 'cuda' in inference mode: keep it on the CPU here)
    real_tv, real_knn, real_feats = G.get_time_valid_conn_ixs, G.get_knn_mask, G.compute_edge_feats_dict
    MG.get_time_valid_conn_ixs = lambda **kw: real_tv(**dict(kw, use_cuda=False))
    MG.get_knn_mask = lambda **kw: real_knn(**dict(kw, use_cuda=False))
    MG.compute_edge_feats_dict = lambda **kw: real_feats(**dict(kw, use_cuda=False))
    names = ["secs_time_dists", "norm_feet_x_dists", "norm_feet_y_dists", "bb_height_dists", "bb_width_dists", "emb_dist"]
    rec = {}
    cases = [("train_recip", False, 5, True, "max"), ("train_plain", False, 4, False, 6), ("infer", True, 5, True, "max"),
             ("infer_mfd", True, None, True, 4)]
    for tag, inference, top_k, recip, mfd in cases:
        det = synth.make_detections(frames=10, dets_lo=3, dets_hi=7, seed=21, emb_dim=32, node_in_dim=64, frame_stride=2)
        n = det["frame"].shape[0]
        df = pd.DataFrame({k: det[k] for k in ("frame", "bb_height", "bb_width", "feet_x", "feet_y")})
        df["frame_path"] = "synthetic/img1/000001.jpg"
        mg = object.__new__(MG.MOTGraph)
        mg.graph_df = df
        mg.max_frame_dist = mfd
        mg.inference_mode = inference
        mg.seq_info_dict = {"fps": 25.0}
        mg.dataset_params = {"top_k_nns": top_k, "reciprocal_k_nns": recip, "edge_feats_to_use": names}
        emb = torch.from_numpy(det["reid"])
        mg._load_appearance_data = lambda emb=emb, det=det, n=n: (emb, torch.from_numpy(det["x"]).view(n, 64, 1, 1), None)
        mg.construct_graph_object()
        go = mg.graph_obj
        rec.update({f"{tag}:frame": det["frame"], f"{tag}:bb_height": det["bb_height"], f"{tag}:bb_width": det["bb_width"],
                    f"{tag}:feet_x": det["feet_x"], f"{tag}:feet_y": det["feet_y"], f"{tag}:reid": det["reid"],
                    f"{tag}:edge_index": go.edge_index.numpy(), f"{tag}:edge_attr": go.edge_attr.numpy(),
                    f"{tag}:cfg": np.array([int(inference), -1 if top_k is None else top_k, int(recip), -1 if mfd == "max" else mfd], np.int64)})
        if inference:
            rec[f"{tag}:reid_emb_dists"] = go.reid_emb_dists.numpy()
        print("g14", tag, "nodes", n, "edges", go.edge_index.shape[1])
    np.savez_compressed(os.path.join(GOLD, "g14_construct_graph.npz"), **rec)


def gen_g20():
    """The tail of MPNTracker._to_full_masks (tracker/mpn_tracker.py:284-297) per frame: paste_masks_in_image as
    tests/full_masks_ref.py restates it literally (torchvision is not installed; the resize is torch's own F.interpolate on the
    CPU), then the reference's OWN ensure_unique_masks (utils/mots.py:5-25) and the threshold of 0.5.  pycocotools is not installed
    either: the strings are the restated codec's, which the sample line of the MOTS evaluation kit's README (stored with its
    height and width) pins -- it decodes to counts that sum to height x width and encodes back to the same characters."""
    _import_tracking_stack()
    from mot_neural_solver.utils.mots import ensure_unique_masks
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import full_masks_ref as R
    rng = np.random.default_rng(20)
    H, W, thr = 96, 128, 0.5
    per_frame = [6, 1, 4]
    n = sum(per_frame)
    masks = R.blob_masks(rng, n)
    boxes = R.random_boxes(rng, n, H, W, lo=10.0, hi=90.0)
    boxes[0] = (20.25, 10.5, 70.75, 80.0)           # two large overlapping boxes in the first frame
    boxes[1] = (40.0, 25.0, 110.5, 95.75)
    frame_ptr = np.concatenate(([0], np.cumsum(per_frame))).astype(np.int32)
    bits, strings, shapes = [], [], []
    for f in range(len(per_frame)):
        a, b = int(frame_ptr[f]), int(frame_ptr[f + 1])
        frame_masks = R.literal_paste(masks[a:b], boxes[a:b], H, W)
        frame_masks = ensure_unique_masks(frame_masks)
        frame_masks = np.where(frame_masks >= thr, 1, 0).astype(np.uint8)
        assert frame_masks.sum(axis=0).max() <= 1
        for m in frame_masks:
            counts = R.np_rle_counts(m)
            assert sum(counts) == H * W
            strings.append(R.np_rle_string(counts))
            assert R.np_rle_from_string(strings[-1]) == counts
        bits.append(np.packbits(frame_masks.reshape(-1)))
        shapes.append(frame_masks.shape[0])
    readme = open("/root/reference/MOTChallengeEvalKit/src/MOTChallengeEvalKit/MOTS/README.md").read().splitlines()[66].split()
    assert len(readme) == 6 and readme[1] == "1005"
    sample, sh, sw = readme[5], int(readme[3]), int(readme[4])
    sample_counts = R.np_rle_from_string(sample)
    assert sum(sample_counts) == sh * sw and min(sample_counts) >= 0 and R.np_rle_string(sample_counts) == sample
    rec = {"masks": masks, "boxes": boxes, "frame_ptr": frame_ptr, "img_shape": np.array([H, W], np.int64),
           "mask_threshold": np.float32(thr), "binary_bits": np.concatenate(bits), "rle": np.array(strings),
           "sample_rle": np.array(sample), "sample_shape": np.array([sh, sw], np.int64)}
    covered = int(np.unpackbits(rec["binary_bits"]).sum())
    print("g20: masks per frame", shapes, "set pixels", covered, "string lengths", [len(s) for s in strings], "sample counts",
          len(sample_counts))
    assert covered > 2000 and min(len(s) for s in strings) >= 1
    np.savez_compressed(os.path.join(GOLD, "g20_full_masks.npz"), **rec)


def _real_scatter_min(src, index, dim=-1, out=None, dim_size=None):
    """torch_scatter.scatter_min for 1-D inputs: (min, arg) with arg = src.numel() for an empty segment -- the position of the
    -1 the reference appends (data/mot_graph.py:246-248).  Ties: the first position (they cannot change a label: equal
    distances on one side of a row are stored duplicates of ONE edge, and the reference compares node ids, not positions)."""
    assert src.dim() == 1 and index.shape == src.shape
    n = int(dim_size)
    mn = torch.full((n,), torch.iinfo(src.dtype).max, dtype=src.dtype)
    arg = torch.full((n,), src.numel(), dtype=torch.long)
    for j in range(src.numel() - 1, -1, -1):
        i = int(index[j])
        if src[j] <= mn[i]:
            mn[i], arg[i] = src[j], j
    return mn, arg


def gen_g21():
    """The reference's OWN MOTGraph.assign_edge_labels (data/mot_graph.py:223-262, unbound on a namespace) and
    MOTNeuralSolver._compute_loss (pl_module/pl_module.py:88-120) with autograd; inputs from tests/training_targets_ref.py."""
    EV, TR, PL = _import_tracking_stack()
    import pandas as pd
    from mot_neural_solver.data import mot_graph as MG
    MG.scatter_min = _real_scatter_min   # (mot_graph.py binds the name at import; the shim's raises)
    mpn = import_reference()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import training_targets_ref as R
    rec = {}

    def ref_labels(ei, ids, mode):
        x = torch.zeros((len(ids), 1))
        ns = types.SimpleNamespace(dataset_params={"true_edge_labels": mode}, graph_df=pd.DataFrame({"id": np.asarray(ids, np.int64)}),
                                   graph_obj=_GeoData(edge_index=torch.from_numpy(np.ascontiguousarray(ei)), x=x))
        MG.MOTGraph.assign_edge_labels(ns)
        return ns.graph_obj.edge_labels.numpy().astype(np.float32)

    # ---- label cases
    g = synth.make_graph(48, 400, T=8, seed=21, node_in_dim=4)
    ids = R.track_ids(g["frame"], 21)
    ei = g["edge_index"]
    lab_all, lab_cl = ref_labels(ei, ids, "all"), ref_labels(ei, ids, "closest")
    # what the case is for: unmatched nodes, gaps of >= 2 frames inside a track, and a node whose nearest same-id detection in time
    # has no edge to it while a farther one has
    assert (ids == -1).any()
    fr = g["frame"]
    assert any(np.diff(np.unique(fr[ids == t])).max() >= 2 for t in np.unique(ids[ids >= 0]) if (ids == t).sum() > 1)
    skipped = 0
    for n in range(48):
        later = [m for m in range(n + 1, 48) if ids[m] == ids[n] and ids[n] != -1]
        cols = set(ei[1][(ei[0] == n)].tolist())
        if later and later[0] not in cols and any(m in cols for m in later[1:]):
            skipped += 1
    assert skipped >= 1 and 0 < lab_cl.sum() < lab_all.sum()
    cases = {"base": (ei, ids)}
    act = np.nonzero(lab_cl == 1)[0][:3]
    oth = np.nonzero(lab_cl == 0)[0][:3]
    real = np.nonzero(ids >= 0)[0][[0, 5, 11, 17]]
    cases["dups"] = (np.concatenate([ei, ei[:, act], ei[:, oth], np.stack([real, real])], axis=1), ids)
    cases["unique"] = (ei, np.arange(48, dtype=np.int64))
    cases["one"] = (np.array([[0], [1]], np.int64), np.array([3, 3], np.int64))
    cases["none"] = (np.zeros((2, 0), np.int64), np.array([3, 3, -1], np.int64))
    gs = [synth.make_graph(20, 120, T=5, seed=30 + i, node_in_dim=4) for i in range(3)]
    b = synth.batch_graphs(gs)
    cases["batch"] = (b["edge_index"], np.concatenate([R.track_ids(x["frame"], 33 + i) for i, x in enumerate(gs)]))
    gb = synth.make_graph(300, 3000, T=12, seed=23, node_in_dim=4)
    cases["big"] = (gb["edge_index"], R.track_ids(gb["frame"], 24))
    assert tuple(cases) == R.LABEL_CASES
    for tag, (e, i) in cases.items():
        rec[f"lab:{tag}:edge_index"], rec[f"lab:{tag}:ids"] = e.astype(np.int64), i.astype(np.int64)
        for mode in R.MODES:
            rec[f"lab:{tag}:{mode}"] = ref_labels(e, i, mode)
            assert np.array_equal(rec[f"lab:{tag}:{mode}"], R.edge_labels(e, i, mode)), (tag, mode)
    assert rec["lab:dups:all"][-4:].sum() == 4 and rec["lab:dups:closest"][-4:].sum() == 0 and rec["lab:dups:closest"][400:403].sum() == 3
    assert rec["lab:unique:all"].sum() == 0 and rec["lab:big:closest"].sum() > 0

    # ---- loss cases
    solver = types.SimpleNamespace(hparams={"train_params": {"loss_weights": dict(R.LOSS_WEIGHTS)}})

    def ref_loss(logits, labels, preds, mlab, valid):
        k = logits.shape[0]
        lg = torch.from_numpy(logits).clone().requires_grad_(True)
        pr = [torch.from_numpy(np.ascontiguousarray(preds[s])).clone().requires_grad_(True) for s in range(k)]
        outputs = {"classified_edges": [lg[s].view(-1, 1) for s in range(k)], "mask_predictions": pr}
        batch = types.SimpleNamespace(edge_labels=torch.from_numpy(labels), mask_labels=torch.from_numpy(mlab),
                                      mask_gt_ixs=torch.from_numpy(valid))
        return PL.MOTNeuralSolver._compute_loss(solver, outputs, batch), lg, pr

    def store_mask_grads(tag, grads, valid):
        rows = R.sample_rows(valid)
        rec[f"{tag}:gmask_rows"] = np.stack([gm[rows] for gm in grads])
        rec[f"{tag}:gmask_norm"] = np.array([np.sqrt((gm.astype(np.float64) ** 2).sum()) for gm in grads])
        rec[f"{tag}:gmask_row_abssum"] = np.stack([np.abs(gm.astype(np.float64)).reshape(gm.shape[0], -1).sum(axis=1) for gm in grads])

    for tag in R.LOSS_CASES:
        logits, labels, preds, mlab, valid = R.loss_inputs(tag)
        loss, lg, pr = ref_loss(logits, labels, preds, mlab, valid)
        loss.backward()
        grads = [p_.grad.numpy() if p_.grad is not None else np.zeros(p_.shape, np.float32) for p_ in pr]
        if tag == "novalid":
            assert all(p_.grad is None for p_ in pr)
        if tag == "extreme":
            assert float(np.abs(preds).max()) >= 80.0
        rec[f"{tag}:loss"], rec[f"{tag}:glogits"] = np.float64(float(loss.detach())), lg.grad.numpy()
        store_mask_grads(tag, grads, valid)
    # the graphs variant: the reference called once per graph, the losses averaged (g16's recipe)
    logits, labels, preds, mlab, valid, node_graph, edge_graph = R.graph_inputs()
    k = logits.shape[0]
    lg = torch.from_numpy(logits).clone().requires_grad_(True)
    pr = torch.from_numpy(preds).clone().requires_grad_(True)
    total, per_graph = 0, []
    for i in range(3):
        er, nr = edge_graph == i, node_graph == i
        outputs = {"classified_edges": [lg[s][torch.from_numpy(er)].view(-1, 1) for s in range(k)],
                   "mask_predictions": [pr[s][torch.from_numpy(nr)] for s in range(k)]}
        batch = types.SimpleNamespace(edge_labels=torch.from_numpy(labels[er]), mask_labels=torch.from_numpy(mlab[nr]),
                                      mask_gt_ixs=torch.from_numpy(valid[nr]))
        li = PL.MOTNeuralSolver._compute_loss(solver, outputs, batch)
        per_graph.append(float(li.detach()))
        total = total + li
    loss = total / 3
    loss.backward()
    rec["graphs:loss"], rec["graphs:per_graph"], rec["graphs:glogits"] = np.float64(float(loss.detach())), np.array(per_graph), lg.grad.numpy()
    store_mask_grads("graphs", [pr.grad[s].numpy() for s in range(k)], valid)

    # ---- end to end: g6's model, graph and weights under the reference's own loss
    N, E, L, nin = 40, 360, 3, 64
    params = synth.model_params(32, L, "sum", num_class_steps=2, node_in_dim=nin)
    W = synth.make_weights(params, seed=7)
    W.update(synth.make_mask_weights(seed=17))
    full = dict(params)
    full.update(MASK_PARAMS)
    model = mpn.MOTMPNet(full)
    model.load_state_dict({k_: torch.from_numpy(v) for k_, v in W.items()}, strict=True)
    g = synth.make_graph(N, E, T=8, seed=4, node_in_dim=nin)
    d = Data()
    d.x = torch.from_numpy(g["x"]).view(N, nin, 1, 1)
    d.x_ext = torch.from_numpy(synth.normal(5, (N, 256, 14, 14), stream=1, std=0.5))
    d.edge_index = torch.from_numpy(g["edge_index"])
    d.edge_attr = torch.from_numpy(g["edge_attr"])
    ids = R.track_ids(g["frame"], 6)
    d.edge_labels = torch.from_numpy(ref_labels(g["edge_index"], ids, "closest"))
    assert float(d.edge_labels.sum()) >= 4
    d.mask_labels = torch.from_numpy((synth.uniform01(65, N * 56 * 56).reshape(N, 1, 56, 56) < 0.4).astype(np.float32))
    valid = R.first_valid(25, N)
    d.mask_gt_ixs = torch.from_numpy(valid)
    out = model(d)
    loss = PL.MOTNeuralSolver._compute_loss(solver, out, d)
    names = [k_ for k_ in W if k_.startswith(("encoder.", "MPNet.", "classifier."))] + ["MPAttentionNet.node_model.layers.0.weight",
                                                                                      "mask_predictor.mask_head.layers.0.bias"]
    pd_ = dict(model.named_parameters())
    grads = torch.autograd.grad(loss, [pd_[k_] for k_ in names])
    rec.update({"e2e:ids": ids, "e2e:edge_labels": d.edge_labels.numpy(), "e2e:loss": np.float64(float(loss.detach()))})
    for k_, gr in zip(names, grads):
        a = gr.numpy()
        rec["e2e:G:" + k_] = a if a.size < 20000 else a.reshape(-1)[:20000]
        rec["e2e:Gn:" + k_] = np.float64(np.sqrt((a.astype(np.float64) ** 2).sum()))
    path = os.path.join(GOLD, "g21_training_targets.npz")
    np.savez_compressed(path, **rec)
    print("g21 ok:", {k_: round(float(v), 6) for k_, v in rec.items() if k_.endswith(":loss")}, "positives",
          {t: (int(rec[f"lab:{t}:all"].sum()), int(rec[f"lab:{t}:closest"].sum())) for t in R.LABEL_CASES}, "skipped-nearest nodes", skipped,
          "bytes", os.path.getsize(path))


# ------------------------------------------------------------------ g22: the MOTS evaluation kit
def _install_pycocotools_standin():
    """``pycocotools.mask`` as the kit uses it (area, merge, iou with the crowd flag) in numpy over the project's codec
    (mpntrackseg_amd.masks): a mask is {'size': [h, w], 'counts': bytes}.  As in the C library, merging no masks gives a 0 x 0
    mask, and iou is -1 for masks of different sizes -- so a frame without ignore rows ignores nothing."""
    from mpntrackseg_amd import masks as M

    def decode(m):
        h, w = m["size"]
        if h * w == 0:
            return np.zeros((h, w), bool)
        c = m["counts"]
        return M.rle_to_mask(c.decode("ascii") if isinstance(c, bytes) else c, h, w).astype(bool)

    def encode(mask):
        h, w = mask.shape
        flat = mask.T.reshape(-1).astype(np.int8)
        edges = np.flatnonzero(np.diff(np.concatenate(([0], flat, [0]))))
        return {"size": [h, w], "counts": M.rle_string(M.rle_counts_from_events(edges[edges < h * w], h * w)).encode("ascii")}

    def area(m):
        return [int(decode(x).sum()) for x in m] if isinstance(m, list) else int(decode(m).sum())

    def merge(ms, intersect=False):
        if len(ms) == 0:
            return {"size": [0, 0], "counts": b""}
        out = decode(ms[0])
        for x in ms[1:]:
            out = (out & decode(x)) if intersect else (out | decode(x))
        return encode(out)

    def iou(dt, gt, iscrowd):
        if len(dt) == 0 or len(gt) == 0:
            return []
        out = np.zeros((len(dt), len(gt)), np.float64)
        for g, gm in enumerate(gt):
            G = decode(gm)
            for d, dm in enumerate(dt):
                D = decode(dm)
                if D.shape != G.shape:
                    out[d, g] = -1.0
                    continue
                i = np.float64((D & G).sum())
                u = np.float64(D.sum()) if iscrowd[g] else np.float64(D.sum()) + np.float64(G.sum()) - i
                with np.errstate(invalid="ignore", divide="ignore"):
                    out[d, g] = i / u
        return out

    pkg, mod = types.ModuleType("pycocotools"), types.ModuleType("pycocotools.mask")
    mod.area, mod.merge, mod.iou, mod.decode, mod.encode = area, merge, iou, decode, encode
    pkg.mask = mod
    sys.modules["pycocotools"], sys.modules["pycocotools.mask"] = pkg, mod


def _g22_rect(img, f, obj, y0, y1, x0, x1):
    assert (img[f, y0:y1, x0:x1] == 0).all(), (f, obj)   # masks of a frame are disjoint
    img[f, y0:y1, x0:x1] = obj


def _g22_cases():
    """12 frames of 37 x 29, every case of the metric at least once (the asserts of gen_g22 check that they are there)"""
    F, H, W = 12, 37, 29
    gt, pr = np.zeros((F, H, W), np.uint16), np.zeros((F, H, W), np.uint16)
    jit = (synth.uniform01(22, 4 * F * 2, stream=1) * 2).astype(np.int64).reshape(4, F, 2)   # prediction offsets in {0, 1}
    for f in range(F):
        if f in (0, 1, 2, 3, 4, 5, 8, 9):
            _g22_rect(gt, f, 10000, 0, H, 22, W)                      # the ignore region (none in frames 6, 7, 10, 11)
        if f <= 9:                                                    # 2001: tracked throughout, the prediction changes its id
            _g22_rect(gt, f, 2001, 2, 10, 2, 7)
            dy, dx = jit[0, f]
            if f == 2:                                                # ... and once reaches into a second ignore patch, still matched
                _g22_rect(gt, f, 10001, 2, 10, 7, 9)
                _g22_rect(pr, f, 2001, 2, 10, 2, 9)
            else:
                _g22_rect(pr, f, 2001 if f < 6 else 2007, 2 + dy, 10 + dy, 2 + dx, 7 + dx)
            _g22_rect(gt, f, 2002, 14, 22, 2, 7)                      # 2002: missed in frames 3-5 and 8-9 (a fragment; partly tracked)
            if f in (0, 1, 2, 6, 7):
                dy, dx = jit[1, f]
                _g22_rect(pr, f, 2002, 14 + dy, 22 + dy, 2 + dx, 7 + dx)
        if 2 <= f <= 7:
            _g22_rect(gt, f, 2003, 26, 34, 2, 7)                      # 2003: never found
        if f in (0, 1, 8, 9):                                         # 2004: leaves and comes back
            dy, dx = jit[2, f]
            _g22_rect(gt, f, 2004, 2, 10, 10, 15)
            _g22_rect(pr, f, 2004, 2 + dy, 10 + dy, 10 + dx, 15 + dx)
        if f in (4, 5):                                               # 2005: IoU exactly 4 / 8 in frame 4, found in frame 5
            _g22_rect(gt, f, 2005, 14, 17, 10, 12)
            _g22_rect(pr, f, 2005, 15 if f == 4 else 14, 18 if f == 4 else 17, 10, 12)
        if f == 1:
            _g22_rect(pr, f, 2009, 26, 32, 20, 26)                    # four of six columns inside the ignore region
        if f in (3, 10):
            _g22_rect(pr, f, 2008, 26, 30, 12, 16)                    # a false positive; frame 10 has no ground truth at all
        if f == 6:
            _g22_rect(gt, f, 1001, 26, 32, 12, 18)                    # a car under a prediction
            _g22_rect(pr, f, 2010, 26, 32, 12, 18)
        if f == 11:
            _g22_rect(gt, f, 2006, 5, 10, 5, 10)                      # a frame without predictions
    return gt, pr, 12   # seqlength 12: frame 12 is empty on both sides


def _g22_crowded(n_obj=110):
    """3 frames of 64 x 48: a 16 x 12 grid of 4 x 4 cells; n_obj cells hold a ground-truth object and a prediction (random
    sub-rectangles of the cell), 5 a prediction alone, 3 an ignore patch (one with a prediction inside)"""
    F, H, W, C = 3, 64, 48, 4
    cells = (H // C) * (W // C)
    gt, pr = np.zeros((F, H, W), np.uint16), np.zeros((F, H, W), np.uint16)
    for f in range(F):
        perm = np.argsort(synth.splitmix64(22, cells, stream=10 + f), kind="stable")
        u = (synth.uniform01(22, cells * 8, stream=20 + f).reshape(cells, 8) * 2).astype(np.int64)   # {0, 1}

        def sub(cell, k):   # rows / columns [a, b) of a sub-rectangle of the cell, at least 2 x 2
            y, x = (cell // (W // C)) * C, (cell % (W // C)) * C
            return y + u[cell, k], y + C - u[cell, k + 1], x + u[cell, k + 2], x + C - u[cell, k + 3]
        for k in range(n_obj):
            _g22_rect(gt, f, 2001 + k, *sub(perm[k], 0))
            pid = 2001 + (k ^ 1 if (f == 1 and k < 20) else k)       # twenty pairs swap their ids in the middle frame
            _g22_rect(pr, f, pid, *sub(perm[k], 4))
        for k in range(n_obj, n_obj + 5):
            _g22_rect(pr, f, 2001 + k + 100, *sub(perm[k], 4))
        for j, k in enumerate(range(n_obj + 5, n_obj + 8)):
            y, x = (perm[k] // (W // C)) * C, (perm[k] % (W // C)) * C
            _g22_rect(gt, f, 10000 + j, y, y + C, x, x + C)
            if j == 0:
                _g22_rect(pr, f, 2001 + k + 100, *sub(perm[k], 4))
    return gt, pr, F - 1


def gen_g22():
    """The MOTS evaluation kit's OWN MOTSMetrics.compute_metrics_per_sequence + compute_clearmot
    (MOTChallengeEvalKit/MOTS/MOTS_metrics.py) on text files written from id images.  Two stand-ins: collections.Iterable
    (Metrics.py:2 predates Python 3.10) and a numpy pycocotools.mask (_install_pycocotools_standin) -- so the fixture rests on
    the project's RLE codec (mpntrackseg_amd.masks, pinned by g20's sample line) for decoding the masks.  Per-frame counts are
    differences of the kit's totals over the sequence cut after every frame; the matched-id sequences are read off the calls
    of its overlap function."""
    import collections
    import collections.abc
    import tempfile
    collections.Iterable = collections.abc.Iterable
    _install_pycocotools_standin()
    sys.path.insert(0, "/root/reference/MOTChallengeEvalKit/src")
    from MOTChallengeEvalKit.MOTS import MOTS_metrics as MM
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import mots_metrics_ref as R

    loaded = []
    kit_load = MM.load_txt

    def keeping_load(path):
        loaded.append(kit_load(path))
        return loaded[-1]
    MM.load_txt = keeping_load

    def run(rows_gt, rows_pr, seq_length):
        matched = {}

        def overlap(a, b, criterion="union"):
            c = MM.mask_iou(a, b, criterion)
            if criterion == "union" and c > 0.5:
                matched[id(a)] = b.track_id
            return c
        del loaded[:]
        with tempfile.TemporaryDirectory() as d:
            R.write_txt(os.path.join(d, "gt.txt"), rows_gt)
            R.write_txt(os.path.join(d, "pred.txt"), rows_pr)
            with open(os.path.join(d, "seqinfo.ini"), "w") as fh:
                fh.write("[Sequence]\nname=g22\nseqlength=%d\n" % seq_length)
            m = MM.MOTSMetrics("g22")
            m.compute_metrics_per_sequence("g22", os.path.join(d, "pred.txt"), os.path.join(d, "gt.txt"), d, "MOTS",
                                           overlap_function=overlap)
            m.compute_clearmot()
        seqs = collections.OrderedDict()
        for f in sorted(loaded[0]):
            for obj in loaded[0][f]:
                if obj.class_id == MM.CLASS_ID and f <= seq_length:
                    seqs.setdefault(obj.track_id, []).append(matched.get(id(obj), -1))
        return m, seqs

    rec = {}
    for name, (gt, pr, seq_length) in (("cases", _g22_cases()), ("crowded", _g22_crowded())):
        rows_gt, rows_pr = R.id_image_rows(gt), R.id_image_rows(pr)
        m, seqs = run(rows_gt, rows_pr, seq_length)
        cum = np.zeros((seq_length + 2, 4), np.int64)
        for f in range(seq_length + 1):   # the kit over the frames 0 .. f alone
            cut = lambda rows: [r for r in rows if int(r.split(" ")[0]) <= f]
            mf, _ = run(cut(rows_gt), cut(rows_pr), f)
            cum[f + 1] = (mf.tp, mf.fp, mf.fn, mf.n_itr)
        assert tuple(cum[-1]) == (m.tp, m.fp, m.fn, m.n_itr)
        rec[f"{name}:gt"], rec[f"{name}:pred"], rec[f"{name}:seq_length"] = gt, pr, np.int64(seq_length)
        rec[f"{name}:per_frame"] = np.diff(cum, axis=0)
        for k in m.names:
            rec[f"{name}:m:{k}"] = np.float64(getattr(m, k))
        gt_ids = sorted(seqs)
        rec[f"{name}:traj_ids"] = np.asarray(gt_ids, np.int64)
        rec[f"{name}:traj_ptr"] = np.concatenate(([0], np.cumsum([len(seqs[i]) for i in gt_ids]))).astype(np.int64)
        rec[f"{name}:traj_matched"] = np.asarray([v for i in gt_ids for v in seqs[i]], np.int64)
        print("g22", name, {k: getattr(m, k) for k in ("sMOTSA", "MOTSA", "MOTSP", "IDF1", "tp", "fp", "fn", "n_itr", "id_switches",
                                                       "fragments", "MT", "PT", "ML", "IDTP")})
        if name == "cases":
            assert m.id_switches >= 1 and m.fragments >= 1 and m.fn >= 1 and m.fp >= 1 and m.n_itr >= 1 and min(m.MT, m.PT, m.ML) >= 1
            L = R.scene_lists(gt, pr)
            t, tp = R.label_overlap(L["labels_a"], L["labels_b"], L["a_ptr"], L["b_ptr"])
            o = R.frame_match(t, tp, L["a_ptr"], L["b_ptr"], L["a_ignore"], L["a_traj"], L["b_traj"], L["n_a_traj"], L["n_b_traj"])
            assert o["id_match"].sum() == m.tp + 1                       # the pair at IoU exactly 0.5
            assert (o["b_ignored"] & ~o["b_matched"]).sum() == m.n_itr
            assert seqs[2004] == [2004] * 4 and seqs[2003] == [-1] * 6   # back after a gap; never found
        else:
            assert all(min(len(np.unique(gt[f])), len(np.unique(pr[f]))) > 100 for f in range(gt.shape[0]))
    MM.load_txt = kit_load
    path = os.path.join(GOLD, "g22_mots_metrics.npz")
    np.savez_compressed(path, **rec)
    print("g22 bytes", os.path.getsize(path))


# ------------------------------------------------------------------ g23: TrackEval's HOTA on KITTI-MOTS
def _g23_association():
    """12 frames of 37 x 29 (and an empty thirteenth timestep); the asserts of gen_g23 check that the cases are there"""
    F, H, W = 12, 37, 29
    gt, pr = np.zeros((F, H, W), np.uint16), np.zeros((F, H, W), np.uint16)
    jit = (synth.uniform01(23, 3 * F * 2, stream=1) * 3).astype(np.int64).reshape(3, F, 2)   # prediction offsets in {0, 1, 2}
    for f in range(10):
        if f <= 5:
            _g22_rect(gt, f, 10000, 0, H, 24, W)                      # the ignore region
        _g22_rect(gt, f, 2001, 2, 10, 1, 5)                           # 2001: covered by prediction 2001, then by 2002
        _g22_rect(pr, f, 2001 if f < 5 else 2002, 2 + jit[0, f, 0], 10 + jit[0, f, 0], 0 + jit[0, f, 1], 4 + jit[0, f, 1])
        _g22_rect(gt, f, 2003, 13, 21, 1, 5)                          # 2003 / 2004: their predictions swap ids from frame 5 on
        _g22_rect(gt, f, 2004, 25, 33, 1, 5)
        _g22_rect(pr, f, 2003 if f < 5 else 2004, 13 + jit[1, f, 0], 21 + jit[1, f, 0], 0 + jit[1, f, 1], 4 + jit[1, f, 1])
        _g22_rect(pr, f, 2004 if f < 5 else 2003, 25 + jit[2, f, 0], 33 + jit[2, f, 0], 0 + jit[2, f, 1], 4 + jit[2, f, 1])
        _g22_rect(gt, f, 2005, 2, 12, 7, 12)                          # 2005 / 2006: found exactly by 2011 / 2010 ...
        _g22_rect(gt, f, 2006, 14, 24, 7, 12)
        if f != 7:
            _g22_rect(pr, f, 2011, 2, 12, 7, 12)
            _g22_rect(pr, f, 2010, 14, 24, 7, 12)
        else:                                                         # ... but once 2010 alone lies over both: 35 / 90 and 30 / 95
            _g22_rect(pr, f, 2010, 5, 20, 7, 12)
        _g22_rect(gt, f, 2007, 2, 22, 15, 16)                         # two strips of 20 pixels with f + 1 and f + 10 of them found:
        _g22_rect(pr, f, 2007, 2, 3 + f, 15, 16)                      # IoU = every twentieth from 0.05 to 0.95
        _g22_rect(gt, f, 2008, 2, 22, 18, 19)
        _g22_rect(pr, f, 2008, 2, 12 + f, 18, 19)
    _g22_rect(pr, 1, 2020, 26, 32, 22, 28)                            # four of six columns inside the ignore region: removed
    _g22_rect(pr, 2, 2021, 26, 32, 22, 26)                            # two of four: exactly half, kept
    _g22_rect(gt, 6, 1001, 26, 32, 20, 26)                            # a car under a prediction
    _g22_rect(pr, 6, 2030, 26, 32, 20, 26)
    _g22_rect(pr, 10, 2002, 2, 10, 1, 5)                              # frame 10 has no ground truth,
    _g22_rect(pr, 10, 2010, 14, 24, 7, 12)
    _g22_rect(gt, 11, 2001, 2, 10, 1, 5)                              # frame 11 no prediction
    _g22_rect(gt, 11, 2005, 2, 12, 7, 12)
    return gt, pr, F + 1


def gen_g23():
    """TrackEval's OWN KittiMOTS._load_raw_file / get_preprocessed_seq_data and HOTA.eval_sequence / combine_sequences on text
    files written from id images, in the KittiMOTS folder layout.  Stand-ins: the numpy pycocotools.mask of g22 and the aliases
    np.float / np.bool / np.int where numpy no longer has them.  The prediction ids the preprocessing keeps are read off its call
    of _calculate_mask_ious for the ignore region."""
    import tempfile
    for name, t in (("float", float), ("bool", bool), ("int", int)):
        if not hasattr(np, name):
            setattr(np, name, t)
    _install_pycocotools_standin()
    # a frame without ignore rows: the merged region is a 0 x 0 mask.  The C library compares bounding boxes first and leaves 0
    # where they do not meet, so it never reaches the size check the stand-in answers with -1 (which the kit's range assertion
    # refuses)
    standin_iou = sys.modules["pycocotools.mask"].iou
    sys.modules["pycocotools.mask"].iou = lambda dt, gt, iscrowd: np.maximum(standin_iou(dt, gt, iscrowd), 0.0)
    sys.path.insert(0, "/root/reference/TrackEval")
    import trackeval
    from trackeval.metrics import hota as hota_module
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import mots_metrics_ref as R
    eps = np.finfo("float").eps
    real_lsa = hota_module.linear_sum_assignment

    def run(gt, pr, num_timesteps, noise_seed=None):
        ds = trackeval.datasets.KittiMOTS.__new__(trackeval.datasets.KittiMOTS)
        removed = set()
        real_ious = ds._calculate_mask_ious

        def ious(masks1, masks2, is_encoded=False, do_ioa=False):
            out = real_ious(masks1, masks2, is_encoded=is_encoded, do_ioa=do_ioa)
            if do_ioa:
                removed.update(id(m) for m, v in zip(masks1, np.any(out > 0.5 + eps, axis=1)) if v)
            return out
        ds._calculate_mask_ious = ious
        rng = np.random.default_rng(noise_seed)
        assigned = []   # (rows, cols) of every frame the metric assigns, in frame order

        def lsa(cost):
            if noise_seed is not None:   # every score_mat times 1 + 1e-9 * noise: a near-tied assignment would change
                cost = cost * (1 + 1e-9 * rng.standard_normal(cost.shape))
            assigned.append(real_lsa(cost))
            return assigned[-1]
        hota_module.linear_sum_assignment = lsa
        try:
            with tempfile.TemporaryDirectory() as d:
                os.makedirs(os.path.join(d, "label_02"))
                os.makedirs(os.path.join(d, "trk", "data"))
                R.write_txt(os.path.join(d, "label_02", "0000.txt"), R.id_image_rows(gt))
                R.write_txt(os.path.join(d, "trk", "data", "0000.txt"), R.id_image_rows(pr))
                ds.config = {"GT_LOC_FORMAT": "{gt_folder}/label_02/{seq}.txt"}
                ds.gt_fol, ds.tracker_fol, ds.tracker_sub_fol, ds.data_is_zipped = d, d, "data", False
                ds.seq_lengths = {"0000": num_timesteps}
                ds.class_name_to_class_id = {"car": "1", "pedestrian": "2", "ignore": "10"}
                raw = ds.get_raw_seq_data("trk", "0000")
                data = ds.get_preprocessed_seq_data(raw, "pedestrian")
            res = trackeval.metrics.HOTA().eval_sequence(data)
        finally:
            hota_module.linear_sum_assignment = real_lsa
        kept = []
        for t in range(num_timesteps):
            ped = np.flatnonzero(raw["tracker_classes"][t] == 2)
            kept.append([int(raw["tracker_ids"][t][j]) for j in ped if id(raw["tracker_dets"][t][j]) not in removed])
            assert len(kept[-1]) == len(data["tracker_ids"][t])
            # no ground-truth mask split exactly in half by two predictions: the one case the kit decides by scipy's tie order
            sim = raw["similarity_scores"][t][raw["gt_classes"][t] == 2][:, ped]
            assert ((sim >= 0.5 - eps).sum(axis=1) <= 1).all(), t
        ids = np.unique([v for k in kept for v in k])
        for t in range(num_timesteps):   # ... and they are the ones the kit renumbered
            assert np.array_equal(np.searchsorted(ids, kept[t]), data["tracker_ids"][t]), t
        counts = {k: int(data[k]) for k in ("num_gt_dets", "num_tracker_dets", "num_gt_ids", "num_tracker_ids")}
        return res, counts, kept, assigned

    g22 = np.load(os.path.join(GOLD, "g22_mots_metrics.npz"))
    scenes = [(name, g22[name + ":gt"], g22[name + ":pred"], int(g22[name + ":seq_length"]) + 1) for name in ("cases", "crowded")]
    scenes.append(("association",) + _g23_association())
    rec, all_res = {}, {}
    fields = None
    for name, gt, pr, num_timesteps in scenes:
        res, counts, kept, assigned = run(gt, pr, num_timesteps)
        fields = sorted(res)
        for seed in (1, 2, 3):
            noisy, counts_n, _, _ = run(gt, pr, num_timesteps, noise_seed=seed)
            assert counts_n == counts
            for k in fields:
                assert np.allclose(noisy[k], res[k], rtol=1e-9, atol=1e-9), (name, seed, k)
        all_res[name] = res
        rec[f"{name}:num_timesteps"] = np.int64(num_timesteps)
        for k in fields:
            rec[f"{name}:{k}"] = np.asarray(res[k], np.float64)
        for k, v in counts.items():
            rec[f"{name}:{k}"] = np.int64(v)
        rec[f"{name}:kept_ptr"] = np.concatenate(([0], np.cumsum([len(k) for k in kept]))).astype(np.int64)
        rec[f"{name}:kept_ids"] = np.asarray([v for k in kept for v in k], np.int64)
        print("g23", name, counts, "HOTA(0) %.6f" % res["HOTA(0)"], "TP", res["HOTA_TP"].astype(int).tolist())
        if name == "association":
            rec[f"{name}:gt"], rec[f"{name}:pred"] = gt, pr
            tp = res["HOTA_TP"]
            assert (tp > 0).all() and tp[0] > tp[18] and (np.diff(tp) < 0).all()   # every alpha changes the counts
            assert 2020 not in kept[1] and 2021 in kept[2] and 2030 in kept[6]
            assert counts["num_tracker_ids"] == len(np.unique(pr[pr // 1000 == 2])) - 1
            # frame 7: prediction 2010 has the higher IoU with 2005 (35 / 90 against 30 / 95) but belongs to 2006 by the global
            # alignment, and the kit assigns it to 2006 (frames 0 .. 9 are assigned, so frame 7 is the eighth)
            L = R.scene_lists(gt[7:8], pr[7:8])
            t_, tp_ = R.label_overlap(L["labels_a"], L["labels_b"], L["a_ptr"], L["b_ptr"])
            cell = lambda g, p: t_[(list(L["gt_ids"]).index(g) + 1) * (L["b_ptr"][-1] + 1) + list(L["tr_ids"]).index(p) + 1]
            assert (cell(2005, 2010), cell(2006, 2010)) == (35, 30)
            rows, cols = assigned[7]
            assert len(assigned) == 10 and list(L["tr_ids"])[cols[list(rows).index(list(L["gt_ids"]).index(2006))]] == 2010
    comb = trackeval.metrics.HOTA().combine_sequences(all_res)
    for k in sorted(comb):
        rec[f"combined:{k}"] = np.asarray(comb[k], np.float64)
    path = os.path.join(GOLD, "g23_hota.npz")
    np.savez_compressed(path, **rec)
    print("g23 bytes", os.path.getsize(path))


# ------------------------------------------------------------------ g24: TrackEval's CLEAR, Identity and Count on KITTI-MOTS
def _g24_clear():
    """12 frames of 30 x 40, both classes; the asserts of gen_g24 check that the cases are there.  Lists are in ascending id order,
    so of two entries the one with the higher id is the LATER one."""
    F, H, W = 12, 30, 40
    gt, pr = np.zeros((F, H, W), np.uint16), np.zeros((F, H, W), np.uint16)
    for f in range(5):
        _g22_rect(gt, f, 2001, 0, 8, 0, 4)                            # 2001: found by 2012 throughout (5 of 5) ...
        if f == 2:                                                    # ... and once split into two exact halves: a row star, the
            _g22_rect(pr, f, 2011, 0, 4, 0, 4)                        # later prediction continues the previous frame's match
            _g22_rect(pr, f, 2012, 4, 8, 0, 4)
        else:
            _g22_rect(pr, f, 2012, 0, 8, 0, 4)
        _g22_rect(gt, f, 2002, 10, 14, 0, 4)                          # 2002 / 2003: two equal objects; 2013 finds the later one
        _g22_rect(gt, f, 2003, 14, 18, 0, 4)                          # (5 of 5) ...
        _g22_rect(pr, f, 2013, 10 if f == 2 else 14, 18, 0, 4)        # ... and is once exactly their union: a column star
        if f == 4:
            _g22_rect(pr, f, 2014, 10, 14, 0, 4)                      # 2002 is matched in exactly 1 of 5 frames,
        _g22_rect(gt, f, 2004, 20, 26, 0, 4)                          # 2004 in exactly 4 of 5 (a fragment)
        if f != 3:
            _g22_rect(pr, f, 2015, 21, 27, 0, 4)
    for f in (5, 6, 7, 8, 9, 11):
        _g22_rect(gt, f, 2005, 0, 8, 10, 14)                          # 2005: found by 2016; frame 7 has no prediction at all, and in
    for f in (5, 6, 9):                                               # frame 8 the later half continues the match of frame 6
        _g22_rect(pr, f, 2016, 0, 8, 10, 14)
    _g22_rect(pr, 8, 2010, 0, 4, 10, 14)
    _g22_rect(pr, 8, 2016, 4, 8, 10, 14)
    _g22_rect(pr, 10, 2016, 0, 8, 10, 14)                             # frame 10 has predictions and no ground truth
    _g22_rect(pr, 10, 1002, 20, 28, 21, 29)
    _g22_rect(pr, 11, 2017, 0, 8, 10, 14)                             # an id switch against the match of frame 9
    for f in range(6):
        _g22_rect(gt, f, 10000, 0, H, 34, W)                          # the ignore region
    for f in range(10):                                               # the car: its prediction is absent in frame 4 (and 7) and
        _g22_rect(gt, f, 1001, 20, 28, 20, 28)                        # comes back under another id
        if f not in (4, 7):
            _g22_rect(pr, f, 1001 if f < 4 else 1002, 20, 28, 21, 29)
    _g22_rect(pr, 1, 1009, 2, 8, 32, 38)                              # a car, four of six columns inside the ignore region: removed
    return gt, pr, F


def gen_g24():
    """TrackEval's OWN KittiMOTS.get_raw_seq_data / get_preprocessed_seq_data, then CLEAR, Identity, Count and HOTA
    .eval_sequence and their combine_sequences / combine_classes_class_averaged / combine_classes_det_averaged, for the classes car
    and pedestrian, on g22's and g23's scenes and one new scene.  The stand-ins are gen_g23's.  Every assignment the metrics
    solve is also repeated with its cost matrix times 1 + 1e-9 * noise: no recorded field may move, so no result rests on
    scipy's tie order."""
    import tempfile
    for name, t in (("float", float), ("bool", bool), ("int", int)):
        if not hasattr(np, name):
            setattr(np, name, t)
    _install_pycocotools_standin()
    standin_iou = sys.modules["pycocotools.mask"].iou   # (a frame without ignore rows: see gen_g23)
    sys.modules["pycocotools.mask"].iou = lambda dt, gt, iscrowd: np.maximum(standin_iou(dt, gt, iscrowd), 0.0)
    sys.path.insert(0, "/root/reference/TrackEval")
    import trackeval
    from trackeval.metrics import clear as clear_module, hota as hota_module, identity as identity_module
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import mots_metrics_ref as R
    from scipy.optimize import linear_sum_assignment as real_lsa
    CLASSES, METRICS = ("car", "pedestrian"), ("HOTA", "CLEAR", "Identity", "Count")
    metric_objs = {"HOTA": trackeval.metrics.HOTA(), "CLEAR": trackeval.metrics.CLEAR({"PRINT_CONFIG": False}),
                   "Identity": trackeval.metrics.Identity({"PRINT_CONFIG": False}), "Count": trackeval.metrics.Count()}

    def run(gt, pr, num_timesteps, noise_seed=None):
        rng = np.random.default_rng(noise_seed)
        stars = []   # of CLEAR's assignments: (class, 'row' | 'column', the arm with continuity is the later one)

        def lsa(cost):
            if noise_seed is not None:
                cost = cost * (1 + 1e-9 * rng.standard_normal(cost.shape))
            return real_lsa(cost)

        def clear_lsa(cost):   # cost = -score_mat (clear.py:84): every star has exactly one arm with continuity
            for kind, m in (("row", cost), ("column", cost.T)):
                for line in m:
                    arms = np.flatnonzero(line)
                    if arms.size > 1:
                        cont = np.flatnonzero(line[arms] < -999)
                        assert arms.size == 2 and cont.size == 1, (kind, line[arms])
                        stars.append((cls_now[0], kind, bool(cont[0] == 1)))
            return lsa(cost)
        cls_now = [None]
        hota_module.linear_sum_assignment = identity_module.linear_sum_assignment = lsa
        clear_module.linear_sum_assignment = clear_lsa
        ds = trackeval.datasets.KittiMOTS.__new__(trackeval.datasets.KittiMOTS)
        res = {}
        try:
            with tempfile.TemporaryDirectory() as d:
                os.makedirs(os.path.join(d, "label_02"))
                os.makedirs(os.path.join(d, "trk", "data"))
                R.write_txt(os.path.join(d, "label_02", "0000.txt"), R.id_image_rows(gt))
                R.write_txt(os.path.join(d, "trk", "data", "0000.txt"), R.id_image_rows(pr))
                ds.config = {"GT_LOC_FORMAT": "{gt_folder}/label_02/{seq}.txt"}
                ds.gt_fol, ds.tracker_fol, ds.tracker_sub_fol, ds.data_is_zipped = d, d, "data", False
                ds.seq_lengths = {"0000": num_timesteps}
                ds.class_name_to_class_id = {"car": "1", "pedestrian": "2", "ignore": "10"}
                raw = ds.get_raw_seq_data("trk", "0000")
                for cls in CLASSES:
                    cls_now[0] = cls
                    data = ds.get_preprocessed_seq_data(raw, cls)
                    res[cls] = {m: metric_objs[m].eval_sequence(data) for m in METRICS}
        finally:
            hota_module.linear_sum_assignment = identity_module.linear_sum_assignment = clear_module.linear_sum_assignment = real_lsa
        return res, stars

    def combined(all_res):   # eval.py:93-112
        comb = {cls: {m: metric_objs[m].combine_sequences({s: r[cls][m] for s, r in all_res.items()}) for m in METRICS} for cls in CLASSES}
        per_class = dict(comb)
        comb["cls_comb_cls_av"] = {m: metric_objs[m].combine_classes_class_averaged({c: per_class[c][m] for c in CLASSES}) for m in METRICS}
        comb["cls_comb_det_av"] = {m: metric_objs[m].combine_classes_det_averaged({c: per_class[c][m] for c in CLASSES}) for m in METRICS}
        return comb

    def same(x, y, what):
        for k in x:
            if isinstance(x[k], dict):
                same(x[k], y[k], what + (k,))
            else:
                assert np.allclose(np.asarray(y[k], np.float64), np.asarray(x[k], np.float64), rtol=1e-9, atol=1e-9), (what, k, x[k], y[k])

    g22, g23 = np.load(os.path.join(GOLD, "g22_mots_metrics.npz")), np.load(os.path.join(GOLD, "g23_hota.npz"))
    scenes = [(name, g22[name + ":gt"], g22[name + ":pred"], int(g22[name + ":seq_length"]) + 1) for name in ("cases", "crowded")]
    scenes.append(("association", g23["association:gt"], g23["association:pred"], int(g23["association:num_timesteps"])))
    scenes.append(("clear",) + _g24_clear())
    rec, all_res = {}, {}
    noisy_res = {seed: {} for seed in range(1, 9)}
    for name, gt, pr, num_timesteps in scenes:
        res, stars = run(gt, pr, num_timesteps)
        for seed in noisy_res:
            noisy_res[seed][name], _ = run(gt, pr, num_timesteps, noise_seed=seed)
            same(res, noisy_res[seed][name], (name, seed))
        all_res[name] = res
        rec[f"{name}:num_timesteps"] = np.int64(num_timesteps)
        print("g24", name, "stars", stars)
        for cls in CLASSES:
            c, i = res[cls]["CLEAR"], res[cls]["Identity"]
            print("   ", cls, {k: int(c[k]) for k in ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag")}, "MOTP_sum %.6f" % c["MOTP_sum"],
                  {k: int(i[k]) for k in ("IDTP", "IDFN", "IDFP")}, res[cls]["Count"])
        if name == "clear":
            rec[f"{name}:gt"], rec[f"{name}:pred"] = gt, pr
            assert gt.shape == (12, 30, 40)
            ped = [s[1:] for s in stars if s[0] == "pedestrian"]
            assert ped.count(("row", True)) == 2 and ped.count(("column", True)) == 1 and len(ped) == 3   # continuity on the later arm
            c = res["pedestrian"]["CLEAR"]
            # continuity survives the empty tracker frame 7 (else 2010, the earlier half, would win frame 8: two more IDSW); the one
            # IDSW is frame 11's, the one Frag 2004's missing frame 3
            assert (c["CLR_TP"], c["CLR_FN"], c["CLR_FP"], c["IDSW"], c["Frag"]) == (20, 6, 3, 1, 1)
            assert not pr[7].any() and gt[7].any() and not gt[10].any() and pr[10].any()
            # 2001, 2003 (5 of 5) and 2005 (5 of 6) are mostly tracked; 2004 (exactly 4 of 5) and 2002 (exactly 1 of 5) partly
            assert (c["MT"], c["PT"], c["ML"]) == (3, 2, 0)
            c, n = res["car"]["CLEAR"], res["car"]["Count"]
            # the car: frames 4 and 7 have no car prediction, so they keep the continuity state (no Frag); 1009 is removed
            assert (c["CLR_TP"], c["IDSW"], c["Frag"], c["CLR_FP"], c["CLR_FN"]) == (8, 1, 0, 1, 2) and n["Dets"] == 9 and n["IDs"] == 2
    comb = combined(all_res)
    for seed, noisy in noisy_res.items():
        same(comb, combined(noisy), ("combined", seed))
    for prefix, per_cls in list(all_res.items()) + [("COMBINED_SEQ", comb)]:
        for cls, per_metric in per_cls.items():
            for m, fields in per_metric.items():
                for k, v in fields.items():
                    rec[f"{prefix}:{cls}:{m}:{k}"] = np.asarray(v, np.float64)
    path = os.path.join(GOLD, "g24_clear_identity.npz")
    np.savez_compressed(path, **rec)
    print("g24 bytes", os.path.getsize(path), "keys", len(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="g0,g1,g4,g5,g6,g7,g8,g2,g3,g11,g12,g10,g9")
    args = ap.parse_args()
    torch.set_num_threads(os.cpu_count())
    os.makedirs(GOLD, exist_ok=True)
    mpn = import_reference()
    only = set(args.only.split(","))
    if "g0" in only: gen_g0(mpn)
    if "g1" in only: gen_g1(mpn)
    if "g4" in only: gen_g4(mpn)
    if "g5" in only: gen_g5(mpn)
    if "g6" in only: gen_g6(mpn)
    if "g7" in only: gen_g7()
    if "g8" in only: gen_g8()
    if "g2" in only: gen_cfg(mpn, "A", "g2_cfgA")
    if "g3" in only: gen_cfg(mpn, "B", "g3_cfgB", sample=4096)
    if "g10" in only: gen_g10()
    if "g9" in only: gen_g9()
    if "g11" in only: gen_g11(mpn)
    if "g12" in only: gen_g12(mpn)
    if "g13" in only: gen_g13(mpn)
    if "g14" in only: gen_g14()
    if "g15" in only: gen_g15(mpn)
    if "g16" in only: gen_g16()
    if "g17" in only: gen_g17()
    if "g18" in only: gen_g18(mpn)
    if "g19" in only: gen_g19()
    if "g20" in only: gen_g20()
    if "g21" in only: gen_g21()
    if "g22" in only: gen_g22()
    if "g23" in only: gen_g23()
    if "g24" in only: gen_g24()


if __name__ == "__main__":
    main()
