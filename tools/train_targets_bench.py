#!/usr/bin/env python3
"""Time the training targets on one MI355X at a user-scale graph (N = 500 detections, k = 3 classified steps, E = 75,000 edges,
56 x 56 masks, every row with a ground-truth mask): the native edge labels, the native loss with both gradients
(``tracking_loss_and_grad`` + ``mask_loss_and_grad``), the same through ``loss.compute_loss`` and autograd, and the reference's
``_compute_loss`` (pl_module.py:88-120) written in stock torch with ``torch.autograd.grad`` on the same device.

    python tools/train_targets_bench.py [--nodes 500] [--steps 3] [--edges 75000] [--repeats 9]

Device events around a synchronised window after two warm-up calls, the median of the repeats (tools/full_masks_bench.py).  The
two losses and their gradients are compared before anything is printed.  Prints one JSON line.  ``--repeats 1`` under a kernel
trace shows the launches of one call each after the warm-up.

``--e2e`` instead runs g6's model end to end (tests/test_gpu_training_targets.py ``e2e_errors``) once under the native loss and
once under the stock-torch one and prints, per parameter, both errors against tests/golden/g21_training_targets.npz."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch
import torch.nn.functional as F
from mpntrackseg_amd import synth
from mpntrackseg_amd.graph import assign_edge_labels
from mpntrackseg_amd.loss import compute_loss, mask_loss_and_grad, tracking_loss_and_grad
import training_targets_ref as R


def device_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}


def stock_compute_loss(outputs, batch, w):
    """the reference's _compute_loss (pl_module.py:88-120) in stock torch on the device"""
    labels = batch.edge_labels
    positive_vals = labels.sum()
    if positive_vals:
        pos_weight = (labels.shape[0] - positive_vals) / positive_vals
    else:
        pos_weight = torch.zeros(1, device=labels.device)
    loss = 0
    for s in range(len(outputs["classified_edges"])):
        loss = loss + w["tracking"] * F.binary_cross_entropy_with_logits(outputs["classified_edges"][s].view(-1), labels.view(-1),
                                                                         pos_weight=pos_weight)
        gt, pm = batch.mask_labels[batch.mask_gt_ixs], outputs["mask_predictions"][s][batch.mask_gt_ixs]
        if gt.numel():
            loss = loss + w["segmentation"] * F.binary_cross_entropy_with_logits(pm, gt)
    return loss


def e2e():
    import test_gpu_training_targets as T
    z = np.load(os.path.join(REPO, "tests", "golden", "g21_training_targets.npz"))
    w = R.LOSS_WEIGHTS
    loss, errs = T.e2e_errors(z, lambda out, d: compute_loss(out, d, w))
    stock, stock_errs = T.e2e_errors(z, lambda out, d: stock_compute_loss(out, d, w))
    hot = ("encoder.", "MPNet.", "classifier.")
    print(json.dumps({
        "loss": {"native": loss, "stock": stock, "reference": float(z["e2e:loss"])},
        "max_err_hot_path": {"native": max(max(v) for k, v in errs.items() if k.startswith(hot)),
                             "stock": max(max(v) for k, v in stock_errs.items() if k.startswith(hot))},
        "max_err_mask_branch": {"native": max(max(v) for k, v in errs.items() if not k.startswith(hot)),
                                "stock": max(max(v) for k, v in stock_errs.items() if not k.startswith(hot))},
        "per_tensor_native_stock": {k: [errs[k][0], errs[k][1], stock_errs[k][0], stock_errs[k][1]] for k in errs}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=500)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--edges", type=int, default=75000)
    ap.add_argument("--valid", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_targets_bench.py measures on a HIP device; none is visible")
    if a.e2e:
        return e2e()
    dev = torch.device("cuda:0")
    N, k, E = a.nodes, a.steps, a.edges
    w = R.LOSS_WEIGHTS
    g = synth.make_graph(N, E, T=20, seed=5, node_in_dim=4)
    ei = torch.from_numpy(g["edge_index"]).to(dev)
    ids = torch.from_numpy(R.track_ids(g["frame"], 5)).to(dev)
    labels = assign_edge_labels(ei, ids, mode="closest")
    assert np.array_equal(labels.cpu().numpy(), R.edge_labels(g["edge_index"], ids.cpu().numpy(), "closest"))
    logits = torch.from_numpy(synth.normal(7, (k, E), std=2.0)).to(dev)
    preds = [torch.from_numpy(synth.normal(8, (N, 1, 56, 56), stream=s, std=1.5)).to(dev) for s in range(k)]
    mlab = torch.from_numpy((synth.uniform01(9, N * 3136).reshape(N, 1, 56, 56) < 0.4).astype(np.float32)).to(dev)
    valid = torch.from_numpy(R.first_valid(a.valid, N)).to(dev)
    batch = argparse.Namespace(edge_labels=labels, mask_labels=mlab, mask_gt_ixs=valid)
    res = {}

    def native_ops():
        res["tl"], res["gl"] = tracking_loss_and_grad(logits, labels, 0, w["tracking"])
        res["ml"], res["gm"] = mask_loss_and_grad(preds, mlab, valid, w["segmentation"])

    def native_autograd():
        lg = logits.detach().requires_grad_(True)
        pr = [p.detach().requires_grad_(True) for p in preds]
        loss = compute_loss({"classified_edges": [lg[s].view(-1, 1) for s in range(k)], "mask_predictions": pr}, batch, w)
        loss.backward()

    def stock():
        lg = logits.detach().requires_grad_(True)
        pr = [p.detach().requires_grad_(True) for p in preds]
        loss = stock_compute_loss({"classified_edges": [lg[s].view(-1, 1) for s in range(k)], "mask_predictions": pr}, batch, w)
        grads = torch.autograd.grad(loss, [lg] + pr)
        res["stock"], res["stock_gl"], res["stock_gm"] = loss.detach(), grads[0], grads[1:]

    out = {"shape": {"nodes": N, "steps": k, "edges": E, "valid_rows": a.valid, "mask": 56},
           "edge_labels_closest_ms": device_ms(lambda: assign_edge_labels(ei, ids, mode="closest", validate=False), a.repeats),
           "edge_labels_all_ms": device_ms(lambda: assign_edge_labels(ei, ids, mode="all", validate=False), a.repeats),
           "native_loss_and_grads_ms": device_ms(native_ops, a.repeats),
           "native_compute_loss_autograd_ms": device_ms(native_autograd, a.repeats),
           "stock_torch_loss_and_grads_ms": device_ms(stock, a.repeats)}
    native = float(res["tl"][0]) + float(res["ml"][0])
    ref = float(res["stock"])
    d_gl = float((res["gl"] - res["stock_gl"]).abs().max() / res["stock_gl"].abs().max())
    d_gm = max(float((a_ - b_).abs().max() / b_.abs().max()) for a_, b_ in zip(res["gm"], res["stock_gm"]))
    out.update({"positive_labels": int(labels.sum()), "loss_native": native, "loss_stock": ref, "grad_logits_max_rel_diff": d_gl,
                "grad_masks_max_rel_diff": d_gm,
                "mask_pass_mb": round((a.valid * (1 + k) + N * k) * 3136 * 4 / 1e6, 1), "repeats": a.repeats})
    print(json.dumps(out))
    if abs(native - ref) > 1e-5 * max(1.0, abs(ref)) or d_gl > 1e-5 or d_gm > 1e-5:
        raise SystemExit("the native loss differs from the stock-torch one")


if __name__ == "__main__":
    main()
