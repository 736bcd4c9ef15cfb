#!/usr/bin/env python3
"""Time of the mask branch in TRAINING: MOTMPNet.mask_predictions forward + backward with the stock convolution backward (MIOpen
under autograd), with the native Conv2d one (mask_conv_grads = 'native': mpnhip_conv2d_forward under autograd,
mpnhip_conv2d_backward) and with every layer native ('native_all': mpnhip_conv_transpose2d_backward and
mpnhip_layer_norm_backward as well), on the batch of tools/time_joint_step.py: 2 graphs of synth.make_knn_graph(frames=20, dets=7, top_k=100)
(280 nodes, 28,748 edges), synth.MASK_PARAMS, L = 4 with 2 classified steps, x_ext [280, 256, 14, 14].  The loss is sum(pred * r)
with fixed r; the logits are a leaf that takes a gradient, x_ext takes none -- what the joint training step asks of the branch.

The selectors are timed in the same process with device events, alternating, after 5 warm-up calls each; reported are the median
and the min .. max of at least 20 calls, and the largest difference between each native route's parameter gradients and the stock route's.  The first call of
each selector (code-object load, the library's algorithm search) is timed in a fresh child process of its own.

Writes profiles/mask_convs/train_timing.json (or --out).  Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mpntrackseg_amd import synth
from mpntrackseg_amd.mpn import MOTMPNet

L = 4
SELECTORS = ("stock", "native", "native_all")


def problem(dev):
    params = synth.model_params(32, L, "sum", num_class_steps=2, node_in_dim=64)
    params.update(synth.MASK_PARAMS)
    model = MOTMPNet(params)
    W = synth.make_weights(params, seed=7, gain=0.6)
    W.update(synth.make_mask_weights(seed=17))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    model = model.to(dev).train()
    b = synth.batch_graphs([synth.make_knn_graph(frames=20, dets=7, top_k=100, seed=1 + i, node_in_dim=64) for i in range(2)])
    n = b["x"].shape[0]
    t = lambda a: torch.from_numpy(a).to(dev)
    x, ei, ea = t(b["x"]), t(b["edge_index"]), t(b["edge_attr"])
    x_ext = t(synth.normal(9, (n, 256, 14, 14), stream=1, std=0.5))
    with torch.no_grad():
        logits = model.hot_path(x, ei, ea)
    r = [t(synth.normal(10, (n, 1, 56, 56), stream=i)) for i in range(2)]
    return model, x_ext, ei, logits.detach().clone().requires_grad_(True), r


class Holder:
    pass


def run(model, x_ext, ei, logits, r, holder, selector):
    model.mask_conv_grads = selector
    model.zero_grad(set_to_none=True)
    logits.grad = None
    preds = model.mask_predictions(x_ext, ei, logits, holder=holder)
    torch.autograd.backward(preds, grad_tensors=r)


def mask_grads(model):
    return [p.grad.detach().clone() for m in model._mask_modules() for p in m.parameters()]


def first_call(selector):
    model, x_ext, ei, logits, r = problem(torch.device("cuda:0"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(model, x_ext, ei, logits, r, Holder(), selector)
    torch.cuda.synchronize()
    print(json.dumps({"selector": selector, "first_call_ms": (time.perf_counter() - t0) * 1e3}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mask_convs",
                                                  "train_timing.json"))
    ap.add_argument("--first-call", choices=SELECTORS, help="time the first call of one selector in this (fresh) process")
    ap.add_argument("--only", choices=SELECTORS, help="run one selector alone, a few calls, no file: the run to put under a profiler")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mask_branch_train.py needs a GPU")
    if a.first_call:
        return first_call(a.first_call)
    runs = max(a.runs, 20)
    model, x_ext, ei, logits, r = problem(torch.device("cuda:0"))
    holder = Holder()
    if a.only:
        for _ in range(a.warmup):
            run(model, x_ext, ei, logits, r, holder, a.only)
        torch.cuda.synchronize()
        return
    grads = {}
    for sel in SELECTORS:
        for _ in range(a.warmup):
            run(model, x_ext, ei, logits, r, holder, sel)
        grads[sel] = mask_grads(model)
    torch.cuda.synchronize()
    times = {sel: [] for sel in SELECTORS}
    for _ in range(runs):
        for sel in SELECTORS:              # alternating: the routes see the same neighbours on the machine
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run(model, x_ext, ei, logits, r, holder, sel)
            t1.record()
            t1.synchronize()
            times[sel].append(t0.elapsed_time(t1))
    rel = lambda sel: max(float((n_ - s_).abs().max() / s_.abs().max().clamp_min(1e-30)) for n_, s_ in zip(grads[sel], grads["stock"]))
    res = {"problem": {"graphs": 2, "nodes": int(x_ext.shape[0]), "edges": int(ei.shape[1]), "L": L, "x_ext": list(x_ext.shape)},
           "what": "mask_predictions forward + backward, device events, ms", "runs": runs, "warmup": a.warmup,
           "native_vs_stock_max_rel_grad_diff": rel("native"), "native_all_vs_stock_max_rel_grad_diff": rel("native_all")}
    for sel, ts in times.items():
        res[sel] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    res["native_over_stock_median"] = res["native"]["median_ms"] / res["stock"]["median_ms"]
    res["native_all_over_stock_median"] = res["native_all"]["median_ms"] / res["stock"]["median_ms"]
    for sel in SELECTORS:                  # a fresh process per selector: nothing loaded, nothing tuned
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--first-call", sel], capture_output=True, text=True, timeout=600)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        res[sel]["first_call_ms"] = json.loads(line[-1])["first_call_ms"] if p.returncode == 0 and line else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
