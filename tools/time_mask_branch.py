#!/usr/bin/env python3
"""Time of the mask branch (MOTMPNet.mask_predictions) with the stock PyTorch-ROCm modules and with the native convolutions
(mask_convs = 'stock' | 'native'), on ONE window-sized problem: synth.make_knn_graph(frames=20, dets=25, top_k=60) (500 nodes),
synth.MASK_PARAMS, L = 4, last_only=True, under no-grad -- what one window of sliding-window inference runs.

Both paths are timed in the same process with device events, alternating, after 5 warm-up calls each; reported are the median
and the min .. max of at least 20 calls.  The first call of each path (code-object load, the library's algorithm search) is
timed in a fresh child process of its own.  The FLOP count is computed from the modules' shapes (2 per multiply-add of every
convolution; the attention aggregation, LayerNorm and element-wise work are not counted), so "fraction of peak" is the branch's
convolution arithmetic over the WHOLE branch's time: an end-to-end figure, not a kernel's share of peak.

Writes profiles/mask_convs/timing.json (or --out).  Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch import nn

from mpntrackseg_amd import synth
from mpntrackseg_amd.mpn import MOTMPNet

FP32_MATRIX_PEAK = 157e12     # MI355X, fp32-input MFMA (MI355X_MICROARCH.md)
L = 4


def problem(dev):
    params = synth.model_params(32, L, "sum", num_class_steps=2, node_in_dim=64)
    params.update(synth.MASK_PARAMS)
    model = MOTMPNet(params)
    W = synth.make_weights(params, seed=7, gain=0.6)
    W.update(synth.make_mask_weights(seed=17))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    model = model.to(dev).eval()
    g = synth.make_knn_graph(frames=20, dets=25, top_k=60, seed=3, node_in_dim=64)
    n = g["x"].shape[0]
    x = torch.from_numpy(g["x"]).to(dev)
    ei = torch.from_numpy(g["edge_index"]).to(dev)
    ea = torch.from_numpy(g["edge_attr"]).to(dev)
    x_ext = torch.from_numpy(synth.normal(9, (n, 256, 14, 14), stream=1, std=0.5)).to(dev)
    with torch.no_grad():
        logits = model.hot_path(x, ei, ea)
    return model, x_ext, ei, logits


def conv_flop_per_node(model, hw=(14, 14)):
    """2 x multiply-adds of every convolution one call with last_only=True runs, per node."""
    def stack(layers, h, w):
        total = 0
        for m in layers:
            if isinstance(m, nn.ConvTranspose2d):
                total += 2 * h * w * m.in_channels * m.out_channels * m.kernel_size[0] * m.kernel_size[1]
                h, w = h * m.stride[0], w * m.stride[1]
            elif isinstance(m, nn.Conv2d):
                total += 2 * h * w * m.in_channels * m.out_channels * m.kernel_size[0] * m.kernel_size[1]
        return total, h, w
    h, w = hw
    enc, _, _ = stack(model.node_ext_encoder.layers, h, w)
    step, _, _ = stack(model.MPAttentionNet.node_model.layers, h, w)
    mm = model.mask_predictor
    head = stack(mm.feature_encoder.layers, h, w)[0] + stack(mm.mask_head.layers, h, w)[0] + stack(mm.mask_predictor.layers, h, w)[0]
    return enc + L * step + head


def run(model, x_ext, ei, logits, holder):
    return model.mask_predictions(x_ext, ei, logits, holder=holder, last_only=True)[-1]


def first_call(path):
    dev = torch.device("cuda:0")
    model, x_ext, ei, logits = problem(dev)
    model.mask_convs = path

    class Holder:
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        run(model, x_ext, ei, logits, Holder())
    torch.cuda.synchronize()
    print(json.dumps({"path": path, "first_call_ms": (time.perf_counter() - t0) * 1e3}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mask_convs",
                                                  "timing.json"))
    ap.add_argument("--first-call", choices=("stock", "native"), help="time the first call of one path in this (fresh) process")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mask_branch.py needs a GPU")
    if a.first_call:
        return first_call(a.first_call)
    runs = max(a.runs, 20)
    dev = torch.device("cuda:0")
    model, x_ext, ei, logits = problem(dev)

    class Holder:
        pass
    holder = Holder()
    out = {}
    times = {"stock": [], "native": []}
    with torch.no_grad():
        for path in times:
            model.mask_convs = path
            for _ in range(a.warmup):
                out[path] = run(model, x_ext, ei, logits, holder)
        torch.cuda.synchronize()
        for _ in range(runs):
            for path in times:             # alternating: both paths see the same neighbours on the machine
                model.mask_convs = path
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run(model, x_ext, ei, logits, holder)
                t1.record()
                t1.synchronize()
                times[path].append(t0.elapsed_time(t1))
    n = int(x_ext.shape[0])
    flop = conv_flop_per_node(model) * n
    diff = float((out["native"] - out["stock"]).abs().max() / out["stock"].abs().max())
    res = {"problem": {"nodes": n, "edges": int(ei.shape[1]), "L": L, "last_only": True, "x_ext": list(x_ext.shape)},
           "runs": runs, "warmup": a.warmup, "conv_gflop": flop / 1e9, "native_vs_stock_max_rel_diff": diff}
    for path, ts in times.items():
        med = statistics.median(ts)
        res[path] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "conv_tflops_end_to_end": flop / med / 1e9,
                     "fraction_of_fp32_matrix_peak": flop / (med * 1e-3) / FP32_MATRIX_PEAK}
    res["native_over_stock_median"] = res["native"]["median_ms"] / res["stock"]["median_ms"]
    for path in times:                     # a fresh process per path: nothing loaded, nothing tuned
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--first-call", path], capture_output=True, text=True, timeout=600)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        res[path]["first_call_ms"] = json.loads(line[-1])["first_call_ms"] if p.returncode == 0 and line else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
