#!/usr/bin/env python3
"""Time of the ReID ResNet50 (reid_net.resnet50_fc256, seeded weights) on n = 64 and n = 1000 crops of 128 x 64 (1000 is the
reference's img_batch_size): ``forward`` -- the stock PyTorch-ROCm modules under no_grad -- against ``forward_native``
(csrc/conv_strided.hip).

Per n, both paths are timed in one process with device events, alternating, after warm-up calls of each (long enough for the
stock library's algorithm choice to settle); reported are the median and the min .. max of at least 20 calls.  Every n runs in
a child process of its own under its own time limit; after a child that fails or runs out of time nothing more is started.  The
multiply-adds are computed from the layer shapes (every convolution and the two fc layers; BatchNorm, pooling and element-wise
work are not counted), so the native rate against the 157.3 TFLOP/s fp32-MFMA peak is the network's arithmetic over the WHOLE
forward's time: a whole-forward rate, not a kernel's share of peak.

Writes profiles/reid_net/timing.json (or --out).  Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FP32_MATRIX_PEAK = 157.3e12     # MI355X, fp32-input MFMA (MI355X_MICROARCH.md)
SEED = 31


def network_macs(net, H=128, W=64):
    """multiply-adds of one crop: every convolution of featuremaps and the Linear layers of fc"""
    from torch import nn
    macs = sum(c["cout"] * c["Hout"] * c["Wout"] * c["cin"] * c["k"] * c["k"] for c in net.conv_layers(H, W))
    if net.fc is not None:
        macs += sum(m.in_features * m.out_features for m in net.fc if isinstance(m, nn.Linear))
    return macs


def one(n, runs, warmup):
    import torch
    from mpntrackseg_amd import reid_net, synth
    dev = torch.device("cuda:0")
    net = reid_net.resnet50_fc256(10)
    synth.make_reid_weights(net, SEED)
    net = net.to(dev).eval()
    base = torch.from_numpy(synth.normal(SEED, (8, 3, 128, 64), stream=synth.REID_INPUT_STREAM)).to(dev)
    x = base.repeat((n + 7) // 8, 1, 1, 1)[:n].contiguous()
    paths = {"stock": lambda: net(x), "native": lambda: net.forward_native(x)}
    out, times = {}, {"stock": [], "native": []}
    with torch.no_grad():
        for path, fn in paths.items():
            for _ in range(warmup):
                out[path] = fn()
        torch.cuda.synchronize()
        for _ in range(runs):
            for path, fn in paths.items():     # alternating: both paths see the same neighbours on the machine
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                times[path].append(t0.elapsed_time(t1))
    macs = network_macs(net) * n
    res = {"n": n, "runs": runs, "warmup": warmup, "gmac": macs / 1e9,
           "native_vs_stock_max_rel_diff": {"f": float((out["native"][0] - out["stock"][0]).abs().max() / out["stock"][0].abs().max()),
                                            "v": float((out["native"][1] - out["stock"][1]).abs().max() / out["stock"][1].abs().max())}}
    for path, ts in times.items():
        med = statistics.median(ts)
        res[path] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "images_per_s": n / (med * 1e-3),
                     "whole_forward_tflops": 2 * macs / (med * 1e-3) / 1e12,
                     "whole_forward_fraction_of_fp32_matrix_peak": 2 * macs / (med * 1e-3) / FP32_MATRIX_PEAK}
    res["native_over_stock_median"] = res["native"]["median_ms"] / res["stock"]["median_ms"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1000])
    ap.add_argument("--limit", type=int, default=240, help="seconds one size may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reid_net", "timing.json"))
    ap.add_argument("--one", type=int, help="time one size in this process")
    a = ap.parse_args()
    runs = max(a.runs, 20)
    if a.one is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("time_reid_net.py needs a GPU")
        return one(a.one, runs, a.warmup)
    res = {"sizes": []}
    for n in a.sizes:                          # a child per size, each under its own time limit; this process never opens the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(n), "--runs", str(runs), "--warmup", str(a.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            res["sizes"].append({"n": n, "error": "ran longer than %d s" % a.limit})
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            res["sizes"].append({"n": n, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]})
            break
        res["sizes"].append(json.loads(line[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if any("error" in s for s in res["sizes"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
