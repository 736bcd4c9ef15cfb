#!/usr/bin/env python3
"""Time of the Mask R-CNN FPN backbone (fpn_net.resnet50_fpn_backbone, seeded weights) on 1 and 8 frames of 375 x 1242 (KITTI)
and 1080 x 1920 (MOT17): ``forward`` -- the stock PyTorch-ROCm modules under no_grad -- against ``forward_native``
(csrc/conv_strided.hip), both behind ``embed_inputs.rcnn_transform`` (timed on its own, once per size).

Per size, both paths are timed in one process with device events, alternating, after warm-up calls of each (long enough for the
stock library's algorithm choice to settle); reported are the median and the min .. max of the calls.  Every size runs in a
child process of its own under its own time limit; after a child that fails or runs out of time nothing more is started.  The
multiply-adds are computed from the layer shapes (the 53 convolutions of the body and the 8 of the pyramid at the padded size;
frozen BatchNorm, pooling and element-wise work are not counted), so the rate against the 157.3 TFLOP/s fp32-MFMA peak is the
network's arithmetic over the WHOLE forward's time: a whole-forward rate, not a kernel's share of peak.  ``native_groups`` says
where the native forward's time goes: every convolution of the launch list timed alone, summed by group (``group_times``).

Writes profiles/fpn_backbone/timing.json (or --out).  Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FP32_MATRIX_PEAK = 157.3e12     # MI355X, fp32-input MFMA
SEED = 37
SIZES = ["375x1242x1", "375x1242x8", "1080x1920x1", "1080x1920x8"]


def network_macs(net, H, W):
    """multiply-adds of one frame whose padded batch image is ``H x W``: the body's convolutions and the pyramid's eight"""
    macs = sum(c["cout"] * c["Hout"] * c["Wout"] * c["cin"] * c["k"] * c["k"] for c in net.conv_layers(H, W))
    for i, (h, w) in enumerate(net.level_shapes(H, W)[:4]):
        macs += 256 * h * w * (net.fpn.inner_blocks[i].in_channels + 256 * 9)
    return macs


def timed(fn):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def one(size, runs, warmup):
    import numpy as np
    import torch
    from mpntrackseg_amd import embed_inputs as E, fpn_net, synth
    H, W, n = (int(v) for v in size.split("x"))
    dev = torch.device("cuda:0")
    net = fpn_net.resnet50_fpn_backbone()
    synth.make_fpn_weights(net, SEED)
    net = net.to(dev).eval()
    base = torch.from_numpy((synth.uniform01(SEED, H * W * 3, stream=1) * 256).astype(np.uint8).reshape(1, H, W, 3)).to(dev)
    frames = torch.cat([base.roll(17 * i, dims=2) for i in range(n)], dim=0).contiguous()
    t_transform = [timed(lambda: E.rcnn_transform(frames))[0] for _ in range(warmup + 5)][warmup:]
    x, image_size = E.rcnn_transform(frames)
    paths = {"stock": lambda: net(x), "native": lambda: net.forward_native(x)}
    out, times = {}, {"stock": [], "native": []}
    with torch.no_grad():
        for path, fn in paths.items():
            for _ in range(warmup):
                out[path] = fn()
        torch.cuda.synchronize()
        for _ in range(runs):
            for path, fn in paths.items():     # alternating: both paths see the same neighbours on the machine
                times[path].append(timed(fn)[0])
    macs = network_macs(net, int(x.shape[2]), int(x.shape[3])) * n
    res = {"frames": [n, H, W], "batch": list(x.shape), "image_size": list(image_size), "runs": runs, "warmup": warmup, "gmac": macs / 1e9,
           "rcnn_transform_median_ms": statistics.median(t_transform),
           "native_vs_stock_max_rel_diff": {k: float((out["native"][k] - out["stock"][k]).abs().max() / out["stock"][k].abs().max())
                                            for k in out["native"]}}
    for path, ts in times.items():
        med = statistics.median(ts)
        res[path] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "frames_per_s": n / (med * 1e-3),
                     "whole_forward_tflops": 2 * macs / (med * 1e-3) / 1e12,
                     "whole_forward_fraction_of_fp32_matrix_peak": 2 * macs / (med * 1e-3) / FP32_MATRIX_PEAK}
    res["native_over_stock_median"] = res["native"]["median_ms"] / res["stock"]["median_ms"]
    res["native_groups"] = group_times(net, x)
    print(json.dumps(res))


def group_times(net, x):
    """Where the native forward's time goes: every convolution of the forward's own launch plan (its ``Launch`` records: layer,
    residual or not, ReLU, the ``up`` size) alone, on an input of its shape and through the entry point and epilogue the record
    names, as the median of five device-event-timed calls after one warm-up; summed by group (the stem's convolution, layer1 ..
    layer4, the pyramid's laterals and its output convolutions) with the group's multiply-adds.  The max-pool and the host's work
    between launches are not in it."""
    import torch
    from mpntrackseg_amd.conv_affine import Launch, conv2d_affine_native, conv2d_affine_up_native
    n, _, H, W = (int(s) for s in x.shape)
    steps = net._plan(net._native if net._native is not None else net.prepare_native(), H, W)["steps"]
    groups = {}
    for st in steps:
        if not isinstance(st, Launch) or st.kind != "conv":
            continue
        c, name = st.layer, st.layer["name"]
        group = ("stem" if name == "body.conv1" else "fpn_lateral" if name.startswith("fpn.inner_blocks.") else
                 "fpn_output" if name.startswith("fpn.layer_blocks.") else name.split(".")[1])
        xin = torch.randn((n, c["cin"], c["H"], c["W"]), device=x.device)
        wt = torch.randn((c["cout"], c["cin"], c["k"], c["k"]), device=x.device)
        sh = torch.ones(c["cout"], device=x.device)
        sc = sh if c["scale"] is not None else None
        out = torch.empty((n,) + c["out_shape"], device=x.device)
        if st.up is not None:
            coarse = torch.randn((n, c["cout"]) + tuple(st.up), device=x.device)
            call = lambda: conv2d_affine_up_native(xin, wt, sc, sh, coarse, out=out)
        else:
            res = torch.randn_like(out) if st.residual is not None else None
            call = lambda: conv2d_affine_native(xin, wt, sc, sh, stride=c["stride"], residual=res, relu=st.relu, out=out)
        call()
        ms = statistics.median(timed(call)[0] for _ in range(5))
        g = groups.setdefault(group, {"launches": 0, "ms": 0.0, "gmac": 0.0})
        g["launches"] += 1
        g["ms"] += ms
        g["gmac"] += n * c["cout"] * c["Hout"] * c["Wout"] * c["cin"] * c["k"] * c["k"] / 1e9
    for g in groups.values():
        g["tflops"] = 2 * g["gmac"] / g["ms"]
    return groups


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", nargs="+", default=SIZES, help="HxWxN: N frames of H x W")
    ap.add_argument("--limit", type=int, default=240, help="seconds one size may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fpn_backbone", "timing.json"))
    ap.add_argument("--one", help="time one size in this process")
    a = ap.parse_args()
    runs = max(a.runs, 5)
    if a.one is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("time_fpn_backbone.py needs a GPU")
        return one(a.one, runs, a.warmup)
    res = {"sizes": []}
    for size in a.sizes:                       # a child per size, each under its own time limit; this process never opens the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--one", size, "--runs", str(runs), "--warmup", str(a.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            res["sizes"].append({"size": size, "error": "ran longer than %d s" % a.limit})
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            res["sizes"].append({"size": size, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]})
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
