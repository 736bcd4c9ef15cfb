#!/usr/bin/env python3
"""Time of the Mask R-CNN RoI heads (rcnn_heads.RoIHeads at the true sizes, seeded weights) on one MOT17-sized frame batch: FRAMES
frames of 1080 x 1920 (a 768 x 1344 network image, a seeded N(0, 1) pyramid in place of the backbone's), 30 boxes per frame.

``predict_boxes`` and ``predict_masks``: ``convs='stock'`` -- the torch modules under no_grad behind mpnhip_fpn_roi_align --
against ``convs='native'`` (csrc/rcnn_heads.hip and the kernels its route names).  ``nms_batched`` for one frame and for the
batch: mpnhip_nms_batched against a torch restatement -- the IoU matrix on the device, the greedy loop on the host.  Both
paths are timed in one process with device events (the NMS restatement, which ends on the host, with a host clock around a
synchronised call), alternating, after warm-up calls of each; reported are the median and the min .. max of the calls.
``native_steps`` says where the native time goes: the pooler, fc6, fc7, mpnhip_box_predict and the mask layers each timed alone,
with fc6's weight traffic (its 51 MB of weights once) over its time.

The measurement runs in a child process under a time limit.  Writes profiles/rcnn_heads/timing.json (or --out).  Needs a GPU:
there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SEED = 53
FRAMES, BOXES_PER_FRAME = 4, 30
ORIGINAL, IMAGE, LEVELS = (1080, 1920), (749, 1333), ((192, 336), (96, 168), (48, 84), (24, 42))


def timed(fn):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def host_timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def compare(paths, runs, warmup, clock=timed):
    times = {k: [] for k in paths}
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    for _ in range(runs):
        for k, fn in paths.items():            # alternating: both paths see the same neighbours on the machine
            times[k].append(clock(fn)[0])
    res = {k: summary(v) for k, v in times.items()}
    res["native_over_stock_median"] = res["native"]["median_ms"] / res["stock"]["median_ms"]
    return res


def nms_torch(boxes, scores, frame, iou_threshold):
    """the restatement: per frame the IoU matrix on the device, the greedy loop on the host"""
    import torch
    kept = []
    for f in torch.unique(frame).tolist():
        rows = torch.nonzero(frame == f)[:, 0]
        b = boxes[rows]
        order = torch.argsort(scores[rows], descending=True, stable=True)
        b = b[order]
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        wh = (torch.min(b[:, None, 2:], b[None, :, 2:]) - torch.max(b[:, None, :2], b[None, :, :2])).clamp(min=0)
        inter = wh[..., 0] * wh[..., 1]
        over = (inter / (area[:, None] + area[None, :] - inter) > iou_threshold).cpu().numpy()
        alive, mine = [True] * len(rows), []
        for i in range(len(rows)):
            if alive[i]:
                mine.append(i)
                for j in range(i + 1, len(rows)):
                    if over[i, j]:
                        alive[j] = False
        kept.append(rows[order[torch.tensor(mine, dtype=torch.int64)]])
    return torch.cat(kept)


def one(runs, warmup):
    import numpy as np
    import torch
    from mpntrackseg_amd import rcnn_heads as RH, synth
    from mpntrackseg_amd.conv_affine import conv2d_affine_native
    dev = torch.device("cuda:0")
    heads = RH.RoIHeads().eval()
    synth.make_roi_head_weights(heads, SEED)
    heads = heads.to(dev)
    feats = [torch.from_numpy(synth.normal(SEED, (FRAMES, 256) + s, stream=10 + l)).to(dev) for l, s in enumerate(LEVELS)]
    n = FRAMES * BOXES_PER_FRAME
    u = synth.uniform01(SEED, 4 * n, stream=20).reshape(n, 4).astype(np.float64)
    w, h = 40 + 160 * u[:, 2], 100 + 400 * u[:, 3]
    x1, y1 = u[:, 0] * (ORIGINAL[1] - w), u[:, 1] * (ORIGINAL[0] - h)
    boxes = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)
    frame = np.repeat(np.arange(FRAMES), BOXES_PER_FRAME)
    args = (heads, feats, torch.from_numpy(boxes).to(dev), frame, IMAGE, ORIGINAL)
    res = {"frames": [FRAMES, ORIGINAL[0], ORIGINAL[1]], "image_size": list(IMAGE), "boxes": n, "runs": runs, "warmup": warmup}
    with torch.no_grad():
        res["predict_boxes"] = compare({"stock": lambda: RH.predict_boxes(*args), "native": lambda: RH.predict_boxes(*args, convs='native')},
                                       runs, warmup)
        res["predict_masks"] = compare({"stock": lambda: RH.predict_masks(*args), "native": lambda: RH.predict_masks(*args, convs='native')},
                                       runs, warmup)
        refined, scores = RH.predict_boxes(*args, convs='native')
        tf = torch.from_numpy(frame).to(dev)
        for name, rows in (("nms_one_frame", slice(0, BOXES_PER_FRAME)), ("nms_batch", slice(0, n))):
            b, s, f = refined[rows].contiguous(), scores[rows].contiguous(), frame[rows]
            paths = {"stock": lambda: nms_torch(b, s, tf[rows], 0.5), "native": lambda: RH.nms_batched(b, s, f, 0.5)}
            res[name] = compare(paths, runs, warmup, clock=host_timed)
            res[name]["same_rows"] = bool(torch.equal(paths["stock"](), paths["native"]()))
            res[name]["clock"] = "host, around a synchronised call (both paths end with a read on the host)"
        # where the native time goes
        b_net = RH.embed_inputs.resize_boxes(args[2], ORIGINAL, IMAGE)
        idx = tf.to(torch.int32)
        p7, p14 = RH.fpn_roi_align(feats, b_net, idx, IMAGE, 7), RH.fpn_roi_align(feats, b_net, idx, IMAGE, 14)
        fc6, fc7 = heads.box_head.fc6, heads.box_head.fc7
        h6 = RH.linear_native(p7.reshape(n, -1), fc6.weight, fc6.bias, True)
        h7 = RH.linear_native(h6, fc7.weight, fc7.bias, True)
        conv = heads.mask_head.convs()[0]
        m1 = conv2d_affine_native(p14, conv.weight, None, conv.bias, relu=True)
        up, last = heads.mask_predictor.conv5_mask, heads.mask_predictor.mask_fcn_logits
        m5 = RH.conv2d_native([m1], up.weight, up.bias, relu=True, transposed=True)
        lg = RH.conv2d_native([m5], last.weight[1:2], last.bias[1:2])
        steps = {
            "fpn_roi_align_7": lambda: RH.fpn_roi_align(feats, b_net, idx, IMAGE, 7),
            "fc6_linear": lambda: RH.linear_native(p7.reshape(n, -1), fc6.weight, fc6.bias, True),
            "fc6_torch": lambda: torch.relu(fc6(p7.reshape(n, -1))),
            "fc7_linear": lambda: RH.linear_native(h6, fc7.weight, fc7.bias, True),
            "box_predict": lambda: RH.box_predict_native(h7, heads.box_predictor, b_net, 1, RH.back_ratios(IMAGE, ORIGINAL)),
            "fpn_roi_align_14": lambda: RH.fpn_roi_align(feats, b_net, idx, IMAGE, 14),
            "mask_fcn_3x3_one_of_four": lambda: conv2d_affine_native(p14, conv.weight, None, conv.bias, relu=True),
            "conv5_mask_transposed": lambda: RH.conv2d_native([m1], up.weight, up.bias, relu=True, transposed=True),
            "mask_fcn_logits_one_channel": lambda: RH.conv2d_native([m5], last.weight[1:2], last.bias[1:2]),
            "roi_mask_finish_up2": lambda: RH.roi_mask_finish_native(lg, 0, 2),
        }
        res["native_steps"] = {}
        for k, fn in steps.items():
            for _ in range(warmup):
                fn()
            res["native_steps"][k] = summary([timed(fn)[0] for _ in range(runs)])
        wbytes = fc6.weight.numel() * 4
        for k in ("fc6_linear", "fc6_torch"):
            res["native_steps"][k]["weight_gbytes_per_s"] = wbytes / (res["native_steps"][k]["median_ms"] * 1e-3) / 1e9
        res["fc6"] = {"rows": n, "k": int(fc6.weight.shape[1]), "n": int(fc6.weight.shape[0]), "weight_mbytes": wbytes / 1e6,
                      "gmac": n * fc6.weight.numel() / 1e9}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rcnn_heads", "timing.json"))
    ap.add_argument("--one", action="store_true", help="measure in this process")
    a = ap.parse_args()
    runs = max(a.runs, 5)
    if a.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("time_rcnn_heads.py needs a GPU")
        return one(runs, a.warmup)
    cmd = [sys.executable, os.path.abspath(__file__), "--one", "--runs", str(runs), "--warmup", str(a.warmup)]
    try:                                       # a child under its own time limit; this process never opens the GPU
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        sys.exit("ran longer than %d s" % a.limit)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit("exit status %d" % p.returncode)
    res = json.loads(line[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
