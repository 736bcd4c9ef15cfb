#!/usr/bin/env python3
"""Time of the two embedding-input operators (mpntrackseg_amd.embed_inputs) at the workload's shapes, 50 boxes per frame:

fpn_roi_align   C = 256, S = 14, sampling_ratio 2, the four levels of an 800 x 1333 image (200 x 336 .. 25 x 42), with the
                detection-id channel: output bytes per second, beside a device-to-device copy of the same byte count timed in
                the same run, alternating with it;
reid_crops      1080 x 1920 frames to 128 x 64: patches per second, and beside it the reference's pipeline on the host
                (numpy's pad, PIL's resize, ToTensor and Normalize in numpy) when PIL can be imported.

Every call is timed with device events after warm-up calls; reported are the median and the min .. max.  "call" is the public
function as a user calls it: the per-box host work (geometry, box mapping, levels) and the upload of its few integers per box
included.  "launch" is the C entry point alone on arguments already on the device -- the operator's kernels, which is what the
copy is compared with.  One process; every step
runs under its own time limit (an alarm that ends the process).  Prints one JSON line (and writes it to --out when given).
Needs a GPU: there is no CPU fall-back."""
import argparse
import ctypes
import json
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mpntrackseg_amd import capi, embed_inputs as E
from mpntrackseg_amd.capi import check, ptr, stream_ptr

IMAGE, ORIGINAL = (800, 1333), (1080, 1920)
LEVELS = ((200, 336), (100, 168), (50, 84), (25, 42))
CHANNELS, S, BOXES_PER_FRAME = 256, 14, 50


class step:
    """a time limit of its own for one step: the alarm's default action ends the process"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def pedestrian_boxes(n_frames, rng):
    """50 boxes per frame: 30 .. 220 wide, 2 .. 3 times as tall, a tenth of them over an edge of the frame"""
    n = n_frames * BOXES_PER_FRAME
    w = rng.uniform(30, 220, n)
    h = w * rng.uniform(2.0, 3.0, n)
    left, top = rng.uniform(-0.1 * w, ORIGINAL[1] - 0.9 * w, n), rng.uniform(-0.05 * h, ORIGINAL[0] - 0.95 * h, n)
    return np.stack([left, top, left + w, top + h], axis=1), np.repeat(np.arange(n_frames), BOXES_PER_FRAME)


def timed(fn, runs):
    ts = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    return ts


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def roi_launcher(feats, boxes, box_frame, ids, out):
    """mpnhip_fpn_roi_align alone: the arguments fpn_roi_align makes, made once"""
    lib, dev = capi.load(), out.device
    b, scales, levels = E.map_boxes(boxes, [f.shape[2:] for f in feats], IMAGE, ORIGINAL)
    lv = capi.FpnLevels()
    for l, f in enumerate(feats):
        lv.data[l], lv.h[l], lv.w[l], lv.scale[l] = f.data_ptr(), int(f.shape[2]), int(f.shape[3]), scales[l]
    keep = [b.to(dev), torch.from_numpy(box_frame.astype(np.int32)).to(dev), levels.to(torch.int32).to(dev),
            torch.from_numpy(ids.astype(np.int32)).to(dev), lv]
    n, B = b.shape[0], feats[0].shape[0]
    return lambda: check(lib.mpnhip_fpn_roi_align(ctypes.byref(keep[4]), B, CHANNELS, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), n, S, 2,
                                                  ptr(keep[3]), ptr(out), stream_ptr()), "mpnhip_fpn_roi_align")


def crops_launcher(frames, boxes, box_frame, out):
    """mpnhip_reid_crops alone (its three kernels), all boxes in one call"""
    lib, dev = capi.load(), frames.device
    B, H, W = frames.shape[:3]
    g = E.crop_geometry(boxes, H, W)
    max_ph, max_pw = int((g[:, 4] + g[:, 1] - g[:, 0] + g[:, 5]).max()), int((g[:, 6] + g[:, 3] - g[:, 2] + g[:, 7]).max())
    ws = torch.empty(lib.mpnhip_reid_crops_workspace_bytes(len(g), max_ph, max_pw, 128, 64), dtype=torch.uint8, device=dev)
    gd, fd = torch.from_numpy(g).to(dev), torch.from_numpy(box_frame.astype(np.int32)).to(dev)
    ms = (ctypes.c_float * 6)(*(E.IMAGENET_MEAN + E.IMAGENET_STD))
    return lambda: check(lib.mpnhip_reid_crops(ptr(frames), B, H, W, ptr(gd), ptr(fd), len(g), max_ph, max_pw, 128, 64, ms, ptr(out), None,
                                               ptr(ws), ws.numel(), stream_ptr()), "mpnhip_reid_crops")


def host_pipeline(frames, boxes, box_frame):
    from PIL import Image
    mean, std = np.asarray(E.IMAGENET_MEAN, np.float32).reshape(3, 1, 1), np.asarray(E.IMAGENET_STD, np.float32).reshape(3, 1, 1)
    H, W = frames.shape[1:3]
    out = np.empty((len(boxes), 3, 128, 64), np.float32)
    for k, (left, top, right, bot) in enumerate(boxes):
        img = frames[box_frame[k], int(max(0, top)):int(max(0, bot)), int(max(0, left)):int(max(0, right))]
        pads = ((int(abs(top - max(top, 0))), int(abs(bot - min(bot, H)))), (int(abs(left - max(left, 0))), int(abs(right - min(right, W)))), (0, 0))
        img = np.asarray(Image.fromarray(np.pad(img, pads, mode="mean")).resize((64, 128), Image.BILINEAR))
        out[k] = (img.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - mean) / std
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_embed_inputs.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    boxes, box_frame = pedestrian_boxes(a.frames, rng)
    n = len(boxes)
    res = {"frames": a.frames, "boxes": n, "runs": a.runs, "warmup": a.warmup}

    with step(120):
        feats = [torch.randn((a.frames, CHANNELS) + s, device=dev) for s in LEVELS]
        ids = np.arange(n)
        roi = lambda: E.fpn_roi_align(feats, boxes, box_frame, IMAGE, ORIGINAL, S, 2, detection_id=ids)
        out = roi()
        nbytes = out.numel() * 4
        src, dst = torch.randn_like(out), torch.empty_like(out)
        copy = lambda: dst.copy_(src)
        launch = roi_launcher(feats, boxes, box_frame, ids, dst)
        launch()
        same = bool(torch.equal(dst, out))
        for _ in range(a.warmup):
            roi()
            launch()
            copy()
        torch.cuda.synchronize()
    with step(300):
        t_roi, t_launch, t_copy = [], [], []
        for _ in range(a.runs):                # alternating: all see the same neighbours on the machine
            t_roi += timed(roi, 1)
            t_launch += timed(launch, 1)
            t_copy += timed(copy, 1)
    res["fpn_roi_align"] = {"shape": list(out.shape), "output_bytes": nbytes, "call": summary(t_roi), "launch": summary(t_launch),
                            "copy": summary(t_copy), "launch_equals_call": same,
                            "call_output_bytes_per_s": nbytes / (statistics.median(t_roi) * 1e-3),
                            "launch_output_bytes_per_s": nbytes / (statistics.median(t_launch) * 1e-3),
                            "copy_bytes_per_s": nbytes / (statistics.median(t_copy) * 1e-3),
                            "launch_share_of_copy_rate": statistics.median(t_copy) / statistics.median(t_launch)}
    del feats, src, dst, out

    with step(120):
        frames_host = rng.integers(0, 256, (a.frames,) + ORIGINAL + (3,), dtype=np.uint8)
        frames = torch.from_numpy(frames_host).to(dev)
        crops = lambda: E.reid_crops(frames, boxes, box_frame)
        patches = torch.empty((n, 3, 128, 64), dtype=torch.float32, device=dev)
        launch = crops_launcher(frames, boxes, box_frame, patches)
        launch()
        same = bool(torch.equal(patches, crops()))
        for _ in range(a.warmup):
            crops()
            launch()
        torch.cuda.synchronize()
    with step(300):
        t_crops, t_launch = [], []
        for _ in range(a.runs):
            t_crops += timed(crops, 1)
            t_launch += timed(launch, 1)
    res["reid_crops"] = {"shape": [n, 3, 128, 64], "call": summary(t_crops), "launch": summary(t_launch), "launch_equals_call": same,
                         "call_patches_per_s": n / (statistics.median(t_crops) * 1e-3),
                         "launch_patches_per_s": n / (statistics.median(t_launch) * 1e-3)}
    try:
        import PIL
    except ImportError:
        res["host_pipeline"] = None
    else:
        with step(600):
            host_pipeline(frames_host, boxes[:20], box_frame[:20])
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                host_pipeline(frames_host, boxes, box_frame)
                ts.append((time.perf_counter() - t0) * 1e3)
        res["host_pipeline"] = {"pillow": PIL.__version__, "call": summary(ts), "patches_per_s": n / (statistics.median(ts) * 1e-3),
                                "threads": 1}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
