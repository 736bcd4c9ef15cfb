#!/usr/bin/env python3
"""Time the full-frame mask path on one MI355X against its numpy restatement on the same host: one MOTS20-sized group of frames
(1080 x 1920, 8 frames x 30 detections, boxes around 100 x 250 px, 56 x 56 RoI masks) from RoI masks to COCO strings.

    python tools/full_masks_bench.py [--frames 8] [--dets 30] [--repeats 9] [--cpu-repeats 3]

Device side: ``tracker.to_full_masks`` (paste + arg-max + threshold, run boundaries, two host reads, strings), timed with device
events around a synchronised window after two warm-up calls; the paste kernel alone the same way; medians over the repeats.
Host side: tests/full_masks_ref.py (every mask in an image of its own, np.argmax, threshold, boundaries with numpy) and the same
string code.  The two results are compared before anything is printed.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch
from mpntrackseg_amd import masks as M, tracker
import full_masks_ref as R


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
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--dets", type=int, default=30)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--cpu-repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("full_masks_bench.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    H, W, F, n = a.height, a.width, a.frames, a.frames * a.dets
    rng = np.random.default_rng(20)
    masks = R.blob_masks(rng, n)
    bw, bh = rng.uniform(80, 120, n), rng.uniform(200, 300, n)
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
    boxes = np.stack((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), axis=1)
    frame = np.repeat(np.arange(F), a.dets)
    keep = np.ones(n, bool)
    node_preds = torch.from_numpy(masks).view(n, 1, 56, 56).to(dev)
    boxes_d = torch.from_numpy(boxes).to(dev)
    frame_ptr = torch.arange(0, n + 1, a.dets, dtype=torch.int32, device=dev)

    result = {}

    def full():
        result["rles"] = tracker.to_full_masks(node_preds, boxes_d, frame, keep, (H, W), 0.5, frames_per_launch=F)
    full_ms = device_ms(full, a.repeats)
    paste_ms = device_ms(lambda: M.paste_unique_masks(node_preds, boxes_d, frame_ptr, (H, W), 0.5), a.repeats)
    labels = M.paste_unique_masks(node_preds, boxes_d, frame_ptr, (H, W), 0.5)
    events_ms = device_ms(lambda: M.mask_run_events(labels, n), a.repeats)
    pos, counts = M.mask_run_events(labels, n)

    def host():
        out = []
        for f in range(F):
            sel = slice(f * a.dets, (f + 1) * a.dets)
            lab, _ = R.np_frame(masks[sel], boxes[sel], H, W, 0.5)
            p, c = R.np_events(lab, a.dets)
            ends = np.cumsum(c)
            out += [M.rle_string(M.rle_counts_from_events(p[e - k:e], H * W)) for e, k in zip(ends, c)]
        return out
    cpu_s = []
    for _ in range(a.cpu_repeats):
        t0 = time.perf_counter()
        want = host()
        cpu_s.append(time.perf_counter() - t0)
    same = result["rles"].tolist() == want
    t0 = time.perf_counter()
    ends = np.cumsum(counts)
    for e, k in zip(ends, counts):
        M.rle_string(M.rle_counts_from_events(pos[e - k:e], H * W))
    strings_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({
        "shape": {"frames": F, "detections": n, "height": H, "width": W, "mask": 56},
        "device_to_full_masks_ms": {"median": round(full_ms[0], 3), "min": round(full_ms[1], 3), "max": round(full_ms[2], 3)},
        "device_paste_unique_ms": {"median": round(paste_ms[0], 3), "min": round(paste_ms[1], 3), "max": round(paste_ms[2], 3)},
        "device_run_events_with_host_reads_ms": {"median": round(events_ms[0], 3), "min": round(events_ms[1], 3), "max": round(events_ms[2], 3)},
        "host_strings_ms": round(strings_ms, 3),
        "numpy_restatement_s": {"median": round(statistics.median(cpu_s), 3), "min": round(min(cpu_s), 3), "max": round(max(cpu_s), 3)},
        "run_boundaries": int(counts.sum()),
        "label_workspace_mb": round(4 * H * W * F / 2 ** 20, 1),
        "reference_stack_mb_per_frame": round(4 * H * W * a.dets / 2 ** 20, 1),
        "strings_equal": bool(same),
        "repeats": a.repeats, "cpu_repeats": a.cpu_repeats,
    }))
    if not same:
        raise SystemExit("the device strings differ from the restatement's")


if __name__ == "__main__":
    main()
