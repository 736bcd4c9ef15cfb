#!/usr/bin/env python3
"""Time the batched COCO run-length codec on one MI355X against the host codec it replaces, through its two consumers:

  encode   ``tracker.to_full_masks`` over one MOTS20-sized group of frames (the shape of tools/full_masks_bench.py: 1080 x 1920,
           8 frames x 30 detections) with ``strings='host'`` (one numpy ``rle_string`` per detection) and ``strings='device'``;
  decode   ``mots_eval.load_mots_txt`` of a generated file of 4,000 elliptical masks at 1080 x 1920 (one run per column, one mask
           per frame) on the host path and with ``device=``; and, of the device path, the host's shares: splitting the lines, and the
           check for overlapping masks both paths end with.

    python tools/time_rle_codec.py [--masks 4000] [--repeats 9] [--out profiles/rle_codec/timing.json]

Every window is synchronised before and behind and timed with device events; the two paths of a pair alternate inside one loop,
after two warm-up calls each; median, min and max over the repeats.  The results of both pairs are compared for equality before
anything is printed.  Prints one JSON line and, with ``--out``, stores it."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch
from mpntrackseg_amd import masks as M, mots_eval as ME, tracker
import full_masks_ref as R


def window_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop), out


def alternate(fns, repeats, warmup=2):
    """the windows of several functions, taken in turns: {name: ([ms], last result)}"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times, last = {k: [] for k in fns}, {}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms, last[k] = window_ms(fn)
            times[k].append(ms)
    return times, last


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def ellipse_rows(n, H, W, seed=21):
    """MOTS rows of ``n`` elliptical masks, one per frame, built from their columns' runs (no dense image)"""
    rng = np.random.default_rng(seed)
    rows, runs = [], 0
    for i in range(n):
        rx, ry = rng.uniform(20, 55), rng.uniform(60, 160)
        cx, cy = rng.uniform(rx + 1, W - rx - 1), rng.uniform(ry + 1, H - ry - 1)
        xs = np.arange(int(np.ceil(cx - rx)), int(np.floor(cx + rx)) + 1)
        half = ry * np.sqrt(np.maximum(0.0, 1.0 - ((xs - cx) / rx) ** 2))
        y0, y1 = np.ceil(cy - half).astype(np.int64), np.floor(cy + half).astype(np.int64) + 1
        ok = y1 > y0
        events = np.stack((xs[ok] * H + y0[ok], xs[ok] * H + y1[ok]), axis=1).reshape(-1)
        runs += int(ok.sum())
        rows.append("%d %d 2 %d %d %s" % (i, 2001 + i % 900, H, W, M.rle_string(M.rle_counts_from_events(events, H * W))))
    return rows, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--dets", type=int, default=30)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--masks", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rle_codec.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    H, W, F, n = a.height, a.width, a.frames, a.frames * a.dets

    # ---- encode: the inputs of tools/full_masks_bench.py
    rng = np.random.default_rng(20)
    masks = R.blob_masks(rng, n)
    bw, bh = rng.uniform(80, 120, n), rng.uniform(200, 300, n)
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
    boxes_d = torch.from_numpy(np.stack((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), axis=1)).to(dev)
    frame, keep = np.repeat(np.arange(F), a.dets), np.ones(n, bool)
    node_preds = torch.from_numpy(masks).view(n, 1, 56, 56).to(dev)
    full = lambda strings: tracker.to_full_masks(node_preds, boxes_d, frame, keep, (H, W), 0.5, frames_per_launch=F, strings=strings)
    enc_ms, enc_out = alternate({"host": lambda: full("host"), "device": lambda: full("device")}, a.repeats)
    enc_same = enc_out["host"].tolist() == enc_out["device"].tolist()
    labels = M.paste_unique_masks(node_preds, boxes_d, torch.arange(0, n + 1, a.dets, dtype=torch.int32, device=dev), (H, W), 0.5)
    tail_ms, tail_out = alternate({"events_and_host_strings": lambda: M.mask_run_events(labels, n),
                                   "device_strings": lambda: M.mask_run_strings(labels, n)}, a.repeats)
    pos, counts = tail_out["events_and_host_strings"]

    # ---- decode: a generated file
    rows, n_runs = ellipse_rows(a.masks, H, W)
    chars = sum(len(r.split(" ")[5]) for r in rows)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "masks.txt")
        with open(path, "w") as fh:
            fh.write("".join(r + "\n" for r in rows))
        dec_ms, dec_out = alternate({"host": lambda: ME.load_mots_txt(path), "device": lambda: ME.load_mots_txt(path, device=dev)},
                                    a.repeats)
        split_s = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            cols, strings, _, _ = ME._split_mots_rows(path)
            split_s.append((time.perf_counter() - t0) * 1e3)
    want = dec_out["host"]
    overlap_ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ME.refuse_overlapping_masks(want["frame"], want["run_row"], want["run_begin"], want["run_end"])
        overlap_ms.append((time.perf_counter() - t0) * 1e3)
    codec_ms, _ = alternate({"rle_decode_batch": lambda: M.rle_decode_batch(strings, cols[:, 3], cols[:, 4], dev)}, a.repeats)
    want, got = dec_out["host"], dec_out["device"]
    dec_same = list(want) == list(got) and all(want[k].dtype == got[k].dtype and np.array_equal(want[k], got[k]) for k in want)

    med = lambda ms: statistics.median(ms)
    line = {
        "encode": {
            "shape": {"frames": F, "detections": n, "height": H, "width": W, "mask": 56, "run_boundaries": int(counts.sum())},
            "to_full_masks_host_strings_ms": stats(enc_ms["host"]),
            "to_full_masks_device_strings_ms": stats(enc_ms["device"]),
            "ratio_host_over_device": round(med(enc_ms["host"]) / med(enc_ms["device"]), 2),
            "run_events_with_host_reads_ms": stats(tail_ms["events_and_host_strings"]),
            "run_strings_with_host_reads_ms": stats(tail_ms["device_strings"]),
            "strings_equal": bool(enc_same),
        },
        "decode": {
            "shape": {"masks": a.masks, "height": H, "width": W, "characters": chars, "runs": n_runs},
            "load_mots_txt_host_ms": stats(dec_ms["host"]),
            "load_mots_txt_device_ms": stats(dec_ms["device"]),
            "ratio_host_over_device": round(med(dec_ms["host"]) / med(dec_ms["device"]), 2),
            "host_line_splitting_ms": stats(split_s),
            "line_splitting_share_of_device_path": round(med(split_s) / med(dec_ms["device"]), 3),
            "host_overlap_check_ms": stats(overlap_ms),
            "rle_decode_batch_with_copies_ms": stats(codec_ms["rle_decode_batch"]),
            "dicts_equal": bool(dec_same),
        },
        "repeats": a.repeats,
    }
    text = json.dumps(line)
    if not (enc_same and dec_same):
        raise SystemExit("the device codec's results differ from the host codec's")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
