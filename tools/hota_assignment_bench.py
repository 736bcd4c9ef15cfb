#!/usr/bin/env python3
"""Time HOTA with the frames' assignment problems on the host (scipy, the default) and on the device
(``assignment.linear_sum_assignment_batched``) on one MI355X, same build, same inputs:

    python tools/hota_assignment_bench.py [--repeats 15] [--frames-per-launch 8]

Two sequences: the ``crowded`` scene of tests/golden/g23_hota.npz (up to 110 x 115 entries a frame) and a synthetic one of 200
frames x 20 objects a side (rectangles on a grid; the predictions moved by up to two pixels, two ids swapped now and then).
``hota_eval.evaluate_hota_files`` is timed with a host clock around a synchronised window after two warm-up calls, the two
routes alternating; medians with their spread over the repeats.  The solver alone: every launch of one device-route evaluation
is replayed through ``mpnhip_lsa_batched`` (its two fills and the kernel) between device events.  The two routes' results are
compared before anything is printed.  Prints one JSON line."""
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
from mpntrackseg_amd import assignment, capi, hota_eval as HE
import hota_ref as HR
import mots_metrics_ref as R


def synthetic(frames, objects, seed=40):
    """(pred, gt) as ``mots_eval.load_mots_txt`` returns them: ``objects`` rectangles a frame on a 4-column grid"""
    rng = np.random.default_rng(seed)
    cols = 4
    rows = -(-objects // cols)
    ch, cw = 24, 32
    H, W = rows * ch, cols * cw

    def side(shift, swap):
        out = {k: [] for k in ("frame", "track_id", "class_id", "run_row", "run_begin", "run_end")}
        for f in range(frames):
            ids = np.arange(objects)
            if swap and f % 7 == 3:
                ids[[0, 1]] = ids[[1, 0]]
            for o in range(objects):
                dy, dx = (rng.integers(0, 3, 2) if shift else (0, 0))
                y0, x0 = (o // cols) * ch + 3 + dy, (o % cols) * cw + 3 + dx
                xs = np.arange(x0, x0 + cw - 10)
                out["run_row"].append(np.full(xs.size, len(out["frame"]), np.int64))
                out["run_begin"].append(xs * H + y0)
                out["run_end"].append(xs * H + y0 + ch - 10)
                out["frame"].append(f); out["track_id"].append(2001 + int(ids[o])); out["class_id"].append(2)
        n = len(out["frame"])
        d = {k: (np.concatenate(v) if k.startswith("run") else np.asarray(v)).astype(np.int64) for k, v in out.items()}
        d["h"], d["w"] = np.full(n, H, np.int64), np.full(n, W, np.int64)
        d["area"] = np.bincount(d["run_row"], weights=d["run_end"] - d["run_begin"], minlength=n).astype(np.int64)
        return d
    return side(True, True), side(False, False), frames


def spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def time_routes(pred, gt, T, fpl, repeats, dev):
    run = lambda how: HE.evaluate_hota_files(pred, gt, T, frames_per_launch=fpl, device=dev, assignment=how)
    results = {how: run(how) for how in ("host", "device")}
    for how in ("host", "device"):
        run(how)
    times = {"host": [], "device": []}
    for _ in range(repeats):
        for how in ("host", "device"):   # (alternating: whatever else the host is doing falls on both)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(how)
            torch.cuda.synchronize()
            times[how].append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(results["host"][k], results["device"][k]) for k in HE.INTEGER_ARRAY_FIELDS + HE.COUNT_FIELDS) and \
        all(np.allclose(results["host"][k], results["device"][k], rtol=1e-9, atol=1e-12) for k in HE.FLOAT_ARRAY_FIELDS + HE.FLOAT_FIELDS)
    return {how: spread(ms) for how, ms in times.items()}, same


def solver_launches(pred, gt, T, fpl, dev, iters=20):
    """device time of mpnhip_lsa_batched for every launch of one evaluation: (frames, cells, us per call)"""
    calls, wrapped = [], assignment.linear_sum_assignment_batched

    def record(*a, **kw):
        calls.append((a, kw))
        return wrapped(*a, **kw)
    assignment.linear_sum_assignment_batched = record
    try:
        HE.evaluate_hota_files(pred, gt, T, frames_per_launch=fpl, device=dev, assignment="device")
    finally:
        assignment.linear_sum_assignment_batched = wrapped
    lib, out = capi.load(), []
    for (cost, cp, ap, bp, ka, kb), kw in calls:
        ka, kb = ka.to(torch.uint8), kb.to(torch.uint8)
        n_a, n_b, F = ka.numel(), kb.numel(), ap.numel() - 1
        mb, ma, st = (torch.empty(max(n, 1), dtype=torch.int32, device=dev) for n in (n_a, n_b, F))
        ws = capi.workspace(lib.mpnhip_lsa_workspace_bytes(n_a, n_b, F), dev, "lsa")
        call = lambda: capi.check(lib.mpnhip_lsa_batched(capi.ptr(cost), cost.numel(), capi.ptr(cp), capi.ptr(ap), n_a, capi.ptr(bp), n_b, F,
                                                         capi.ptr(ka), capi.ptr(kb), 1, capi.ptr(mb), capi.ptr(ma), capi.ptr(st),
                                                         capi.ptr(ws), ws.numel(), capi.stream_ptr()), "mpnhip_lsa_batched")
        call()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            call()
        stop.record()
        torch.cuda.synchronize()
        out.append((F, int(cost.numel()), start.elapsed_time(stop) * 1e3 / iters))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--frames-per-launch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--objects", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hota_assignment_bench.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    gold, gold22 = dict(np.load(HR.GOLDEN)), dict(np.load(R.GOLDEN))
    out, ok = {"frames_per_launch": a.frames_per_launch, "repeats": a.repeats}, True
    with tempfile.TemporaryDirectory() as tmp:
        import pathlib
        from mpntrackseg_amd.mots_eval import load_mots_txt
        pred, gt, T = HR.scene_files(gold, gold22, "crowded", pathlib.Path(tmp))
        cases = {"crowded": (load_mots_txt(pred), load_mots_txt(gt), T),
                 "synthetic_%dx%d" % (a.frames, a.objects): synthetic(a.frames, a.objects)}
    for name, (pred, gt, T) in cases.items():
        ms, same = time_routes(pred, gt, T, a.frames_per_launch, a.repeats, dev)
        launches = solver_launches(pred, gt, T, a.frames_per_launch, dev)
        us = [u for _, _, u in launches]
        out[name] = {"frames": T, "evaluate_hota_files_ms": ms, "results_equal": bool(same), "solver_launches": len(launches),
                     "solver_launch_us": {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)},
                     "solver_all_launches_ms": round(sum(us) / 1e3, 3), "largest_launch_cells": max(c for _, c, _ in launches)}
        ok = ok and same
    print(json.dumps(out))
    if not ok:
        raise SystemExit("the two routes' results differ")


if __name__ == "__main__":
    main()
