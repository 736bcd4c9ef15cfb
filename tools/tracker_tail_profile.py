#!/usr/bin/env python3
"""Per-kernel times of the sliding-window tail (csrc/tracker_tail.hip) from a kernel trace.

  run:     rocprofv3 --kernel-trace --stats -d DIR -o tail -- python tools/tracker_tail_profile.py run
           evaluates the longer sequence of tests/golden/g17_window_tail.npz (104 nodes, 10,088 directed edges, 12 windows)
           WARM + 1 times with tracker.evaluate_sequence, then launches mpnhip_node_mask_accumulate alone SYNTH times on a
           user-scale window (500 nodes x 3136); a marker kernel (mpnhip_threshold_flags on MARK elements) separates the phases.
  report:  python tools/tracker_tail_profile.py report DIR > profiles/tracker_tail/README.md
           reads the kernel trace under DIR: the tail's kernels in the LAST evaluate_sequence call and the synthetic launches,
           with the bytes they move computed from the shapes.

No counters and nothing else traced in that run; end-to-end times belong to a run without the profiler."""
import csv
import glob
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WARM, SYNTH, MARK = 2, 20, 77777
SYNTH_ROWS, ROW_LEN = 500, 3136
HBM_MEASURED = 6.29e12   # bytes/s, float4 copy (MI355X_MICROARCH.md); spec 8.0e12
TAIL_KERNELS = ("k_node_accumulate", "k_node_average", "k_pair_keys", "k_run_heads", "k_inverse", "k_merge_fill", "k_threshold")


def run():
    import torch
    from mpntrackseg_amd import capi, synth, tracker
    from mpntrackseg_amd.mpn import MOTMPNet
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(REPO, "tests", "golden", "g17_window_tail.npz"))
    params = dict(synth.model_params(32, 4, "sum", num_class_steps=2, node_in_dim=64))
    W = synth.make_weights(params, seed=7, gain=0.6)
    W.update(synth.make_mask_weights(seed=17))
    params.update(synth.MASK_PARAMS)
    model = MOTMPNet(params)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    model = model.to(dev).eval()
    t = [torch.from_numpy(z[f"l:{k}"]).to(dev) for k in ("x", "edge_index", "edge_attr", "reid_emb_dists")]
    n = t[0].shape[0]
    x_ext = torch.from_numpy(synth.normal(9, (n, 256, 14, 14), stream=1, std=0.5)).to(dev)
    inactive, recip, fpg, top_k = [int(v) for v in z["l1:cfg"]]
    lib = capi.load()
    mark_src = torch.zeros(MARK, device=dev)
    mark_dst = torch.empty(MARK, dtype=torch.uint8, device=dev)

    def mark():
        capi.check(lib.mpnhip_threshold_flags(capi.ptr(mark_src), MARK, 0.5, capi.ptr(mark_dst), capi.stream_ptr()), "mark")

    for _ in range(WARM + 1):
        mark()
        res = tracker.evaluate_sequence(model, *t, z["l:frame"], fpg, top_k, reciprocal_k_nns=bool(recip),
                                        set_pruned_edges_to_inactive=bool(inactive), x_ext=x_ext)
        torch.cuda.synchronize()
    mark()
    logits = torch.randn((SYNTH_ROWS, ROW_LEN), device=dev)
    overall = torch.zeros((2 * SYNTH_ROWS, ROW_LEN), device=dev)
    count = torch.zeros(2 * SYNTH_ROWS, device=dev)
    for _ in range(SYNTH):
        capi.check(lib.mpnhip_node_mask_accumulate(capi.ptr(logits), SYNTH_ROWS, ROW_LEN, 100, 2 * SYNTH_ROWS, capi.ptr(overall),
                                                   capi.ptr(count), capi.stream_ptr()), "mpnhip_node_mask_accumulate")
    torch.cuda.synchronize()
    print("evaluated: kept", res.edge_index.shape[1], "pairs; node_preds", tuple(res.node_preds.shape))


def report(directory):
    rec = _dispatches(directory)
    marks = [i for i, (name, _, grid) in enumerate(rec) if "k_threshold" in name and grid >= MARK]
    assert len(marks) == WARM + 2, len(marks)
    last, synth = rec[marks[-2] + 1:marks[-1]], rec[marks[-1] + 1:]
    z = np.load(os.path.join(REPO, "tests", "golden", "g17_window_tail.npz"))
    n, E = z["l:frame"].shape[0], z["l:edge_index"].shape[1]
    print("# Sliding-window tail: per-kernel times (rocprofv3 --kernel-trace --stats, a run of its own)\n")
    print("`tools/tracker_tail_profile.py`; `tracker.evaluate_sequence` on the longer sequence of `tests/golden/g17_window_tail.npz`")
    print("(%d nodes, %d directed edges, configuration l1), the call after %d warm-up calls.  One call launches %d kernels in all"
          % (n, E, WARM, len(last)))
    print("(hot path, attention, convolutions, kNN, ...), %.0f us of kernel time; the tail's own:\n" % (sum(d for _, d, _ in last) / 1e3))
    print("| kernel | launches | total us | mean us |\n|---|---|---|---|")
    for k in TAIL_KERNELS:
        d = [dur for name, dur, _ in last if k in name]
        if d:
            print("| `%s` | %d | %.1f | %.2f |" % (k, len(d), sum(d) / 1e3, np.mean(d) / 1e3))
    acc = [dur for name, dur, _ in last if "k_node_accumulate" in name]
    avg = [dur for name, dur, _ in last if "k_node_average" in name]
    print("\nBytes from the shapes: an accumulate launch reads the window's logits and reads and writes the same rows of the accumulator,")
    print("3 x rows x 3136 x 4 B; the average reads and writes all %d rows, 2 x %d x 3136 x 4 B = %.2f MB." % (n, n, 2 * n * ROW_LEN * 4 / 1e6))
    if acc:
        windows = [(int(a), int(b)) for a, b in _windows(z)]
        bts = sum(3 * (b - a) * ROW_LEN * 4 for a, b in windows)
        print("Accumulate: %d launches, %.2f MB in %.1f us = %.3f TB/s = %.1f %% of the measured HBM copy rate (6.29 TB/s; spec 8.0)."
              % (len(acc), bts / 1e6, sum(acc) / 1e3, bts / (sum(acc) * 1e-9) / 1e12, 100 * bts / (sum(acc) * 1e-9) / HBM_MEASURED))
    if avg:
        bts = 2 * n * ROW_LEN * 4
        print("Average: %.2f MB in %.1f us = %.3f TB/s = %.1f %% of it."
              % (bts / 1e6, sum(avg) / 1e3, bts / (sum(avg) * 1e-9) / 1e12, 100 * bts / (sum(avg) * 1e-9) / HBM_MEASURED))
    print("\n**At this size these figures measure launch overhead, not bandwidth**: a window is 20-50 rows (0.25-0.6 MB), a few")
    print("microseconds of kernel time whatever the memory system could do, and the data sits in the caches.\n")
    sy = [dur for name, dur, _ in synth if "k_node_accumulate" in name]
    if sy:
        bts = 3 * SYNTH_ROWS * ROW_LEN * 4
        best, med = min(sy), float(np.median(sy))
        print("The accumulate kernel alone at a user-scale window (%d nodes x %d, %.1f MB moved per launch, %d launches back to back):"
              % (SYNTH_ROWS, ROW_LEN, bts / 1e6, len(sy)))
        print("median %.1f us = %.2f TB/s (%.0f %% of the measured copy rate), best %.1f us.  The 18.8 MB working set fits the 256 MiB"
              % (med / 1e3, bts / (med * 1e-9) / 1e12, 100 * bts / (med * 1e-9) / HBM_MEASURED, best / 1e3))
        print("Infinity Cache, so this is a cache-resident rate, not an HBM one; it is the kernel's rate at the size a user runs.")


def _dispatches(directory):
    """[(kernel name, duration ns, grid size)] in start order, from the trace rocprofv3 left under ``directory``: the rocpd
    database (its default output) or the CSV of --output-format csv."""
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    if dbs:
        import sqlite3
        return [(name, end - start, grid) for name, start, end, grid in
                sqlite3.connect(dbs[0]).execute("select name, start, end, grid_x from kernels order by start")]
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, paths
    rows = sorted(csv.DictReader(open(paths[0])), key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0))
            for r in rows]


def _windows(z):
    from mpntrackseg_amd.tracker import frame_windows
    return frame_windows(z["l:frame"], int(z["l1:cfg"][2]))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 3 and sys.argv[1] == "report":
        report(sys.argv[2])
    else:
        sys.exit(__doc__)
