#!/usr/bin/env python3
"""Per-kernel times of the projection onto trajectories (csrc/projection.hip) from a kernel trace.

  run:     rocprofv3 --kernel-trace --stats -d DIR -o projection -- python tools/projection_profile.py run
           the hub case of tests/golden/g19_projection.npz (650 nodes, 2,633 edges, one node with > 256 active edges on each
           side): projectors.greedy_round, tracker.assign_ped_ids and tracker.drop_short_trajectories WARM + 1 times, then the
           same on a random graph of LARGE_N nodes and LARGE_K edges; a marker kernel (mpnhip_threshold_flags on MARK elements)
           separates the phases.
  report:  python tools/projection_profile.py report DIR > profiles/projection/README.md
           reads the kernel trace under DIR: the kernels of the LAST repetition of either phase.

No counters and nothing else traced in that run; end-to-end times belong to a run without the profiler."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WARM, MARK = 2, 77777
LARGE_N, LARGE_K = 200000, 2000000
KERNELS = ("k_round_count", "k_constraint_counts", "k_argmax", "k_keep_winner", "k_cc_init", "k_cc_union", "k_cc_roots", "k_cc_labels",
           "k_label_count", "k_label_keep")


def _large():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, LARGE_N, LARGE_K), rng.integers(0, LARGE_N, LARGE_K)
    sel = a != b
    ei = np.stack((np.minimum(a, b)[sel], np.maximum(a, b)[sel])).astype(np.int64)
    return ei, rng.random(ei.shape[1]).astype(np.float32), LARGE_N


def run():
    import torch
    from mpntrackseg_amd import capi, projectors, tracker
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(REPO, "tests", "golden", "g19_projection.npz"))
    lib = capi.load()
    mark_src = torch.zeros(MARK, device=dev)
    mark_dst = torch.empty(MARK, dtype=torch.uint8, device=dev)

    def mark():
        capi.check(lib.mpnhip_threshold_flags(capi.ptr(mark_src), MARK, 0.5, capi.ptr(mark_dst), capi.stream_ptr()), "mark")

    for ei, p, n in ((z["hub:edge_index"], z["hub:edge_preds"], int(z["hub:num_nodes"])), _large()):
        t_ei, t_p = torch.from_numpy(ei).to(dev), torch.from_numpy(p).to(dev)
        for _ in range(WARM + 1):
            mark()
            rounded, rate = projectors.greedy_round(t_ei, t_p, n)
            ids = tracker.assign_ped_ids(t_ei, rounded, n)
            keep = tracker.drop_short_trajectories(ids, 2)
            torch.cuda.synchronize()
        print("nodes", n, "edges", ei.shape[1], "rate", rate, "active", int(rounded.sum()), "tracks", int(ids.max()) + 1, "kept", int(keep.sum()))
    mark()
    torch.cuda.synchronize()


def report(directory):
    from tracker_tail_profile import _dispatches
    rec = _dispatches(directory)
    marks = [i for i, (name, _, grid) in enumerate(rec) if "k_threshold" in name and grid >= MARK]
    assert len(marks) == 2 * (WARM + 1) + 1, len(marks)
    phases = (("the hub case of `tests/golden/g19_projection.npz` (650 nodes, 2,633 edges, a node with > 256 active edges on each side)",
               rec[marks[WARM] + 1:marks[WARM + 1]]),
              ("a random graph of %d nodes and about %d edges (uniform scores)" % (LARGE_N, LARGE_K), rec[marks[-2] + 1:marks[-1]]))
    print("# Projection onto trajectories: per-kernel times (rocprofv3 --kernel-trace --stats, a run of its own)\n")
    print("`tools/projection_profile.py`; `projectors.greedy_round`, `tracker.assign_ped_ids` and `tracker.drop_short_trajectories`,")
    print("the repetition after %d warm-up repetitions.\n" % WARM)
    for title, part in phases:
        print("On %s: %d kernels, %.1f us of kernel time (memsets, the scan and torch's own kernels included); this file's:\n"
              % (title, len(part), sum(d for _, d, _ in part) / 1e3))
        print("| kernel | launches | total us | mean us |\n|---|---|---|---|")
        for k in KERNELS:
            d = [dur for name, dur, _ in part if k in name]
            if d:
                print("| `%s` | %d | %.1f | %.2f |" % (k, len(d), sum(d) / 1e3, np.mean(d) / 1e3))
        print()


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 3 and sys.argv[1] == "report":
        report(sys.argv[2])
    else:
        sys.exit(__doc__)
