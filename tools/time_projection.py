#!/usr/bin/env python3
"""Time of ``projectors.exact_round`` with the default host LP solver (``pulp`` if it imports, else scipy's HiGHS) and with
``solver='device'`` (the LP as batched linear assignment, csrc/exact_projection.hip + ``mpnhip_lsa_batched``), on two inputs:

  hub     the ``hub`` case of tests/golden/g19_projection.npz: 650 nodes, one component of 548 x 537 (294,276 cost cells)
  small   ``--copies`` (default 3000) disjoint copies of the three-edge graph [[0,0,1],[3,4,3]] with scores .9 .8 .85 in a random
          edge order: that many components of 2 x 2

Both paths read from the device (the host path copies the sub-problem down and the values back, the device path reads two
small blocks of integers), so a call is timed with a host clock around the call and a device synchronise.  The two paths are
timed in the same process, alternating, after ``--warmup`` calls each; reported are the median and the min .. max of at least 20
calls, the rounded vectors are compared (equal where the optimum is unique: both inputs), and the objective of either is given.

Writes profiles/projection/timing.json (or --out).  Needs a GPU: there is no CPU fall-back."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from mpntrackseg_amd import projectors


def hub():
    z = np.load(os.path.join(REPO, "tests", "golden", "g19_projection.npz"))
    return z["hub:edge_index"], z["hub:edge_preds"], int(z["hub:num_nodes"])


def small(copies, seed=5):
    ei = np.array([[0, 0, 1], [3, 4, 3]], np.int64)
    ei = np.concatenate([ei + 5 * i for i in range(copies)], axis=1)
    p = np.tile(np.array([0.9, 0.8, 0.85], np.float32), copies)
    perm = np.random.default_rng(seed).permutation(p.size)
    return np.ascontiguousarray(ei[:, perm]), p[perm], 5 * copies


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--copies", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "projection", "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_projection.py needs a GPU")
    runs = max(a.runs, 20)
    dev = torch.device("cuda:0")
    res = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "runs": runs, "warmup": a.warmup,
           "host_solver": projectors.default_solver().__name__}
    for name, (ei, p, n) in (("hub", hub()), ("small", small(a.copies))):
        t_ei, t_p = torch.from_numpy(ei).to(dev), torch.from_numpy(p).to(dev)
        paths = {"host": lambda: projectors.exact_round(t_ei, t_p, n)[0], "device": lambda: projectors.exact_round(t_ei, t_p, n, solver='device')[0]}
        out, times = {}, {k: [] for k in paths}
        for k, fn in paths.items():
            for _ in range(a.warmup):
                out[k] = fn()
        for _ in range(runs):
            for k, fn in paths.items():      # alternating: both paths see the same neighbours on the machine
                ms, out[k] = timed(fn)
                times[k].append(ms)
        plan = projectors.exact_plan(t_ei, t_p, n)
        cost = 1.0 - 2.0 * t_p.double()
        r = {"nodes": n, "edges": int(p.size), "problems": plan.n_problems, "max_side": plan.max_side, "cells": plan.cells,
             "equal_vectors": bool(torch.equal(out["host"], out["device"]))}
        for k, ts in times.items():
            r[k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "objective": float((cost * out[k].double()).sum())}
        r["device_over_host_median"] = r["device"]["median_ms"] / r["host"]["median_ms"]
        res[name] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
