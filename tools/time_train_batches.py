#!/usr/bin/env python3
"""Time of one training batch of graphs built on the device (mpntrackseg_amd.train_batch.build_batch) against a loop over the
same samples through the package's single-graph functions (graph.construct_graph(inference_mode=False), assign_edge_labels,
gather_rows, the box shifts in numpy, torch.cat with node offsets) -- the loop is code the package had before build_batch, so
both sides run in this one process, alternating.

Synthetic sequences at the reference's configuration (configs/tracking_cfg.yaml): frames_per_graph 15, max_detects 500,
top_k_nns 150, reciprocal, max_frame_dist 'max', the augmentation ranges of the config switched on; batch_size 8; --dets
detections per frame (default 25: 375 nodes and about 50 000 edges per graph before the pruning).

"build_batch" and "loop" are host-clock times of the whole call, ended by a device synchronise: both contain host reads, so
an event pair would miss part of them.  "host" is dataset.draw_step_size + window_rows + draw_augmentation for the eight
samples (no device).  Reported: median and min .. max over --runs calls after --warmup calls of each side.  Before timing,
the two sides' batches are compared bit for bit.  One process; every step runs under its own time limit (an alarm that ends
the process).  Prints one JSON line (and writes it to --out when given).  Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mpntrackseg_amd import dataset, graph as G, train_batch as TB

PARAMS = {
    "frames_per_graph": 15, "max_detects": 500, "min_detects": 2, "max_frame_dist": "max", "top_k_nns": 150, "reciprocal_k_nns": True,
    "edge_feats_to_use": list(G.EDGE_FEAT_NAMES) + ["emb_dist"], "true_edge_labels": "closest", "augment": True,
    "p_change_fps_step": 0.0, "min_ids_to_drop_perc": 0.0, "max_ids_to_drop_perc": 0.15, "min_detects_to_drop_perc": 0.0,
    "max_detects_to_drop_perc": 0.3, "min_iou_bb_wiggling": 0.8, "target_fps_dict": {"moving": 30, "static": 30},
}


class step:
    """a time limit of its own for one step: the alarm's default action ends the process"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def make_store(seed, frames, dets, reid_dim, device):
    rs = np.random.RandomState(seed)
    counts = rs.randint(max(dets - 5, 1), dets + 6, frames)
    frame = np.repeat(np.arange(1, frames + 1, dtype=np.int64), counts)
    n = frame.size
    ids = np.concatenate([rs.permutation(2 * dets)[:c] for c in counts]).astype(np.int64)
    ids[rs.rand(n) < 0.2] = -1
    w, h = 30.0 + 60.0 * rs.rand(n), 80.0 + 120.0 * rs.rand(n)
    left, top = 1800.0 * rs.rand(n), 100.0 + 700.0 * rs.rand(n)
    det = dict(frame=frame, detection_id=np.arange(n), id=ids, bb_left=left, bb_top=top, bb_width=w, bb_height=h, bb_right=left + w,
               bb_bot=top + h, feet_x=left + 0.5 * w, feet_y=top + h)
    g = torch.Generator().manual_seed(seed)
    return TB.SequenceStore(det, fps=30, step_size=dataset.seq_step_size(30, False, PARAMS["target_fps_dict"]),
                            reid=torch.randn((n, reid_dim), generator=g), x=torch.randn((n, reid_dim, 1, 1), generator=g),
                            x_ext=torch.randn((n, 32, 4, 4), generator=g), mask_labels=(torch.rand((n, 1, 28, 28), generator=g) < 0.5).float(),
                            mask_gt_ixs=(torch.rand(n, generator=g) < 0.6).float(), device=device)


def wiggle_host(boxes, eps):
    """augmentation.py:71-80 in numpy on the gathered rows: (float32 bb_height, bb_width, feet_x, feet_y)"""
    b = boxes.copy()
    top, bot = b[:, 1] + b[:, 5] * eps[:, 0], b[:, 3] + b[:, 5] * eps[:, 1]
    left, right = b[:, 0] + b[:, 4] * eps[:, 2], b[:, 2] + b[:, 4] * eps[:, 3]
    return (bot - top).astype(np.float32), (right - left).astype(np.float32), b[:, 6].astype(np.float32), b[:, 7].astype(np.float32)


def loop_batch(stores, host_boxes, samples, params):
    """the same batch, one graph at a time through the single-graph functions, collated as a PyG Batch"""
    parts, off = [], 0
    for g, (si, rows, eps) in enumerate(samples):
        s = stores[si]
        ids = torch.from_numpy(rows.astype(np.int32)).to(s.device)
        h, w, fx, fy = wiggle_host(host_boxes[si][rows], eps)
        det = dict(frame=s.frame[rows], bb_height=h, bb_width=w, feet_x=fx, feet_y=fy)
        gr = G.construct_graph(det, G.gather_rows(s.reid, ids), s.fps, params["max_frame_dist"], params["edge_feats_to_use"],
                               top_k_nns=params["top_k_nns"], reciprocal_k_nns=params["reciprocal_k_nns"], inference_mode=False)
        labels = G.assign_edge_labels(gr["edge_index"], s.id[rows], params["true_edge_labels"], validate=False)
        gather = lambda t: G.gather_rows(t, ids).view((len(rows),) + tuple(t.shape[1:]))
        e = gr["edge_index"].shape[1]
        parts.append(dict(x=gather(s.x), x_ext=gather(s.x_ext), mask_labels=gather(s.mask_labels), mask_gt_ixs=gather(s.mask_gt_ixs) != 0,
                          edge_index=gr["edge_index"] + off, edge_attr=gr["edge_attr"], edge_labels=labels,
                          edge_graph=torch.full((e,), g, dtype=torch.int32, device=s.device),
                          node_graph=torch.full((len(rows),), g, dtype=torch.int32, device=s.device)))
        off += len(rows)
    return {k: torch.cat([p[k] for p in parts], dim=1 if k == "edge_index" else 0) for k in parts[0]}


def clocked(fn, runs):
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sequences", type=int, default=4)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--dets", type=int, default=25)
    ap.add_argument("--reid-dim", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_train_batches.py needs a GPU")
    dev = torch.device("cuda:0")
    with step(240):
        stores = [make_store(40 + i, a.frames, a.dets, a.reid_dim, dev) for i in range(a.sequences)]
        host_boxes = [s.boxes.cpu().numpy() for s in stores]
        tb = TB.TrainingBatches(stores, PARAMS, batch_size=a.batch_size, mode="train", rng=np.random.RandomState(3), shuffle=True)
        order = tb.rng.permutation(tb.n_samples)[:a.batch_size]
        draw = lambda: [tb.sample(int(i)) for i in order]
        samples = draw()
        batched = lambda: TB.build_batch(tb.set, samples, PARAMS)
        loop = lambda: loop_batch(stores, host_boxes, samples, PARAMS)
        one, other = batched(), loop()
        same = all(bool(torch.equal(one[k], other[k])) for k in other)
        for _ in range(a.warmup):
            batched()
            loop()
            draw()
    with step(900):
        t_b, t_l, t_h = [], [], []
        for _ in range(a.runs):                 # alternating: both sides see the same neighbours on the machine
            t_b += clocked(batched, 1)
            t_l += clocked(loop, 1)
            t0 = time.perf_counter()
            draw()
            t_h.append((time.perf_counter() - t0) * 1e3)
    res = {"sequences": a.sequences, "frames": a.frames, "dets_per_frame": a.dets, "batch_size": a.batch_size, "runs": a.runs,
           "warmup": a.warmup, "nodes": int(one["x"].shape[0]), "edges": int(one["edge_index"].shape[1]), "samples_in_dataset": tb.n_samples,
           "batched_equals_loop": same, "build_batch": summary(t_b), "loop": summary(t_l), "host": summary(t_h),
           "loop_over_build_batch": statistics.median(t_l) / statistics.median(t_b)}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
