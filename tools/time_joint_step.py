#!/usr/bin/env python3
"""Time of one JOINT optimizer step (tracking + segmentation loss) on one KITTI-MOTS-like batch, two routes in one process:

  joint     TrainStep(train_mask_branch=True): native forward / backward, mask branch under autograd on the native logits,
            native loss kernels, one flat bucket, one Adam launch;
  existing  model(data) + loss.compute_loss + .backward() + torch.optim.Adam (foreach) on an identically loaded twin model.

The batch: --graphs (default 2) graphs of synth.make_knn_graph(frames=20, dets=7, top_k=100) (SURVEY.md section 8d cfg-D: 140 nodes
each), block-diagonal, reference dims (32-d, synth.MASK_PARAMS), L = 4 with 2 classified steps, x_ext [N, 256, 14, 14], masks
[N, 1, 56, 56], 60 % of the rows with a ground-truth mask.  Both routes run every convolution / LayerNorm of the mask branch
forward and backward as stock modules; they differ in everything else of the step.

Each step is timed with a host clock around the call and a device synchronise (the step includes its host work: both routes
are host-heavy at this size), alternating between the routes after --warmup steps each; reported are the median and min .. max of
--runs steps.  first_call_ms is the first step of each route in this process; the route that runs first (joint) also pays the
library's algorithm search for the convolutions both routes share.  Writes profiles/joint_step/timing.json (or --out).  Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mpntrackseg_amd import loss as mloss
from mpntrackseg_amd import synth
from mpntrackseg_amd.mpn import MOTMPNet
from mpntrackseg_amd.train import TrainStep

L = 4


def problem(dev, n_graphs):
    params = synth.model_params(32, L, "sum", num_class_steps=2, node_in_dim=64)
    params.update(synth.MASK_PARAMS)
    W = synth.make_weights(params, seed=7, gain=0.6)
    W.update(synth.make_mask_weights(seed=17))

    def fresh():
        m = MOTMPNet(params)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
        return m.to(dev).train()
    graphs = [synth.make_knn_graph(frames=20, dets=7, top_k=100, seed=1 + i, node_in_dim=64) for i in range(n_graphs)]
    b = synth.batch_graphs(graphs)
    n, e = b["x"].shape[0], b["edge_index"].shape[1]
    t = lambda a: torch.from_numpy(a).to(dev)
    batch = dict(x=t(b["x"]), edge_index=t(b["edge_index"]), edge_attr=t(b["edge_attr"]), edge_graph=t(b["edge_graph"]),
                 node_graph=t(b["batch"].astype(np.int32)), n_graphs=n_graphs,
                 edge_labels=t((synth.uniform01(8, e) < 0.15).astype(np.float32)),
                 x_ext=t(synth.normal(9, (n, 256, 14, 14), stream=1, std=0.5)),
                 mask_labels=t((synth.uniform01(6, n * 56 * 56) < 0.5).astype(np.float32).reshape(n, 1, 56, 56)),
                 mask_gt_ixs=t(synth.uniform01(7, n) < 0.6))
    return fresh, batch


class _Obj:
    pass


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=2)
    ap.add_argument("--mask-conv-grads", choices=("stock", "native", "native_all"), default="stock",
                    help="MOTMPNet.mask_conv_grads of BOTH routes: the backward of the mask branch's Conv2d layers (native_all: of its "
                         "transposed convolutions and LayerNorm too)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "joint_step",
                                                  "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_joint_step.py needs a GPU")
    dev = torch.device("cuda:0")
    fresh, b = problem(dev, a.graphs)
    lw = {"tracking": 1, "segmentation": 1}
    step = TrainStep(fresh(), lr=1e-3, train_mask_branch=True, loss_weights=lw)
    twin = fresh()
    step.model.mask_conv_grads = twin.mask_conv_grads = a.mask_conv_grads
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    data = _Obj()
    data.x, data.x_ext, data.edge_index, data.edge_attr = b["x"], b["x_ext"], b["edge_index"], b["edge_attr"]
    tgt = _Obj()
    tgt.edge_labels, tgt.mask_labels, tgt.mask_gt_ixs = b["edge_labels"], b["mask_labels"], b["mask_gt_ixs"]
    last = {}

    def joint():
        step.batch(b, holder=data)
        last["joint"] = step.last_losses["tracking"][0] + step.last_losses["segmentation"][0]

    def existing():
        opt.zero_grad(set_to_none=True)
        out = twin(data)
        loss = mloss.compute_loss(out, tgt, lw, edge_graph=b["edge_graph"], node_graph=b["node_graph"], n_graphs=b["n_graphs"])
        loss.backward()
        opt.step()
        last["existing"] = loss.detach()
    routes = {"joint": joint, "existing": existing}
    first = {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        first[name] = (time.perf_counter() - t0) * 1e3
        for _ in range(max(a.warmup - 1, 0)):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    losses = {k: [] for k in routes}
    for _ in range(max(a.runs, 20)):
        for name, fn in routes.items():       # alternating: both routes see the same neighbours on the machine
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            losses[name].append(float(last[name]))
    res = {"problem": {"graphs": a.graphs, "nodes": int(b["x"].shape[0]), "edges": int(b["edge_index"].shape[1]), "L": L,
                       "x_ext": list(b["x_ext"].shape), "flat_bucket_floats": int(step.bucket.n), "mask_floats": int(step.mask_elems)},
           "mask_conv_grads": a.mask_conv_grads, "runs": len(times["joint"]), "warmup": a.warmup, "timing": "host clock around the step + device synchronise, ms"}
    for name, ts in times.items():
        res[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "first_call_ms": first[name],
                     "loss_first": losses[name][0], "loss_last": losses[name][-1]}
    res["joint_over_existing_median"] = res["joint"]["median_ms"] / res["existing"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
