#!/usr/bin/env python3
"""One training forward + ``mpnhip_backward_flags`` per case over a fixed table of models and graphs (``mpntrackseg_amd.synth``, fixed
seeds), and per case the SHA-256 of every parameter gradient, of ``grad_x`` and of ``grad_edge_attr``, the backward's workspace size
and the path counters.  The cases reach every branch of the backward's orchestration (csrc/backward.hip, BackwardRun): a change there
that is meant to leave the arithmetic alone prints the same lines before and after -- the backward is bitwise reproducible
(tests/test_gpu_backward.py::test_backward_is_bitwise_reproducible).

usage: python tools/backward_digest.py [--case NAME ...] [--repeat K]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from mpntrackseg_amd import capi, synth  # noqa: E402
from mpntrackseg_amd.autograd import native_forward_saved  # noqa: E402
from mpntrackseg_amd.mpn import MOTMPNet  # noqa: E402


def dense_graph(N, E, seed, node_in_dim):
    """More edges than distinct node pairs (E >= 48 N at 20 nodes): pairs drawn WITH repetition, mirrored like synth.make_graph's."""
    half = E // 2
    a = (synth.uniform01(seed, half, stream=1) * N).astype(np.int64)
    b = (a + 1 + (synth.uniform01(seed, half, stream=2) * (N - 1)).astype(np.int64)) % N   # b != a
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    ea = synth.normal(seed, (half, 6), stream=3)
    return {"x": synth.normal(seed, (N, node_in_dim), stream=4), "edge_index": np.stack([np.concatenate([lo, hi]), np.concatenate([hi, lo])]),
            "edge_attr": np.concatenate([ea, ea], axis=0)}


def empty_graph(N, node_in_dim):
    return {"x": synth.normal(3, (N, node_in_dim)), "edge_index": np.zeros((2, 0), np.int64), "edge_attr": np.zeros((0, 6), np.float32)}


def params_for(d, L, agg="sum", node_in_dim=64, reattach=(True, True), deep=False):
    p = synth.model_params(d, L, agg, node_in_dim=node_in_dim)
    p["reattach_initial_nodes"], p["reattach_initial_edges"] = reattach
    if deep:   # tests/test_gpu_backward.py::test_deeper_mlps_and_odd_dims
        p["encoder_feats_dict"]["edge_dims"] = [10]
        p["encoder_feats_dict"]["node_dims"] = [24, 12]
        p["edge_model_feats_dict"]["dims"] = [40, 24, 16]
        p["node_model_feats_dict"]["dims"] = [32]
        p["classifier_feats_dict"]["edge_dims"] = [6, 5]
    return p


def cases():
    """(name, precision, params, graph, options)"""
    g = lambda n, e, seed=4, nin=64: synth.make_graph(n, e, T=8, seed=seed, node_in_dim=nin)
    yield "01 fp32 d32 L3", "fp32", params_for(32, 3), g(200, 2000), {}
    # (the reference's widths run on the fused edge chain too: its one-launch-per-product form only with the chain switched off)
    yield "01b fp32 d32 L3 MPNHIP_NO_CHAIN", "fp32", params_for(32, 3), g(200, 2000), {"env": {"MPNHIP_NO_CHAIN": "1"}}
    yield "02 fp32 d32 L6", "fp32", params_for(32, 6), g(200, 2000), {}
    yield "03 fp32 d32 L4 max no-reattach", "fp32", params_for(32, 4, "max", reattach=(False, False)), g(200, 2000), {}
    yield "03b fp32 deeper odd L2 max no-reattach", "fp32", params_for(32, 2, "max", node_in_dim=20, reattach=(False, False), deep=True), g(50, 300, 6, 20), {}
    yield "04 fp32 d32 L0", "fp32", params_for(32, 0), g(200, 2000), {}
    yield "05 fp32 deeper odd L2 dense", "fp32", params_for(32, 2, "mean", node_in_dim=20, deep=True), dense_graph(20, 1200, 6, 20), {}
    yield "05b fp32 d128 L2 dense", "fp32", params_for(128, 2), dense_graph(20, 1200, 6, 64), {}
    yield "06 fp32 d128 L4 mean", "fp32", params_for(128, 4, "mean"), g(300, 3000), {}
    yield "07 fp32 d128 L6 big", "fp32", params_for(128, 6), g(2000, 20000), {}
    yield "08 split d128 L6", "fp32_split", params_for(128, 6), g(300, 3000), {}
    yield "09 split d64 L4 no-edge-reattach", "fp32_split", params_for(64, 4, reattach=(True, False)), g(300, 3000), {}
    yield "10a split d128 L6 defer big", "fp32_split", params_for(128, 6), g(2000, 20000), {"defer": True}
    yield "10b split d128 L6 defer", "fp32_split", params_for(128, 6), g(300, 3000), {"defer": True}
    yield "11 bf16 d128 L4", "bf16", params_for(128, 4), g(300, 3000), {}
    yield "12a bf16 d128 L4 E0", "bf16", params_for(128, 4), empty_graph(300, 64), {}
    yield "12b fp32 d128 L4 E0", "fp32", params_for(128, 4), empty_graph(300, 64), {}
    yield "13 fp32 d32 L3 seeded", "fp32", params_for(32, 3), g(200, 2000), {"seeded": True}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(precision, params, graph, defer=False, seeded=False):
    """{tensor name: sha256}, backward workspace bytes"""
    lib = capi.load()
    dev = torch.device("cuda:0")
    model = MOTMPNet(params)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(params, seed=7, gain=0.6).items()}, strict=True)
    model = model.to(dev).train()
    model.gemm_precision = precision
    x, ea = (torch.from_numpy(np.ascontiguousarray(graph[k], np.float32)).to(dev) for k in ("x", "edge_attr"))
    ei = torch.from_numpy(graph["edge_index"]).to(dev)
    N, E, L = x.shape[0], ea.shape[0], max(int(params["num_enc_steps"]), 1)
    pg = capi.PreparedGraph(ei, N, validate=True)
    logits = torch.empty((L, E), dtype=torch.float32, device=dev)
    fwd_ws = native_forward_saved(model, pg, x, ea, logits)
    prm = model.hot_path_parameters()
    grads = {id(p): torch.zeros_like(p) for p in prm}
    keep = []
    m = model.c_model(keep, grads=grads, n_edges=E)
    glog = torch.from_numpy(synth.normal(3, (L, E))).to(dev)
    # (seeded: the caller's gradients of the final node / edge features, widths dn / de)
    dn, de = params["encoder_feats_dict"]["node_out_dim"], params["encoder_feats_dict"]["edge_out_dim"]
    gxo = torch.from_numpy(synth.normal(5, (N, dn))).to(dev) if seeded else None
    geo = torch.from_numpy(synth.normal(6, (E, de))).to(dev) if seeded else None
    gx, gea = torch.empty_like(x), torch.empty_like(ea)
    nbytes = lib.mpnhip_backward_workspace_bytes(m, N, E)
    bws = capi.workspace(nbytes, dev, "bwd")
    capi.check(lib.mpnhip_backward_flags(m, capi.ptr(pg.buf), N, E, capi.ptr(x), capi.ptr(ea), capi.ptr(glog), capi.ptr(gxo), capi.ptr(geo),
                                         capi.ptr(gx), capi.ptr(gea), capi.ptr(fwd_ws), fwd_ws.numel(), capi.ptr(bws), bws.numel(),
                                         1 if defer else 0, capi.stream_ptr()), "mpnhip_backward_flags")
    if defer:
        capi.check(lib.mpnhip_side_stream_join(capi.stream_ptr()), "mpnhip_side_stream_join")
    torch.cuda.synchronize()
    out = {"logits": sha(logits), "grad_x": sha(gx), "grad_edge_attr": sha(gea)}
    for k, p in model.named_parameters():
        if id(p) in grads:
            out[k] = sha(grads[id(p)])
    return out, nbytes


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", action="append", help="run only the cases whose name starts with this (repeatable)")
    ap.add_argument("--repeat", type=int, default=1, help="run every case this many times (each run prints its lines)")
    a = ap.parse_args()
    for name, precision, params, graph, opts in cases():
        if a.case and not any(name.startswith(c) for c in a.case):
            continue
        opts = dict(opts)
        env = opts.pop("env", {})   # (the library reads its switches on every call)
        for _ in range(a.repeat):
            capi.path_counters(reset=True)
            os.environ.update(env)
            try:
                digests, nbytes = run_case(precision, params, graph, **opts)
            finally:
                for k in env:
                    del os.environ[k]
            counters = {k: v for k, v in capi.path_counters().items() if v}
            whole = hashlib.sha256(json.dumps(digests, sort_keys=True).encode()).hexdigest()
            print("case %s: all %s  bwd_workspace %d" % (name, whole, nbytes))
            for k in sorted(digests):
                print("  %s %s %s" % (name.split()[0], k, digests[k]))
            print("  %s counters %s" % (name.split()[0], json.dumps(counters, sort_keys=True)))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
