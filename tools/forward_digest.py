#!/usr/bin/env python3
"""The forward's counterpart of tools/backward_digest.py: ``mpnhip_forward`` over a fixed table of models and graphs, one case per
branch of the forward's route (csrc/plan.h ``FwdRoute``, csrc/mpn.hip ``ForwardRun``), each as inference (save 0) and as a training
forward (save 1).  Per run it prints the SHA-256 of ``logits``, ``x_out`` and ``e_out``, for a training forward also of every saved
activation ``capi.saved_activation`` returns (the walk of tests/pinned.py::forward_decisions as raw values, plus ``agg``), the two
workspace sizes, ``mpnhip_edge_chain_active`` and the non-zero path counters.  The forward has no atomics: a change of its host
side that is meant to leave the launches alone prints the same lines before and after.

usage: python tools/forward_digest.py [--case NAME ...] [--brief]
(--brief: per run only the line with the digest over all of its tensors' digests and the counters line)"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from backward_digest import dense_graph, empty_graph, params_for, sha  # noqa: E402,F401
from mpntrackseg_amd import capi, synth  # noqa: E402
from mpntrackseg_amd.mpn import MOTMPNet  # noqa: E402


def cases():
    """(name, precision, params, graph, options); options: env (switches of the run), modes (default inference and training)"""
    g = lambda n, e, seed=4, nin=64: synth.make_graph(n, e, T=8, seed=seed, node_in_dim=nin)
    d32 = lambda: params_for(32, 3)
    yield "01 fp32 d32 L3", "fp32", d32(), g(200, 2000), {}
    yield "02 fp32 d32 L3 MPNHIP_NO_CHAIN", "fp32", d32(), g(200, 2000), {"env": ["MPNHIP_NO_CHAIN"]}
    yield "03 fp32 d32 L3 MPNHIP_NO_NODE_FUSION", "fp32", d32(), g(200, 2000), {"env": ["MPNHIP_NO_NODE_FUSION"]}
    yield "04 fp32 d32 L3 MPNHIP_NO_ENCODER_FUSION", "fp32", d32(), g(200, 2000), {"env": ["MPNHIP_NO_ENCODER_FUSION"]}
    yield "05 fp32 d32 L3 N4097", "fp32", d32(), g(4097, 8200), {}
    yield "06 fp32 d32 L4 max no-reattach", "fp32", params_for(32, 4, "max", reattach=(False, False)), g(200, 2000), {}
    yield "07 fp32 deeper odd L2 mean", "fp32", params_for(32, 2, "mean", node_in_dim=20, deep=True), g(50, 300, 6, 20), {}
    yield "08a fp32 d32 L0", "fp32", params_for(32, 0), g(200, 2000), {}
    yield "08b fp32 deeper odd L0", "fp32", params_for(32, 0, "mean", node_in_dim=20, deep=True), g(50, 300, 6, 20), {}
    yield "09 fp32 d128 L4 mean", "fp32", params_for(128, 4, "mean"), g(300, 3000), {}
    yield "10 fp32 d128 L1", "fp32", params_for(128, 1), g(300, 3000), {}
    yield "11 split d128 L6", "fp32_split", params_for(128, 6), g(300, 3000), {}
    yield "12 split d64 L4 no-edge-reattach", "fp32_split", params_for(64, 4, reattach=(True, False)), g(300, 3000), {}
    yield "13 split d128 L4 max", "fp32_split", params_for(128, 4, "max"), g(300, 3000), {"modes": [1]}
    yield "14 bf16 d128 L4", "bf16", params_for(128, 4), g(300, 3000), {}
    for tag, sw in (("15a", "MPNHIP_NO_AGG_FUSION"), ("15b", "MPNHIP_NO_CHAIN_BF16_E16"), ("15c", "MPNHIP_NO_CHAIN_BF16")):
        yield "%s bf16 d128 L4 %s" % (tag, sw), "bf16", params_for(128, 4), g(300, 3000), {"env": [sw]}
    yield "15d bf16 d128 L4 MPNHIP_NO_CHAIN_BF16_TRAIN", "bf16", params_for(128, 4), g(300, 3000), {"env": ["MPNHIP_NO_CHAIN_BF16_TRAIN"], "modes": [1]}
    yield "16 bf16 d128 L4 max", "bf16", params_for(128, 4, "max"), g(300, 3000), {"modes": [1]}
    yield "17a bf16 d128 L4 E0", "bf16", params_for(128, 4), empty_graph(300, 64), {}
    yield "17b fp32 d128 L4 E0", "fp32", params_for(128, 4), empty_graph(300, 64), {}
    yield "18 split d128 L6 prepacked", "fp32_split", params_for(128, 6), g(300, 3000), {"modes": ["prepacked"]}


@contextlib.contextmanager
def switches(names):
    """the library reads its switches on every call"""
    for k in names:
        os.environ[k] = "1"
    try:
        yield
    finally:
        for k in names:
            del os.environ[k]


def build_model(params, precision, seed=7, gain=0.6):
    model = MOTMPNet(params)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(params, seed=seed, gain=gain).items()}, strict=True)
    model = model.to(torch.device("cuda:0"))
    model.gemm_precision = precision
    return model


def saved_digests(model, pg, ws):
    """every activation a training forward left in `ws` (tests/pinned.py::forward_decisions' walk, raw values), plus agg"""
    out = {}

    def take(site, what, step=0, layer=0):
        out[site] = sha(capi.saved_activation(model, pg, ws, what, step, layer))

    n_en = len(model.encoder.node_model.linears())
    n_ee = len(model.encoder.edge_model.linears())
    n_e = len(model.MPNet.edge_model.edge_model.linears())
    n_f = len(model.MPNet.node_model.flow_in_model.linears())
    n_c = len(model.classifier.edge_model.linears())
    for i in range(n_en):
        take("enc_n.%d" % i, "enc_node" if i + 1 < n_en else "x", 0, i)
    for i in range(n_ee):
        take("enc_e.%d" % i, "enc_edge" if i + 1 < n_ee else "e", 0, i)
    for s in range(1, int(model.num_enc_steps) + 1):
        for i in range(n_e):
            take("s%d.edge.%d" % (s, i), "edge_hidden" if i + 1 < n_e else "e", s, i)
        for i in range(n_f):
            take("s%d.flow.%d" % (s, i), "flow_hidden" if i + 1 < n_f else "msg", s, i)
        for i in range(n_c - 1):
            take("s%d.cls.%d" % (s, i), "cls_hidden", s, i)
        take("s%d.node" % s, "x", s)
        take("s%d.agg" % s, "agg", s)
        if model.MPNet.node_model.node_agg_fn.name == "max":
            take("s%d.argmax" % s, "argmax", s)
    return out


def run_forward(model, graph, save):
    """{tensor name: sha256} of one mpnhip_forward call through the C ABI"""
    lib = capi.load()
    dev = torch.device("cuda:0")
    x, ea = (torch.from_numpy(np.ascontiguousarray(graph[k], np.float32)).to(dev) for k in ("x", "edge_attr"))
    ei = torch.from_numpy(graph["edge_index"]).to(dev)
    N, E, L = x.shape[0], ea.shape[0], max(int(model.num_enc_steps), 1)
    pg = capi.PreparedGraph(ei, N, validate=True)
    keep = []
    m = model.c_model(keep, n_edges=E)
    logits = torch.zeros((L, E), dtype=torch.float32, device=dev)
    x_out = torch.zeros((N, m.dn), dtype=torch.float32, device=dev)
    e_out = torch.zeros((E, m.de), dtype=torch.float32, device=dev)
    ws = torch.empty(max(lib.mpnhip_forward_workspace_bytes(m, N, E, save), 256), dtype=torch.uint8, device=dev)
    capi.check(lib.mpnhip_forward(m, capi.ptr(pg.buf), N, E, capi.ptr(x), capi.ptr(ea), capi.ptr(logits), capi.ptr(x_out), capi.ptr(e_out),
                                  capi.ptr(ws), ws.numel(), save, capi.stream_ptr()), "mpnhip_forward")
    torch.cuda.synchronize()
    out = {"logits": sha(logits), "x_out": sha(x_out), "e_out": sha(e_out)}
    if save:
        out.update(saved_digests(model, pg, ws))
    sizes = [int(lib.mpnhip_forward_workspace_bytes(m, N, E, sv)) for sv in (0, 1)]
    return out, sizes, int(lib.mpnhip_edge_chain_active(m))


def run_prepacked(model, graph):
    """two eval calls of the package's own path inside frozen_weights(): the second finds the weight images packed"""
    dev = torch.device("cuda:0")
    x, ea = (torch.from_numpy(np.ascontiguousarray(graph[k], np.float32)).to(dev) for k in ("x", "edge_attr"))
    ei = torch.from_numpy(graph["edge_index"]).to(dev)
    model.eval()
    with torch.no_grad(), model.frozen_weights():
        model.hot_path(x, ei, ea, return_state=True)
        logits, x_out, e_out = model.hot_path(x, ei, ea, return_state=True)
    torch.cuda.synchronize()
    packs = capi.path_counters()["weight_pack"]
    if packs != 1:
        raise SystemExit("prepacked case: weight_pack reads %d over the two calls, not 1" % packs)
    lib = capi.load()
    m = model.c_model([], n_edges=ea.shape[0])
    sizes = [int(lib.mpnhip_forward_workspace_bytes(m, x.shape[0], ea.shape[0], sv)) for sv in (0, 1)]
    return {"logits": sha(logits), "x_out": sha(x_out), "e_out": sha(e_out)}, sizes, int(lib.mpnhip_edge_chain_active(m))


def run_meta_layer():
    """case 19: one mpnhip_meta_layer_forward, inputs as in tests/test_gpu_workspace_exact.py::test_meta_layer at 50 nodes, 300 edges"""
    lib = capi.load()
    dev = torch.device("cuda:0")
    n, E = 50, 300
    params = synth.model_params(32, 1, "mean", node_in_dim=48)
    model = build_model(params, "fp32", seed=15, gain=1.0).eval()
    ei = torch.from_numpy(synth.make_graph(n, E, T=6, seed=40 + n, node_in_dim=48)["edge_index"]).to(dev)
    E = int(ei.shape[1])
    x, e = (torch.from_numpy(a).to(dev) for a in (synth.normal(16, (n, 64)), synth.normal(17, (E, 32))))
    keep = []
    m = model.MPNet.core_struct(keep)
    m.reattach_nodes = m.reattach_edges = 1
    pg = capi.PreparedGraph(ei, n, validate=True)
    x_new = torch.zeros((n, 32), dtype=torch.float32, device=dev)
    e_new = torch.zeros((E, 16), dtype=torch.float32, device=dev)
    nbytes = int(lib.mpnhip_meta_layer_workspace_bytes(m, n, E))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    capi.check(lib.mpnhip_meta_layer_forward(m, capi.ptr(pg.buf), n, E, capi.ptr(x), capi.ptr(e), capi.ptr(x_new), capi.ptr(e_new), capi.ptr(ws),
                                             ws.numel(), capi.stream_ptr()), "mpnhip_meta_layer_forward")
    torch.cuda.synchronize()
    return {"x_new": sha(x_new), "e_new": sha(e_new)}, [nbytes], 0


def report(name, mode, digests, sizes, active, brief=False):
    counters = {k: v for k, v in capi.path_counters().items() if v}
    whole = hashlib.sha256(json.dumps(digests, sort_keys=True).encode()).hexdigest()
    tag = "%s %s" % (name.split()[0], mode)
    print("case %s [%s]: all %s  workspace %s  edge_chain_active %d" % (name, mode, whole, " ".join(map(str, sizes)), active))
    for k in ([] if brief else sorted(digests)):
        print("  %s %s %s" % (tag, k, digests[k]))
    print("  %s counters %s" % (tag, json.dumps(counters, sort_keys=True)))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", action="append", help="run only the cases whose name starts with this (repeatable)")
    ap.add_argument("--brief", action="store_true", help="per run only the digest over all tensors and the counters")
    a = ap.parse_args()
    want = lambda name: not a.case or any(name.startswith(c) for c in a.case)
    for name, precision, params, graph, opts in cases():
        if not want(name):
            continue
        for mode in opts.get("modes", [0, 1]):
            model = build_model(params, precision)
            with switches(opts.get("env", [])):
                capi.path_counters(reset=True)
                if mode == "prepacked":
                    report(name, "eval", *run_prepacked(model, graph), brief=a.brief)
                else:
                    report(name, "save%d" % mode, *run_forward(model.train() if mode else model.eval(), graph, mode), brief=a.brief)
    if want("19 meta layer"):
        capi.path_counters(reset=True)
        report("19 meta layer d32 mean", "op", *run_meta_layer(), brief=a.brief)


if __name__ == "__main__":
    main()
