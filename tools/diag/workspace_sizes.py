#!/usr/bin/env python3
"""Every ``mpnhip_*_workspace_bytes`` function and ``mpnhip_graph_bytes`` of a given libmpnhip.so over a fixed grid of shapes:
one line per family with the number of points and a SHA-256 of the values.  Two builds whose workspace layouts are meant to be
the same (a refactor of the plans in csrc/plan.h, backward_plan.h, ...) print the same lines; ``--dump`` prints the values.

Pure host code over ctypes -- the size functions launch nothing, and the model descriptions hold dims only.  The rocprim scratch
terms of the sort / scan based operators are queried from the runtime: they show with a device present only, so compare two
libraries on the same machine.

usage: python tools/diag/workspace_sizes.py [--lib PATH] [--dump]"""
import argparse
import ctypes as C
import hashlib
import itertools
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from mpntrackseg_amd import capi, synth  # noqa: E402

WIDTHS = [20, 32, 64, 128, 256]
STEPS = [0, 1, 2, 4, 12]
REATTACH = [(True, True), (False, False), (True, False)]   # (nodes, edges)
GRAPHS = [(0, 0), (1, 0), (7, 13), (64, 300), (65, 301), (5000, 50000), (20000, 400000)]


def core_models():
    """(label, capi.Model): widths x steps x precisions x {sum, max} x reattach x {shipped two-layer modules, deeper variant}.
    Width 32 of the shipped form is the reference's own (he 80, hn 56, hc 8, node encoder 2048 -> 128 -> 32)."""
    for d, L, prec, agg, (rn, re_), deep in itertools.product(WIDTHS, STEPS, sorted(capi.PRECISIONS), ["sum", "max"], REATTACH, [False, True]):
        p = synth.model_params(d, L, agg)
        p["reattach_initial_nodes"], p["reattach_initial_edges"] = rn, re_
        if deep:
            synth.deeper_params(p)
        yield "d%d L%d %s %s reattach%d%d %s" % (d, L, prec, agg, rn, re_, "deeper" if deep else "shipped"), capi.dims_model(p, prec)


def load(path):
    lib = C.CDLL(path)
    for name, (res, args) in capi.SIGNATURES.items():
        if name.endswith("_workspace_bytes") or name == "mpnhip_graph_bytes":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def families(lib):
    """{family: [(label, bytes)]}"""
    out = {k: [] for k in ("forward save=0", "forward save=1", "backward", "meta_layer")}
    for label, m in core_models():
        for n, e in GRAPHS:
            at = "%s N%d E%d" % (label, n, e)
            out["forward save=0"].append((at, lib.mpnhip_forward_workspace_bytes(m, n, e, 0)))
            out["forward save=1"].append((at, lib.mpnhip_forward_workspace_bytes(m, n, e, 1)))
            out["backward"].append((at, lib.mpnhip_backward_workspace_bytes(m, n, e)))
            out["meta_layer"].append((at, lib.mpnhip_meta_layer_workspace_bytes(m, n, e)))
    rows = [0, 1, 7, 64, 65, 300, 301, 5000, 50000, 400000]

    def grid(name, fn, *axes):
        out[name] = [(" ".join(map(str, a)), fn(*a)) for a in itertools.product(*axes)]

    grid("graph_bytes", lib.mpnhip_graph_bytes, [n for n, _ in GRAPHS], [e for _, e in GRAPHS])
    grid("graph_prep", lib.mpnhip_graph_prep_workspace_bytes, [n for n, _ in GRAPHS], [e for _, e in GRAPHS])
    widths = [1, 5, 20, 48, 64, 80, 256, 640]
    grid("weight_grad", lib.mpnhip_weight_grad_workspace_bytes, widths, widths, rows, [1, 2, 12])
    grid("weight_grad_bf16_rows", lib.mpnhip_weight_grad_bf16_rows_workspace_bytes, widths, widths, rows, [1, 2, 12])
    grid("bn_dropout", lib.mpnhip_bn_dropout_workspace_bytes, rows, [1, 20, 64, 65, 640])
    out["mlp"] = []
    for dims in ([1], [20, 1], [18, 18, 16], [128, 32], [40, 24, 16, 7]):
        mlp = capi.fill_mlp_dims(capi.Mlp(), 6, dims)
        out["mlp"] += [("%s m%d" % (dims, r), lib.mpnhip_mlp_workspace_bytes(mlp, r)) for r in rows]
    grid("segment_reduce", lib.mpnhip_segment_reduce_workspace_bytes, rows, [0, 1, 64, 65, 5000])
    grid("tracking_loss", lib.mpnhip_tracking_loss_workspace_bytes, [1, 3, 12], rows)
    grid("tracking_loss_graphs", lib.mpnhip_tracking_loss_graphs_workspace_bytes, [1, 3, 12], rows, [1, 2, 8])
    grid("edge_labels", lib.mpnhip_edge_labels_workspace_bytes, rows)
    grid("mask_loss", lib.mpnhip_mask_loss_workspace_bytes, [1, 3], [0, 9, 300], [171, 320, 784], [1, 2])
    grid("time_valid_conn", lib.mpnhip_time_valid_conn_workspace_bytes, rows)
    grid("knn_mask", lib.mpnhip_knn_mask_workspace_bytes, rows, [0, 1])
    grid("compact", lib.mpnhip_compact_workspace_bytes, rows)
    grid("undirected_merge", lib.mpnhip_undirected_merge_workspace_bytes, rows)
    grid("project_round_count", lib.mpnhip_project_round_count_workspace_bytes, rows)
    grid("project_greedy", lib.mpnhip_project_greedy_workspace_bytes, rows)
    grid("connected_components", lib.mpnhip_connected_components_workspace_bytes, rows)
    grid("full_masks", lib.mpnhip_full_masks_workspace_bytes, [0, 5, 300], [1, 2, 15], [37 * 53, 375 * 1242], [0, 1000])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=capi.lib_path(), help="the libmpnhip.so to ask (default: the package's)")
    ap.add_argument("--dump", action="store_true", help="print every value, not only the per-family digests")
    a = ap.parse_args()
    total = 0
    for name, values in families(load(a.lib)).items():
        total += len(values)
        digest = hashlib.sha256(" ".join(str(v) for _, v in values).encode()).hexdigest()
        print("%-24s %7d points  sha256 %s" % (name, len(values), digest))
        if a.dump:
            for label, v in values:
                print("  %s: %s = %d" % (name, label, v))
    print("%-24s %7d points" % ("total", total))


if __name__ == "__main__":
    main()
