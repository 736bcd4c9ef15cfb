#!/usr/bin/env python3
"""The workspace sizes behind the weight-gradient products of a given libmpnhip.so, one line per value: the public entries'
(``mpnhip_weight_grad_workspace_bytes``, ``mpnhip_weight_grad_bf16_rows_workspace_bytes``), the routing's test entry
(``mpnhip_debug_weight_grad_batch_workspace_bytes``: batched or not, one or two direction groups, device-side row ranges or not,
fp32 or bf16 source rows) over the shapes of tests/test_gpu_wgrad.py x rows x batches, and ``mpnhip_backward_workspace_bytes`` of
the benchmark configurations in every precision.  Two builds whose row-panel job plan (csrc/wgrad_panel.hip: wp_job_plan) and
slab rules (csrc/common.h, backward_plan.h) are meant to agree print the same text: diff the two outputs.

Pure host code over ctypes: the size queries launch nothing and follow no pointer (every pointer given is the address 256).

usage: python tools/diag/wgrad_sizes.py [--lib PATH] > sizes.txt"""
import argparse
import ctypes as C
import itertools
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from mpntrackseg_amd import capi, synth  # noqa: E402

ROWS = [3, 16, 17, 44, 300, 1000, 4097, 77800, 400000]
NBATCH = [1, 3, 12]
# the two kNN-built configurations have no fixed edge count: stand-ins of their order of magnitude
KNN_EDGES = {"C": 77800, "D": 9000}


def shapes():
    """SHAPES and SHAPES16 of tests/test_gpu_wgrad.py, read from its source (importing it would need pytest and a device)."""
    ns = {}
    src = open(os.path.join(ROOT, "tests", "test_gpu_wgrad.py")).read()
    for name in ("SHAPES", "SHAPES16"):
        start = src.index("\n%s = [" % name) + 1
        exec(src[start:src.index("]\n", start) + 1], ns)
    return ns["SHAPES"], ns["SHAPES16"]


def load(path):
    lib = C.CDLL(path)
    for name, (res, args) in capi.SIGNATURES.items():
        if name.endswith("_workspace_bytes"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def product(n_out, k_in, rows, nb, groups, ranged, src16):
    p = capi.WgradProduct()
    p.dZ, p.ldz, p.z_bstride = 256, n_out, rows * n_out
    p.H, p.ldh, p.h_bstride = 256, k_in, rows * k_in
    p.ldw, p.rows, p.n_out, p.k_in, p.nbatch, p.src16 = k_in, rows, n_out, k_in, nb, src16
    for q in range(groups):
        p.g[q].grad_w = 256
        if ranged:
            p.g[q].row_begin = p.g[q].row_end = 256
    return p


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=capi.lib_path(), help="the libmpnhip.so to ask (default: the package's)")
    lib = load(ap.parse_args().lib)
    shapes32, shapes16 = shapes()
    for (n_out, k_in), rows, nb in itertools.product(shapes32, ROWS, NBATCH):
        print("weight_grad %d %d %d %d = %d" % (n_out, k_in, rows, nb, lib.mpnhip_weight_grad_workspace_bytes(n_out, k_in, rows, nb)))
    for (n_out, k_in), rows, nb in itertools.product(shapes16, ROWS, NBATCH):
        print("weight_grad_bf16_rows %d %d %d %d = %d" % (n_out, k_in, rows, nb, lib.mpnhip_weight_grad_bf16_rows_workspace_bytes(n_out, k_in, rows, nb)))
    for src16, shp in ((0, shapes32), (1, shapes16)):
        prec = capi.PRECISIONS["bf16" if src16 else "fp32_split"]
        for (n_out, k_in), rows, nb, batched, groups, ranged in itertools.product(shp, ROWS, NBATCH, (0, 1), (1, 2), (0, 1)):
            arr = (capi.WgradProduct * 1)(product(n_out, k_in, rows, nb, groups, ranged, src16))
            print("debug_batch src16=%d %d %d %d %d batched=%d groups=%d ranged=%d = %d" % (
                src16, n_out, k_in, rows, nb, batched, groups, ranged, lib.mpnhip_debug_weight_grad_batch_workspace_bytes(arr, 1, prec, batched, 0)))
    for name, cfg in sorted(synth.CONFIGS.items()):
        e = cfg["E"] if cfg["E"] is not None else KNN_EDGES[name]
        for prec in sorted(capi.PRECISIONS):
            m = capi.dims_model(synth.model_params(cfg["d"], cfg["L"]), prec)
            print("backward cfg-%s N=%d E=%d %s = %d" % (name, cfg["N"], e, prec, lib.mpnhip_backward_workspace_bytes(m, cfg["N"], e)))


if __name__ == "__main__":
    main()
