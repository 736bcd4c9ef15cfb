"""Operator-level parity of the fused node-side chain kernels (csrc/node_chain.hip: node_chain_kernel, node_chain_bwd_kernel) against
the float64 restatement of their documented formulas (tests/chain_ref.py, pinned to the oracle by tests/test_chain_ref_cpu.py), ONE
launch each through the C ABI (mpnhip_debug_node_chain, mpnhip_debug_node_chain_backward: the forward's and the backward's own
packers and launchers).

Guards.  Every output lives between GUARD rows and is prefilled with NaN together with them; afterwards the guards must still be
NaN bit for bit and every row the formula writes must be finite.  Every input carries a NaN row behind its last row, so a read past
the end poisons the result.  Every case asserts, through mpnhip_debug_counters, that the kernel it means to test ran exactly once and
that no other counted kernel ran.

Error measure: max |got - ref64| / max(max |ref64|, 1e-30) per output tensor, over all elements.  Bound: max(2e-6, 4 x the error of
the float32 CPU evaluation of chain_ref on the same case) -- the rule of tests/test_gpu_gemm.py (the kernels multiply three-piece
bf16 operands, an fp32-class product; 4 x covers another summation order of the same formula).

Decisions.  x_new > 0 must equal the reference's z > 0 except where the float64 pre-activation is within MARGIN = 2e-5 x the layer's
rms of zero (tests/test_gpu_pinned.py), and at most one such unit per case; the seeds are chosen so that the float32 CPU evaluation
alone stays within that cap (asserted here, on the CPU side of each case).  The backward takes its decisions as an input (x_prev),
which holds exact zeros, negative values and a NaN guard row.

Shapes: the smallest at which the tiling can go wrong -- a block owns 32 nodes: N = 1, 32, 33 and 70 (one node, one full block, a
block and one node, two blocks and a ragged third); both templates (dn = 64, 128) at the model's projection width (pw = 8.5 dn);
segments of 0, 1, 2, 3, 4, 5, 7 and ~40 rows against the 4 / 2 / 1-row unrolling of the aggregation; two self loops (in neither
aggregate); all three aggregations; P_next and agg_out each given and null.  Every case prints "CHAIN_ERR <case> <tensor> kernel
<err> float32-cpu <err>" (DESIGN.md keeps the table of an MI355X run)."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_ref as CR
import segment_ref as SR
from chain_ops_common import FLOOR_TOL, Guarded, decision_exceptions, dev, only_counter, report, with_nan_row
from mpntrackseg_amd import capi, synth

pytestmark = pytest.mark.gpu
def node_graph(N, seed):
    """edge_index [2, E] over N nodes: node k < 8 gets flow-in and flow-out segments of (0, 1, 2, 3, 4, 5, 7, 40)[k] rows where N
    allows, the other nodes a few random edges, every fifth node none at all as a row; two self loops; shuffled."""
    if N == 1:
        return np.array([[0, 0], [0, 0]], np.int64)
    lens = (0, 1, 2, 3, 4, 5, 7, 40)
    u = synth.uniform01(seed, 16 * N + 1024, stream=0)
    rows, cols, k = [], [], 0
    for n in range(N):
        want = lens[n] if n < len(lens) else (0 if n % 5 == 0 else 1 + int(u[k] * 4))
        k += 1
        for _ in range(want):
            for lo, hi in ((0, n), (n + 1, N)):       # one past neighbour (flow_in), one future neighbour (flow_out)
                if hi > lo:
                    rows.append(n)
                    cols.append(lo + int(u[k] * (hi - lo)))
                k += 1
    rows += [N // 2, N - 1]
    cols += [N // 2, N - 1]
    ei = np.array([rows, cols], np.int64)
    return ei[:, np.argsort(synth.uniform01(seed, ei.shape[1], stream=1), kind="stable")]


@pytest.mark.parametrize("agg", ["sum", "mean", "max"])
@pytest.mark.parametrize("dn,N", [(64, 1), (64, 32), (64, 33), (64, 70), (128, 1), (128, 33), (128, 70)])
def test_node_chain_forward(dn, N, agg):
    run_node_chain_forward(dn, N, agg, "all")


@pytest.mark.parametrize("outputs", ["no_P_next", "no_agg_out", "neither"])
@pytest.mark.parametrize("dn,N,agg", [(64, 33, "sum"), (64, 1, "max"), (128, 70, "mean")])
def test_node_chain_forward_null_outputs(dn, N, agg, outputs):
    """The last step has no P_next, inference no agg_out: what is still written must be bitwise what the full call writes."""
    full = run_node_chain_forward(dn, N, agg, "all")
    part = run_node_chain_forward(dn, N, agg, outputs)
    for k, v in part.items():
        assert np.array_equal(v, full[k]), (k, outputs)


def run_node_chain_forward(dn, N, agg, outputs):
    case = "node_fwd dn%d N%d %s %s" % (dn, N, agg, outputs)
    pw, seed = 17 * dn // 2, 1000 + dn + N
    ei = node_graph(N, seed)
    E = ei.shape[1]
    csr = SR.graph_csr(ei, N)
    M = synth.normal(seed, (E, dn), stream=2)      # the messages, in SORTED edge order (as they cross the ABI)
    Wu = synth.normal(seed, (dn, 2 * dn), stream=3, std=(2 * dn) ** -0.5)
    bu = synth.normal(seed, (dn,), stream=4, std=0.1)
    Wnode = synth.normal(seed, (pw, 2 * dn), stream=5, std=(2 * dn) ** -0.5)
    P0 = synth.normal(seed, (N, pw), stream=6)
    want_P, want_agg = outputs not in ("no_P_next", "neither"), outputs not in ("no_agg_out", "neither")

    ref = CR.node_chain_forward(M, csr["seg_ptr"], N, agg, Wu, bu, Wnode, P0 if want_P else None, torch.float64)
    f32 = CR.node_chain_forward(M, csr["seg_ptr"], N, agg, Wu, bu, Wnode, P0 if want_P else None, torch.float32)
    assert decision_exceptions(ref["z"], f32["z"].numpy() > 0) <= 1, (case, "choose another seed: the float32 evaluation itself is on the edge")

    lib = capi.load()
    pg = capi.PreparedGraph(torch.from_numpy(ei).to(dev()), N, validate=True, full=True)
    perm = pg.buf.cpu().numpy()[256:256 + 4 * E].view(np.int32).astype(np.int64)
    assert np.array_equal(perm, csr["perm"])
    # the rows of self loops (behind both direction groups in the sorted order) are NaN: no segment holds them
    Ms = M.copy()
    Ms[int(csr["seg_ptr"][2 * N]):] = np.nan
    assert np.isnan(Ms).any()
    M_d = with_nan_row(Ms)
    Wu_d, bu_d, Wn_d = (torch.from_numpy(a).to(dev()) for a in (Wu, bu, Wnode))
    P0_d = with_nan_row(P0) if want_P else None
    x_new, P_next, agg_out = Guarded(N, dn), Guarded(N, pw) if want_P else None, Guarded(N, 2 * dn) if want_agg else None
    need = lib.mpnhip_debug_node_chain_workspace_bytes(dn, pw)
    assert need > 0
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=dev())
    capi.path_counters(reset=True)
    capi.check(lib.mpnhip_debug_node_chain(capi.ptr(pg.buf), N, E, capi.ptr(M_d), dn, pw, capi.AGG_CODE[agg], capi.ptr(Wu_d), capi.ptr(bu_d),
                                           capi.ptr(Wn_d), capi.ptr(P0_d), x_new.ptr(), P_next.ptr() if want_P else None,
                                           agg_out.ptr() if want_agg else None, capi.ptr(ws), need, capi.stream_ptr()), "debug_node_chain")
    torch.cuda.synchronize()
    only_counter("node_chain")
    assert (ws[need:] == 0xFF).all(), "the workspace was written past its stated size"

    got = {"x_new": x_new.result(case)}
    if want_P:
        got["P_next"] = P_next.result(case)
    if want_agg:
        got["agg"] = agg_out.result(case)
    report(case, {k: (CR.rel_err(v, ref[k]), CR.rel_err(f32[k], ref[k])) for k, v in got.items()})
    assert decision_exceptions(ref["z"], got["x_new"] > 0) <= 1, case
    if want_agg:
        # empty segments are exactly 0; max returns one of its inputs bit for bit
        empty = np.repeat(np.diff(csr["seg_ptr"][:2 * N + 1]).reshape(2, N)[::-1].T == 0, dn, axis=1)
        assert not got["agg"][empty].any(), case
        if agg == "max":
            assert np.array_equal(got["agg"], f32["agg"].numpy()), case
    return got


@pytest.mark.parametrize("dn,N", [(64, 1), (64, 33), (64, 70), (128, 1), (128, 33), (128, 70)])
def test_node_chain_backward(dn, N):
    case = "node_bwd dn%d N%d" % (dn, N)
    pw, seed = 17 * dn // 2, 2000 + dn + N
    dP = synth.normal(seed, (N, pw), stream=0)
    x_prev = np.maximum(synth.normal(seed, (N, dn), stream=1), 0)     # a ReLU output: half the entries exact zeros
    x_prev[::3, ::5] = -1.0                                           # ... and some negative ones (never positive: gradient 0)
    Wu = synth.normal(seed, (dn, 2 * dn), stream=3, std=(2 * dn) ** -0.5)
    Wnode = synth.normal(seed, (pw, 2 * dn), stream=5, std=(2 * dn) ** -0.5)
    ref = CR.node_chain_backward(dP, x_prev > 0, Wnode, Wu, torch.float64)
    f32 = CR.node_chain_backward(dP, x_prev > 0, Wnode, Wu, torch.float32)

    lib = capi.load()
    dP_d, xp_d = with_nan_row(dP), with_nan_row(x_prev)
    Wu_d, Wn_d = torch.from_numpy(Wu).to(dev()), torch.from_numpy(Wnode).to(dev())
    dZn, dAGG = Guarded(N, dn), Guarded(N, 2 * dn)
    need = lib.mpnhip_debug_node_chain_backward_workspace_bytes(dn, pw)
    assert need > 0
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=dev())
    capi.path_counters(reset=True)
    capi.check(lib.mpnhip_debug_node_chain_backward(N, capi.ptr(dP_d), dn, pw, capi.ptr(xp_d), capi.ptr(Wn_d), capi.ptr(Wu_d), dZn.ptr(),
                                                    dAGG.ptr(), capi.ptr(ws), need, capi.stream_ptr()), "debug_node_chain_backward")
    torch.cuda.synchronize()
    only_counter("node_chain_bwd")
    assert (ws[need:] == 0xFF).all(), "the workspace was written past its stated size"
    got = {"dZn": dZn.result(case), "dAGG": dAGG.result(case)}
    report(case, {k: (CR.rel_err(v, ref[k]), CR.rel_err(f32[k], ref[k])) for k, v in got.items()})
    # the masked units are exact zeros (either sign: every other node's gradient is kept negated inside the kernel)
    assert not got["dZn"][~(x_prev > 0)].any(), case


def test_node_chain_refuses_other_widths_before_any_launch():
    lib = capi.load()
    t = torch.zeros(4096, dtype=torch.float32, device=dev())
    p = capi.ptr(t)
    capi.path_counters(reset=True)
    for dn, pw in ((32, 272), (96, 816), (64, 540), (256, 2176)):
        assert lib.mpnhip_debug_node_chain_workspace_bytes(dn, pw) == 0
        assert lib.mpnhip_debug_node_chain(p, 4, 0, p, dn, pw, 0, p, p, p, p, p, p, p, p, 1 << 30, capi.stream_ptr()) == -4
        assert lib.mpnhip_debug_node_chain_backward(4, p, dn, pw, p, p, p, p, p, p, 1 << 30, capi.stream_ptr()) == -4
    torch.cuda.synchronize()
    assert not any(capi.path_counters(reset=True).values())
    assert not t.cpu().numpy().any()
