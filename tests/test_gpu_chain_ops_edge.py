"""Operator-level parity of the fused per-edge chain kernels in the fp32 and the three-piece split form (csrc/edge_chain.hip:
edge_chain_kernel, edge_chain_bwd_kernel) against the float64 restatement of their documented formulas (tests/chain_ref.py, pinned to
the oracle by tests/test_chain_ref_cpu.py): ONE launch each through mpnhip_debug_edge_chain_forward / _backward, i.e. through the
forward's and the backward's own packers and launchers.  Guards, error measure, bound (max(2e-6, 4 x the float32 CPU evaluation's
error)) and the decision rule are those of tests/test_gpu_chain_ops.py; here in addition

  * the rows of msg, hf, dZM and dZF at self loops, which the kernels never write, must still hold their NaN prefill;
  * the mask buffer is followed by 64 words of a pattern that must survive (nothing past mpnhip_debug_edge_chain_mask_ints);
  * dE0 is accumulated into: it is prefilled with finite random values; dE_io holds the incoming gradient and receives dZ2;
  * the inference variant (save = 0) must give e_new, msg and logits bitwise equal to the SAVE variant's, and the hoisted form
    (hoist_e0: Q0 as C-in) must stay within the same bound;
  * the backward is compared with the DEVICE's decisions (value > 0 of the rows the forward stored) imposed on the reference, on the
    mask buffer that forward left: stored bits that disagree with stored values fail the backward.

Shapes.  Every template: (he, de, hn, dn, hc) = 320/64/224/128/32, 160/32/112/64/16, 80/16/56/32/8 (what synth.model_params gives at
d = 128, 64, 32) and the partial-tile set 304/48/208/112/24, in both precisions.  Hand-built edge lists whose three direction groups
have chosen sizes against the kernels' block of 128 edges (four waves of 32): a block and a ragged wave (161), less than a wave
(31), exactly a block (128), an empty group, two self loops and none, E = 1; 24 nodes, one of them the row of the first 70 edges of
its group (a segment across three wave tiles), two nodes that are nobody's row.  With and without edge re-attachment; first_step
0 / 1; skip_e0 where it applies (two column passes: the 128-d sets); sum, mean and max in the backward."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_ref as CR
import segment_ref as SR
from chain_ops_common import (GROUPS, N_NODES, PATTERN, TAIL, WIDTHS, Guarded, decision_exceptions, dev, edge_graph, make_weights, only_counter,
                              report, with_nan_row)
from mpntrackseg_amd import capi, synth

pytestmark = pytest.mark.gpu
SECTIONS = (("H1", "z1"), ("e_new", "z2"), ("HC", "zc"), ("HF", "zf"), ("msg", "zm"))


class Case:
    """One (widths, precision, graph, re-attachment) with its inputs, references and device tensors."""

    def __init__(self, wname, prec, gname, reattach, agg="sum"):
        self.name = "%s %s %s %s %s" % (wname, prec, gname, "cat" if reattach else "nocat", agg)
        self.widths, self.prec, self.reattach, self.agg = WIDTHS[wname], prec, reattach, agg
        he, de, hn, dn, hc = self.widths
        seed = 7 * sum(map(ord, wname + gname)) + reattach
        self.seed = seed
        self.ei = edge_graph(*GROUPS[gname], seed=seed)
        self.E, self.N = self.ei.shape[1], N_NODES
        self.e_out, self.e_in, self.n_self = GROUPS[gname]
        self.csr = SR.graph_csr(self.ei, self.N)
        self.pw = 2 * he + 2 * hn
        self.W = make_weights(self.widths, reattach, seed)
        self.w = CR.edge_weights(self.W, dn, de, reattach)
        self.P = synth.normal(seed, (self.N, self.pw), stream=40)
        self.e0 = np.maximum(synth.normal(seed, (self.E, de), stream=41), 0) if reattach else None
        self.e_prev = np.maximum(synth.normal(seed, (self.E, de), stream=42), 0)
        self.lib = capi.load()
        self.keep = []
        self.Wd = {k: torch.from_numpy(v).to(dev()) for k, v in self.W.items()}
        m = capi.Model()
        lin = lambda prefix: [(self.Wd[prefix + "%d.weight" % i], self.Wd[prefix + "%d.bias" % i]) for i in (0, 2)]
        capi.fill_mlp(m.edge, lin("MPNet.edge_model.edge_model.fc_layers."))
        capi.fill_mlp(m.flow_in, lin("MPNet.node_model.flow_in_model.fc_layers."))
        capi.fill_mlp(m.flow_out, lin("MPNet.node_model.flow_out_model.fc_layers."))
        capi.fill_mlp(m.classifier, lin("classifier.edge_model.fc_layers."))
        m.dn, m.de, m.reattach_nodes, m.reattach_edges = dn, de, 1, int(reattach)
        m.agg, m.precision = capi.AGG_CODE[agg], capi.PRECISIONS[prec]
        self.m = m
        self.pg = capi.PreparedGraph(torch.from_numpy(self.ei).to(dev()), self.N, validate=True, full=True)
        perm = self.pg.buf.cpu().numpy()[256:256 + 4 * self.E].view(np.int32).astype(np.int64)
        assert np.array_equal(perm, self.csr["perm"])
        self.flow = slice(0, self.e_out + self.e_in)
        self.loops = slice(self.e_out + self.e_in, self.E)
        self.ref = CR.edge_chain_forward(self.w, self.csr, self.e_out, self.e_in, self.P, self.e0, self.e_prev, torch.float64)
        self.f32 = CR.edge_chain_forward(self.w, self.csr, self.e_out, self.e_in, self.P, self.e0, self.e_prev, torch.float32)
        for sec, z in SECTIONS:
            rows = self.flow if sec in ("HF", "msg") else slice(None)
            assert decision_exceptions(self.ref[z][rows], self.f32[z][rows].numpy() > 0) <= 1, \
                (self.name, sec, "choose another seed: the float32 evaluation itself is on the edge")

    # ---- forward ---------------------------------------------------------------------------------------------------------------------
    def forward(self, save, hoist=False):
        he, de, hn, dn, hc = self.widths
        E = self.E
        out = dict(e_new=Guarded(E, de), msg=Guarded(E, dn), logits=Guarded(E, 1))
        if save:
            out.update(H1=Guarded(E, he), HC=Guarded(E, hc), HF=Guarded(E, hn))
        nmask = self.lib.mpnhip_debug_edge_chain_mask_ints(C.byref(self.m), E)
        assert nmask > 0
        mask = torch.full((nmask + TAIL,), PATTERN, dtype=torch.int32, device=dev())
        need = self.lib.mpnhip_debug_edge_chain_forward_workspace_bytes(C.byref(self.m), E)
        assert need > 0
        ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=dev())
        self.inputs = [with_nan_row(self.P), with_nan_row(self.e0) if self.reattach else None, with_nan_row(self.e_prev)]
        io = capi.DebugEdgeChainFwd()
        io.P, io.e0, io.e_prev = (None if t is None else t.data_ptr() for t in self.inputs)
        io.e_new, io.msg, io.logits = out["e_new"].ptr(), out["msg"].ptr(), out["logits"].ptr()
        if save:
            io.h1, io.hc, io.hf, io.mask = out["H1"].ptr(), out["HC"].ptr(), out["HF"].ptr(), mask.data_ptr()
        io.save, io.hoist_e0 = int(save), int(hoist)
        capi.path_counters(reset=True)
        capi.check(self.lib.mpnhip_debug_edge_chain_forward(C.byref(self.m), capi.ptr(self.pg.buf), self.N, E, C.byref(io), capi.ptr(ws), need,
                                                            capi.stream_ptr()), "debug_edge_chain_forward")
        torch.cuda.synchronize()
        counts = {k: v for k, v in capi.path_counters(reset=True).items() if v}
        kernel = "edge_chain_fwd_split" if self.prec == "fp32_split" else "edge_chain_fwd"
        assert counts == ({kernel: 1, "gemm_fp32": 1} if hoist else {kernel: 1}), (self.name, counts)
        assert (ws[need:] == 0xFF).all(), "the workspace was written past its stated size"
        m_host = mask.cpu().numpy().view(np.uint32)
        assert (m_host[nmask:] == PATTERN).all(), (self.name, "mask words past mpnhip_debug_edge_chain_mask_ints were written")
        if not save:
            assert (m_host == PATTERN).all(), (self.name, "inference wrote the mask buffer")
        got = {}
        for k, g in out.items():
            got[k] = g.result(self.name + " " + k, nan_rows=self.loops if k in ("msg", "HF") else None)
        got["logits"] = got["logits"].reshape(-1)
        return got, mask

    def check_forward(self, got, tag):
        errs = {}
        for k, v in got.items():
            rows = self.flow if k in ("msg", "HF") else slice(None)
            errs[k] = (CR.rel_err(v[rows], self.ref[k][rows]), CR.rel_err(self.f32[k][rows], self.ref[k][rows]))
        report(self.name + " " + tag, errs)
        for sec, z in SECTIONS:
            if sec in got:
                rows = self.flow if sec in ("HF", "msg") else slice(None)
                assert decision_exceptions(self.ref[z][rows], got[sec][rows] > 0) <= 1, (self.name, sec)

    # ---- backward ----------------------------------------------------------------------------------------------------------------------
    def backward(self, saved, mask, first_step, skip_e0):
        he, de, hn, dn, hc = self.widths
        E, N, seed = self.E, self.N, self.seed
        tag = "bwd first%d skip%d" % (first_step, skip_e0)
        dAGG = synth.normal(seed, (N, 2 * dn), stream=50)
        dlog = synth.normal(seed, (E,), stream=51)
        dE_in = synth.normal(seed, (E, de), stream=52)
        dE0_in = synth.normal(seed, (E, de), stream=53)
        dec = {k: saved[k] > 0 for k, _ in SECTIONS}
        msg = np.where(np.isnan(saved["msg"]), 0, saved["msg"])
        _, ARG = CR.aggregate(msg, self.csr["seg_ptr"], N, self.agg, torch.float32)
        args = (self.w, self.csr, N, self.e_out, self.e_in, self.agg, dec, dAGG, ARG, dlog, dE_in, dE0_in, self.reattach, first_step, skip_e0)
        ref = CR.edge_chain_backward(*args, dtype=torch.float64)
        f32 = CR.edge_chain_backward(*args, dtype=torch.float32)

        out = dict(dZM=Guarded(E, dn), dZF=Guarded(E, hn), dZc=Guarded(E, hc), dZ1=Guarded(E, he), dZ2=Guarded(E, de, fill=dE_in),
                   dE0=Guarded(E, de, fill=dE0_in), dEprev=Guarded(E, de))
        ins = [with_nan_row(dAGG), with_nan_row(dlog.reshape(-1, 1)),
               torch.from_numpy(np.concatenate([ARG.numpy().astype(np.int32), np.full((1, 2 * dn), -7, np.int32)])).to(dev())]
        need = self.lib.mpnhip_debug_edge_chain_backward_workspace_bytes(C.byref(self.m))
        assert need > 0
        ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=dev())
        io = capi.DebugEdgeChainBwd()
        io.dAGG, io.dlog, io.ARG, io.mask = ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr() if self.agg == "max" else None, mask.data_ptr()
        io.dE_io, io.dZM, io.dZF, io.dZc, io.dZ1 = out["dZ2"].ptr(), out["dZM"].ptr(), out["dZF"].ptr(), out["dZc"].ptr(), out["dZ1"].ptr()
        io.dE0, io.dEprev = out["dE0"].ptr(), out["dEprev"].ptr()
        io.first_step, io.skip_e0 = int(first_step), int(skip_e0)
        before = mask.clone()
        capi.path_counters(reset=True)
        capi.check(self.lib.mpnhip_debug_edge_chain_backward(C.byref(self.m), capi.ptr(self.pg.buf), N, E, C.byref(io), capi.ptr(ws), need,
                                                             capi.stream_ptr()), "debug_edge_chain_backward")
        torch.cuda.synchronize()
        only_counter("edge_chain_bwd_split" if self.prec == "fp32_split" else "edge_chain_bwd")
        assert (ws[need:] == 0xFF).all() and torch.equal(mask, before)
        errs = {}
        for k, g in out.items():
            if k == "dEprev" and first_step:
                assert np.isnan(g.t.cpu().numpy()).all(), (self.name, tag, "dEprev written at the first step")
                continue
            v = g.result(self.name + " " + tag + " " + k, nan_rows=self.loops if k in ("dZM", "dZF") else None)
            rows = self.flow if k in ("dZM", "dZF") else slice(None)
            errs[k] = (CR.rel_err(v[rows], ref[k][rows]), CR.rel_err(f32[k][rows], ref[k][rows]))
        report(self.name + " " + tag, errs)


def run_case(wname, prec, gname, reattach, agg="sum"):
    c = Case(wname, prec, gname, reattach, agg)
    saved, mask = c.forward(save=True)
    c.check_forward(saved, "fwd save")
    plain, _ = c.forward(save=False)
    for k, v in plain.items():
        assert np.array_equal(v, saved[k], equal_nan=True), (c.name, k, "inference differs from the SAVE variant")
    de = c.widths[1]
    if reattach and prec == "fp32" and de >= 32 and de % 16 == 0:      # (where the forward takes the hoisted form)
        hoisted, _ = c.forward(save=True, hoist=True)
        c.check_forward(hoisted, "fwd hoist_e0")
    two_passes = reattach and (de + 31) // 32 * 32 == 64
    for first_step in (0, 1):
        for skip_e0 in ((0, 1) if two_passes else (0,)):
            c.backward(saved, mask, first_step, skip_e0)


@pytest.mark.parametrize("reattach", [True, False])
@pytest.mark.parametrize("gname", list(GROUPS))
@pytest.mark.parametrize("prec", ["fp32", "fp32_split"])
@pytest.mark.parametrize("wname", list(WIDTHS))
def test_edge_chain(wname, prec, gname, reattach):
    run_case(wname, prec, gname, reattach)


@pytest.mark.parametrize("agg", ["mean", "max"])
@pytest.mark.parametrize("prec", ["fp32", "fp32_split"])
@pytest.mark.parametrize("wname", ["w128", "w32"])
def test_edge_chain_backward_aggregations(wname, prec, agg):
    run_case(wname, prec, "161-31-2", True, agg)
