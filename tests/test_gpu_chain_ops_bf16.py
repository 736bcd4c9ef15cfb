"""Operator-level parity of the bf16-operand chain kernels (csrc/edge_chain_bf16.hip: edge_chain_bf16_kernel; csrc/edge_chain_bf16_bwd.hip:
edge_chain_bf16_bwd_kernel), ONE launch each through mpnhip_debug_edge_chain_bf16_forward and mpnhip_debug_edge_chain_backward in
MPNHIP_PREC_BF16 (the forward's and the backward's own packers and launchers), compared STAGE BY STAGE: against a whole-chain
reference an intermediate within fp32 noise of a bf16 rounding boundary would need a loose bound, so each stage's reference (tests/
chain_ref.py's product with both operands rounded to bfloat16, float64 sums) consumes the DEVICE's own stored previous stage, all of
which the SAVE variant returns:  inputs -> H1;  H1 -> e_new;  e16 -> HC, HF;  HC -> logits;  HF -> msg.

Bounds.  fp32 results (e_new, logits, msg) against the float64 product of the same bf16 operands: 2e-5 of max(1, max |ref|), the
project's bf16 operator bound (tests/test_gpu_gemm_bf16.py).  Outputs kept as bf16 rows (H1, HC, HF): |got - ref| <= 2^-8 |ref| +
2e-5 max(1, max |ref|) element by element (2^-8: bfloat16's unit roundoff).  e16 must be bitwise the nearest-even rounding of e_new.
The inference variant, the bf16-row input form (rows16), the plain-barrier form and the fused aggregation's e_new / logits must be
bitwise equal to the SAVE variant's; the fused aggregation's agg_out is held to max(2e-6, 4 x the float32 CPU evaluation's error)
against the float64 aggregate of the device's own msg (an fp32 sum of fp32 values), and max must be bitwise.

Decisions.  The decoded mask sections must equal (value > 0) of the decoded rows exactly -- bits and values come from the same
registers -- and the stage references' decisions except within 2e-5 x rms of zero (tests/test_gpu_pinned.py), at most one unit per
section and case.  Guards as in tests/test_gpu_chain_ops_edge.py: NaN guard rows round every output, a NaN row behind every input, the
rows of msg / hf at self loops untouched (hf: still the workspace's prefill), a pattern behind the mask buffer and the workspace, the
msg buffer untouched when the kernel aggregates, the path counter.

Backward.  On the mask buffer the SAVE forward left, with the device's DECODED decisions imposed on the reference, each stage's
reference again consumes the device's own stored previous stage: gathered dAGG -> dZM; dZM -> dZF; dlog -> dZc; dE_in, dZF, dZc ->
dZ2; dZ2 -> dZ1; dZ1 -> dEprev (or, at the first step, += into dE0).  The five dZ blocks are the bf16 rows the kernel stores (bound of bf16
rows), dEprev / dE0 fp32 (2e-5); sum, mean and max; first_step 0 and 1; dE_in must come back unchanged, the buffer of dE0 / dEprev that a
step does not write too, and the rows of dZM / dZF at self loops.

Shapes: every template -- 320/64/224/128/32, 160/32/112/64/16, 80/16/56/32/8, the partial-tile set 304/48/208/112/24 and the 256-d
template 640/128/448/256/64 (exact widths only) -- with direction groups sized against the block mpnhip_debug_edge_chain_bf16_geometry
reports (256 edges, 128 at 256-d): a block and a ragged wave, less than a wave, exactly a block, empty, E = 1; 24 nodes, one the row
of 70 consecutive edges (a segment across three wave tiles: the fused aggregation's piece / fix-up path), rows without edges."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_ref as CR
import segment_ref as SR
from chain_ops_common import (FLOOR_TOL, GUARD, N_NODES, PATTERN, TAIL, WIDTHS as W32, Guarded, decision_exceptions, dev, edge_graph, make_weights,
                              with_nan_row)
from mpntrackseg_amd import capi, synth

pytestmark = pytest.mark.gpu
WIDTHS = dict(W32, w256=(640, 128, 448, 256, 64))
# group sizes in units of (block, extra edges): (row < col, row > col, self loops)
GROUPS = {"B+33,31,2": ((1, 33), (0, 31), 2), "B,0,0": ((1, 0), (0, 0), 0), "0,B+33,2": ((0, 0), (1, 33), 2), "1,0,0": ((0, 1), (0, 0), 0)}
BF16_TOL = 2e-5
U_BF16 = 2.0 ** -8


def bf16_round(a):
    return SR.bf16_value(SR.bf16_bits(np.ascontiguousarray(a, np.float32)))


def check_f32(name, got, ref):
    ref = np.asarray(ref, np.float64)
    e = float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0
    print("CHAIN_ERR %-44s fp32 result  %.2e of max(1, max |ref|)  (bound %.0e)" % (name, e, BF16_TOL))
    assert e <= BF16_TOL, (name, e)


def check_rows16(name, got, ref):
    ref = np.asarray(ref, np.float64)
    if not ref.size:
        return
    excess = np.abs(got - ref) - U_BF16 * np.abs(ref)
    scale = max(1.0, float(np.abs(ref).max()))
    e = float(excess.max()) / scale
    nz = np.abs(ref) > 0
    rel = float((np.abs(got - ref)[nz] / np.abs(ref)[nz]).max()) if nz.any() else 0.0
    print("CHAIN_ERR %-44s bf16 rows    %.2e of max(1, max |ref|) beyond 2^-8 |ref|  (bound %.0e); largest |err| / |ref| %.2e (2^-8 = 3.9e-03)"
          % (name, e, BF16_TOL, rel))
    assert e <= BF16_TOL, (name, e)


class Bf16Case:
    def __init__(self, wname, gname, agg="sum"):
        self.name = "bf16 %s %s" % (wname, gname)
        self.widths, self.agg = WIDTHS[wname], agg
        he, de, hn, dn, hc = self.widths
        self.lib = capi.load()
        seed = 11 * sum(map(ord, wname + gname))
        self.W = make_weights(self.widths, True, seed)
        self.Wd = {k: torch.from_numpy(v).to(dev()) for k, v in self.W.items()}
        m = capi.Model()
        lin = lambda prefix: [(self.Wd[prefix + "%d.weight" % i], self.Wd[prefix + "%d.bias" % i]) for i in (0, 2)]
        capi.fill_mlp(m.edge, lin("MPNet.edge_model.edge_model.fc_layers."))
        capi.fill_mlp(m.flow_in, lin("MPNet.node_model.flow_in_model.fc_layers."))
        capi.fill_mlp(m.flow_out, lin("MPNet.node_model.flow_out_model.fc_layers."))
        capi.fill_mlp(m.classifier, lin("classifier.edge_model.fc_layers."))
        m.dn, m.de, m.reattach_nodes, m.reattach_edges = dn, de, 1, 1
        m.agg, m.precision = capi.AGG_CODE[agg], capi.PRECISIONS["bf16"]
        self.m = m
        epb, nw = C.c_int32(0), C.c_int32(0)
        self.lib.mpnhip_debug_edge_chain_bf16_geometry(C.byref(m), C.byref(epb), C.byref(nw))
        assert (epb.value, nw.value) == ((128, 4) if wname == "w256" else (256, 8))
        (b0, x0), (b1, x1), self.n_self = GROUPS[gname]
        self.e_out, self.e_in = b0 * epb.value + x0, b1 * epb.value + x1
        self.ei = edge_graph(self.e_out, self.e_in, self.n_self, seed)
        self.E, self.N = self.ei.shape[1], N_NODES
        self.csr = SR.graph_csr(self.ei, self.N)
        self.perm = self.csr["perm"]
        self.w = CR.edge_weights(self.W, dn, de, True)
        self.P = synth.normal(seed, (self.N, 2 * he + 2 * hn), stream=40)
        self.e0 = np.maximum(synth.normal(seed, (self.E, de), stream=41), 0)
        self.e_prev = np.maximum(synth.normal(seed, (self.E, de), stream=42), 0)
        self.pg = capi.PreparedGraph(torch.from_numpy(self.ei).to(dev()), self.N, validate=True, full=True)
        assert np.array_equal(self.pg.buf.cpu().numpy()[256:256 + 4 * self.E].view(np.int32).astype(np.int64), self.perm)
        self.flow = slice(0, self.e_out + self.e_in)
        self.loops = slice(self.e_out + self.e_in, self.E)

    def run(self, save=0, rows16=0, fused_agg=0, plain=0):
        he, de, hn, dn, hc = self.widths
        E, N = self.E, self.N
        tag = "%s save%d rows%d agg%d plain%d" % (self.name, save, rows16, fused_agg, plain)
        out = dict(e_new=Guarded(E, de), msg=Guarded(E, dn), logits=Guarded(E, 1), agg=Guarded(N, 2 * dn))
        if save or rows16:
            out["e16"] = Guarded(E, de)
        if save:
            out.update(h1=Guarded(E, he), hc=Guarded(E, hc), hf=Guarded(E, hn), dec_h1=Guarded(E, he), dec_e=Guarded(E, de),
                       dec_hc=Guarded(E, hc), dec_hf=Guarded(E, hn), dec_m=Guarded(E, dn))
        nmask = self.lib.mpnhip_debug_edge_chain_bf16_mask_ints(C.byref(self.m), E)
        need = self.lib.mpnhip_debug_edge_chain_bf16_forward_workspace_bytes(C.byref(self.m), E)
        assert nmask > 0 and need > 0
        mask = torch.full((nmask + TAIL,), PATTERN, dtype=torch.int32, device=dev())
        ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=dev())
        ins = [with_nan_row(self.P), with_nan_row(self.e0), with_nan_row(self.e_prev)]
        io = capi.DebugEdgeChainBf16Fwd()
        io.P, io.e0, io.e_prev = (t.data_ptr() for t in ins)
        io.e_new, io.logits = out["e_new"].ptr(), out["logits"].ptr()
        io.msg, io.agg_out = (None, out["agg"].ptr()) if fused_agg else (out["msg"].ptr(), None)
        for k in out:
            if k in ("e16", "h1", "hc", "hf") or k.startswith("dec_"):
                setattr(io, k, out[k].ptr())
        io.mask = mask.data_ptr()
        io.save, io.rows16, io.fused_agg, io.plain_barriers = save, rows16, fused_agg, plain
        capi.path_counters(reset=True)
        capi.check(self.lib.mpnhip_debug_edge_chain_bf16_forward(C.byref(self.m), capi.ptr(self.pg.buf), N, E, C.byref(io), capi.ptr(ws), need,
                                                                 capi.stream_ptr()), "debug_edge_chain_bf16_forward")
        torch.cuda.synchronize()
        counts = {k: v for k, v in capi.path_counters(reset=True).items() if v}
        assert counts == {"edge_chain_fwd_bf16": 1}, (tag, counts)
        assert (ws[need:] == 0xFF).all(), (tag, "the workspace was written past its stated size")
        mh = mask.cpu().numpy().view(np.uint32)
        assert (mh[nmask:] == PATTERN).all(), (tag, "mask words past mpnhip_debug_edge_chain_bf16_mask_ints were written")
        if not save:
            assert (mh == PATTERN).all(), (tag, "the inference variant wrote the mask buffer")
        got = {}
        unwritten = ("agg",) if not fused_agg else ("msg",)
        for k, g in out.items():
            if k in unwritten:
                assert np.isnan(g.t.cpu().numpy()).all(), (tag, k, "written although not asked for")
                continue
            # (decoded tensors come back in ORIGINAL order: brought to sorted order here; the hf rows of self loops decode the
            # workspace's 0xFF prefill, a NaN)
            orig = k in ("e16", "h1", "hc", "hf") or k.startswith("dec_")
            body = g.result(tag + " " + k, nan_rows=(self.perm[self.loops] if orig else self.loops) if k in ("msg", "hf") else None)
            got[k] = body[self.perm] if orig else body
        got["logits"] = got["logits"].reshape(-1)
        self.last_mask = mask
        return got


def run_bf16_case(wname, gname):
    c = Bf16Case(wname, gname)
    he, de, hn, dn, hc = c.widths
    w, csr, P = c.w, c.csr, torch.from_numpy(c.P).double()
    kx = w["kx"]
    srow, scol = torch.as_tensor(csr["srow"]), torch.as_tensor(csr["scol"])
    t = lambda a: torch.as_tensor(np.asarray(a)).double()
    prod = lambda a, b: CR.product(t(a), t(b), torch.float64, True)
    g = c.run(save=1)
    flow, e_out, e_in = c.flow, c.e_out, c.e_in

    # ---- stage by stage, each reference fed with the device's own previous stage -------------------------------------------------
    z = {}
    z["h1"] = prod(np.concatenate([c.e0, c.e_prev], 1), w["W1"][:, 2 * kx:]) + P[srow, :he] + P[scol, he:2 * he]
    check_rows16(c.name + " H1", g["h1"], torch.relu(z["h1"]))
    z["e"] = prod(g["h1"], w["W2"]) + t(w["b2"])
    check_f32(c.name + " e_new", g["e_new"], torch.relu(z["e"]))
    assert np.array_equal(g["e16"].view(np.uint32), bf16_round(g["e_new"]).view(np.uint32)), (c.name, "e16 is not the RNE rounding of e_new")
    z["hc"] = prod(g["e16"], w["Wc0"]) + t(w["bc0"])
    check_rows16(c.name + " HC", g["hc"], torch.relu(z["hc"]))
    lg = t(g["hc"]) @ t(bf16_round(w["Wc1"].reshape(-1))) + float(w["bc1"].reshape(-1)[0])
    check_f32(c.name + " logits", g["logits"][c.perm], lg)
    z["hf"] = torch.zeros((c.E, hn), dtype=torch.float64)
    z["m"] = torch.zeros((c.E, dn), dtype=torch.float64)
    for q, (b, e) in enumerate(((0, e_out), (e_out, e_out + e_in))):
        z["hf"][b:e] = prod(g["e16"][b:e], w["Wf0_%d" % q][:, kx:]) + P[scol[b:e], 2 * he + q * hn:2 * he + (q + 1) * hn]
        z["m"][b:e] = prod(g["hf"][b:e], w["Wf1_%d" % q]) + t(w["bf1_%d" % q])
    check_rows16(c.name + " HF", g["hf"][flow], torch.relu(z["hf"][flow]))
    check_f32(c.name + " msg", g["msg"][flow], torch.relu(z["m"][flow]))

    # ---- decisions: bits against stored values (exact), and against the stage references (margin) ---------------------------------
    for sec, val, rows in (("h1", g["h1"], slice(None)), ("e", g["e16"], slice(None)), ("hc", g["hc"], slice(None)), ("hf", g["hf"], flow),
                           ("m", g["msg"], flow)):
        dec = g["dec_" + sec][rows] > 0
        assert set(np.unique(g["dec_" + sec])) <= {0.0, 1.0}
        assert np.array_equal(dec, val[rows] > 0), (c.name, sec, "decision bits disagree with the stored values")
        assert decision_exceptions(z[sec][rows], dec) <= 1, (c.name, sec)
    assert not g["dec_hf"][c.loops].any() and not g["dec_m"][c.loops].any()

    # ---- the other variants: bitwise ---------------------------------------------------------------------------------------------------
    def same(a, b, what):
        for k in ("e_new", "msg", "logits"):
            if k in a and k in b:
                assert np.array_equal(a[k], b[k], equal_nan=True), (c.name, what, k, "differs from the SAVE variant")

    same(c.run(save=0), g, "inference")
    same(c.run(save=0, plain=1), g, "plain barriers")
    same(c.run(save=1, plain=1), g, "plain barriers, SAVE")
    if de % 8 == 0:
        r16 = c.run(save=0, rows16=1)
        same(r16, g, "rows16")
        assert np.array_equal(r16["e16"].view(np.uint32), g["e16"].view(np.uint32)), (c.name, "rows16: e16 differs")
    msg = np.where(np.isnan(g["msg"]), 0, g["msg"])
    for agg in ("sum", "mean", "max"):
        c.m.agg = capi.AGG_CODE[agg]
        for save in (0, 1):
            if save and agg == "max":
                continue                      # (a training forward with max keeps the separate aggregation, which records the arg max)
            fa = c.run(save=save, fused_agg=1)
            same(fa, g, "fused aggregation " + agg)
            ref, _ = CR.aggregate(msg, csr["seg_ptr"], c.N, agg, torch.float64)
            f32, _ = CR.aggregate(msg, csr["seg_ptr"], c.N, agg, torch.float32)
            e, e32 = CR.rel_err(fa["agg"], ref), CR.rel_err(f32, ref)
            print("CHAIN_ERR %-44s agg_out      kernel %.2e  float32-cpu %.2e" % (c.name + " " + agg, e, e32))
            assert e <= max(FLOOR_TOL, 4.0 * e32), (c.name, agg, e, e32)
            if agg == "max":
                assert np.array_equal(fa["agg"], f32.numpy()), (c.name, "max must return its inputs bit for bit")
    c.m.agg = capi.AGG_CODE["sum"]


@pytest.mark.parametrize("gname", list(GROUPS))
@pytest.mark.parametrize("wname", list(WIDTHS))
def test_edge_chain_bf16_forward(wname, gname):
    run_bf16_case(wname, gname)


class Guarded16:
    """[GUARD + rows + GUARD, width] bf16 bit patterns on the device, all 0x7FC0 (a NaN); the operator gets the address of row GUARD."""
    NAN_BITS = 0x7FC0

    def __init__(self, rows, width):
        self.G, self.rows, self.width = GUARD, rows, width
        self.t = torch.full((rows + 2 * GUARD, width), self.NAN_BITS, dtype=torch.int16, device=dev())

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 2 * self.G * self.width)

    def result(self, name, nan_rows=None):
        bits = self.t.cpu().numpy().view(np.uint16)
        assert (bits[:self.G] == self.NAN_BITS).all() and (bits[self.G + self.rows:] == self.NAN_BITS).all(), (name, "guard rows written")
        body = SR.bf16_value(bits[self.G:self.G + self.rows])
        written = np.ones(self.rows, bool)
        if nan_rows is not None:
            written[nan_rows] = False
            assert (bits[self.G:self.G + self.rows][~written] == self.NAN_BITS).all(), (name, "rows of self loops were written")
        assert np.isfinite(body[written]).all(), (name, "rows left unwritten or non-finite")
        return body


def run_bf16_backward(c, g, agg, first_step):
    he, de, hn, dn, hc = c.widths
    E, N, w, csr = c.E, c.N, c.w, c.csr
    kx = w["kx"]
    name = "%s bwd %s first%d" % (c.name, agg, first_step)
    seed = 13 * E + first_step
    dAGG, dlog = synth.normal(seed, (N, 2 * dn), stream=50), synth.normal(seed, (E,), stream=51)
    dE_in, dE0_in = synth.normal(seed, (E, de), stream=52), synth.normal(seed, (E, de), stream=53)
    msg = np.where(np.isnan(g["msg"]), 0, g["msg"])
    _, ARG = CR.aggregate(msg, csr["seg_ptr"], N, agg, torch.float32)
    c.m.agg = capi.AGG_CODE[agg]
    out16 = dict(dZM=Guarded16(E, dn), dZF=Guarded16(E, hn), dZc=Guarded16(E, hc), dZ2=Guarded16(E, de), dZ1=Guarded16(E, he))
    dEin_g, dE0_g, dEp_g = Guarded(E, de, fill=dE_in), Guarded(E, de, fill=dE0_in), Guarded(E, de)
    ins = [with_nan_row(dAGG), with_nan_row(dlog.reshape(-1, 1)),
           torch.from_numpy(np.concatenate([ARG.numpy().astype(np.int32), np.full((1, 2 * dn), -7, np.int32)])).to(dev())]
    need = c.lib.mpnhip_debug_edge_chain_backward_workspace_bytes(C.byref(c.m))
    assert need > 0
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=dev())
    io = capi.DebugEdgeChainBwd()
    io.dAGG, io.dlog, io.ARG, io.mask = ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr() if agg == "max" else None, c.last_mask.data_ptr()
    io.dE_io, io.dE0, io.dEprev = dEin_g.ptr(), dE0_g.ptr(), dEp_g.ptr()
    for k, b in out16.items():
        setattr(io, k, b.ptr())
    io.first_step = first_step
    before = c.last_mask.clone()
    capi.path_counters(reset=True)
    capi.check(c.lib.mpnhip_debug_edge_chain_backward(C.byref(c.m), capi.ptr(c.pg.buf), N, E, C.byref(io), capi.ptr(ws), need, capi.stream_ptr()),
               "debug_edge_chain_backward (bf16)")
    torch.cuda.synchronize()
    counts = {k: v for k, v in capi.path_counters(reset=True).items() if v}
    assert counts == {"edge_chain_bwd_bf16": 1}, (name, counts)
    assert (ws[need:] == 0xFF).all() and torch.equal(c.last_mask, before)
    d = {k: b.result(name + " " + k, nan_rows=c.loops if k in ("dZM", "dZF") else None) for k, b in out16.items()}
    assert np.array_equal(dEin_g.result(name + " dE_in"), dE_in), (name, "dE_in was written")

    # ---- stage by stage on the device's own rows and decisions -----------------------------------------------------------------------
    t = lambda a: torch.as_tensor(np.asarray(a)).double()
    prod = lambda a, b: CR.product(t(a), t(b), torch.float64, True)
    dec = {k: t(g["dec_" + k] > 0) for k in ("h1", "e", "hc", "hf", "m")}
    srow = np.asarray(csr["srow"])
    flow_term = torch.zeros((E, de), dtype=torch.float64)
    for q, (b, e) in enumerate(((0, c.e_out), (c.e_out, c.e_out + c.e_in))):
        c0 = dn if q == 0 else 0
        g0 = t(dAGG)[srow[b:e], c0:c0 + dn]
        if agg == "mean":
            g0 = g0 / t(np.maximum(np.diff(np.asarray(csr["seg_ptr"]))[q * N + srow[b:e]], 1))[:, None]
        elif agg == "max":
            g0 = g0 * t(ARG.numpy()[srow[b:e], c0:c0 + dn] == np.arange(b, e)[:, None])
        check_rows16(name + " dZM", d["dZM"][b:e], g0 * dec["m"][b:e])
        check_rows16(name + " dZF", d["dZF"][b:e], prod(d["dZM"][b:e], w["Wf1_%d" % q].T) * dec["hf"][b:e])
        flow_term[b:e] = prod(d["dZF"][b:e], w["Wf0_%d" % q][:, kx:].T)
    dl = t(dlog)[csr["perm"]]
    check_rows16(name + " dZc", d["dZc"], dl[:, None] * t(bf16_round(w["Wc1"].reshape(1, -1))) * dec["hc"])
    check_rows16(name + " dZ2", d["dZ2"], (t(dE_in) + flow_term + prod(d["dZc"], w["Wc0"].T)) * dec["e"])
    check_rows16(name + " dZ1", d["dZ1"], prod(d["dZ2"], w["W2"].T) * dec["h1"])
    dp = prod(d["dZ1"], w["W1"][:, 2 * kx + de:].T)
    if first_step:
        check_f32(name + " dE0", dE0_g.result(name + " dE0"), t(dE0_in) + dp)
        assert np.isnan(dEp_g.t.cpu().numpy()).all(), (name, "dEprev written at the first step")
    else:
        check_f32(name + " dEprev", dEp_g.result(name + " dEprev"), dp)
        assert np.array_equal(dE0_g.result(name + " dE0"), dE0_in), (name, "dE0 written at a later step")
    c.m.agg = capi.AGG_CODE["sum"]


@pytest.mark.parametrize("gname", list(GROUPS))
@pytest.mark.parametrize("wname", list(WIDTHS))
def test_edge_chain_bf16_backward(wname, gname):
    c = Bf16Case(wname, gname)
    g = c.run(save=1)
    for agg in ("sum", "mean", "max"):
        for first_step in (0, 1):
            run_bf16_backward(c, g, agg, first_step)


def test_edge_chain_bf16_refusals_before_any_launch():
    """Other precisions, no re-attachment, rows16 / save at widths they do not take: MPNHIP_ERR_UNSUPPORTED, nothing launched."""
    c = Bf16Case("w32", "1,0,0")
    lib, p = c.lib, capi.ptr(torch.zeros(1 << 16, dtype=torch.float32, device=dev()))
    io = capi.DebugEdgeChainBf16Fwd()
    for n, _ in io._fields_[:17]:
        setattr(io, n, p.value)
    call = lambda: lib.mpnhip_debug_edge_chain_bf16_forward(C.byref(c.m), capi.ptr(c.pg.buf), c.N, c.E, C.byref(io), p, 1 << 40, capi.stream_ptr())
    capi.path_counters(reset=True)
    c.m.precision = capi.PRECISIONS["fp32"]
    assert call() == -4 and lib.mpnhip_debug_edge_chain_bf16_mask_ints(C.byref(c.m), 5) == 0
    c.m.precision = capi.PRECISIONS["bf16"]
    io.rows16, io.e16 = 1, None   # rows16 without a buffer for the mirror
    assert call() == -1
    c.m.reattach_edges = 0
    assert call() != 0
    torch.cuda.synchronize()
    assert not any(capi.path_counters(reset=True).values())
