"""tests/chain_ref.py (the expectation of tests/test_gpu_chain_ops.py) pinned to the oracle, on the CPU: for an L = 1 and an L = 2
model the node-chain forward must reproduce oracle/mpn_oracle.py's node update of every step from the oracle's own messages, its
projections must give the oracle's first edge-layer pre-activation of the next step, and the backward must equal torch autograd of
the oracle's expressions -- all in float64, to 1e-12 of each tensor's largest magnitude.  In the oracle's bf16 operand mode (float32
by construction) the forward must agree as two float32 evaluations of one formula over identical rounded operands do."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import chain_ref as CR
import segment_ref as SR
from mpntrackseg_amd import synth
from oracle import mpn_oracle as O

EPS64 = 1e-12


def case(d, L, agg, seed):
    params = synth.model_params(d, L, agg, node_in_dim=16)
    W = synth.make_weights(params, seed=seed)
    g = synth.make_graph(26, 180, T=5, seed=seed + 1, node_in_dim=16)
    ei = g["edge_index"].copy()
    ei[:, 7] = [4, 4]
    ei[:, 90] = [11, 11]   # two self loops: in neither aggregate
    g["edge_index"] = ei
    return params, W, g


def node_weights(W, dn, dtype):
    """The packed projection weights [pw, 2 dn] and biases of csrc/mpn.hip (pack_node_weights): the node columns of the edge MLP's first
    layer (row part, col part) and of the two flow MLPs' first layers; the edge layer's bias rides on the row part."""
    kx = 2 * dn
    W1, b1 = W["MPNet.edge_model.edge_model.fc_layers.0.weight"], W["MPNet.edge_model.edge_model.fc_layers.0.bias"]
    Wfo, bfo = W["MPNet.node_model.flow_out_model.fc_layers.0.weight"], W["MPNet.node_model.flow_out_model.fc_layers.0.bias"]
    Wfi, bfi = W["MPNet.node_model.flow_in_model.fc_layers.0.weight"], W["MPNet.node_model.flow_in_model.fc_layers.0.bias"]
    Wnode = torch.cat([W1[:, :kx], W1[:, kx:2 * kx], Wfo[:, :kx], Wfi[:, :kx]]).to(dtype)
    bnode = torch.cat([b1, torch.zeros_like(b1), bfo, bfi]).to(dtype)
    return Wnode, bnode


def oracle_steps(params, W, g, dtype):
    """The oracle's forward unrolled with its own functions: per step (x before, [e0 | e] before, messages M in sorted edge order,
    x after); and the final x of O.forward itself, which the unrolled loop must reproduce."""
    ei = torch.from_numpy(g["edge_index"])
    N = g["x"].shape[0]
    csr = SR.graph_csr(g["edge_index"], N)
    x = O.mlp(torch.from_numpy(g["x"]).to(dtype), W, "encoder.node_model")
    e = O.mlp(torch.from_numpy(g["edge_attr"]).to(dtype), W, "encoder.edge_model")
    x0, e0 = x, e
    row, col = ei
    steps = []
    for _ in range(params["num_enc_steps"]):
        xc, ec = torch.cat((x0, x), 1), torch.cat((e0, e), 1) if params["reattach_initial_edges"] else e
        e_new = O.edge_model(xc, ei, ec, W)
        msg = torch.zeros((ei.shape[1], x.shape[1]), dtype=dtype)
        for mask, name in ((row < col, "flow_out_model"), (row > col, "flow_in_model")):
            msg[mask] = O.mlp(torch.cat([xc[col[mask]], e_new[mask]], 1), W, "MPNet.node_model." + name)
        x_new = O.node_model(xc, ei, e_new, W, params["node_agg_fn"])
        steps.append(dict(x=x, M=msg[torch.from_numpy(csr["perm"])], x_new=x_new, e_new=e_new))
        x, e = x_new, e_new
    _, _, x_fwd, _ = O.forward(params, W, torch.from_numpy(g["x"]).to(dtype), ei, torch.from_numpy(g["edge_attr"]).to(dtype), return_state=True)
    assert torch.equal(x_fwd, x)
    return x0, e0, steps, csr


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("agg", ["sum", "mean", "max"])
def test_node_chain_reference_equals_the_oracle_in_float64(L, agg):
    params, W, g = case(64, L, agg, seed=30 + L)
    dt = torch.float64
    W = O.to_tensors(W, dtype=dt)
    x0, e0, steps, csr = oracle_steps(params, W, g, dt)
    N, dn = x0.shape
    Wu, bu = W["MPNet.node_model.node_model.0.weight"], W["MPNet.node_model.node_model.0.bias"]
    Wnode, bnode = node_weights(W, dn, dt)
    P0 = x0 @ Wnode[:, :dn].T + bnode
    W1 = W["MPNet.edge_model.edge_model.fc_layers.0.weight"]
    b1 = W["MPNet.edge_model.edge_model.fc_layers.0.bias"]
    he = W1.shape[0]
    row, col = torch.from_numpy(g["edge_index"])
    for s, st in enumerate(steps):
        out = CR.node_chain_forward(st["M"], csr["seg_ptr"], N, agg, Wu, bu, Wnode, P0, dt)
        assert CR.rel_err(out["x_new"], st["x_new"]) <= EPS64, s
        # the projections are what the NEXT step's edge layer 0 gathers: Pr[row] + Pc[col] + [e0 | e'] W1e^T is its pre-activation
        P = out["P_next"]
        z_edge = P[row, :he] + P[col, he:2 * he] + torch.cat((e0, st["e_new"]), 1) @ W1[:, 4 * dn:].T
        xc = torch.cat((x0, st["x_new"]), 1)
        ref = F.linear(torch.cat([xc[row], xc[col], e0, st["e_new"]], 1), W1, b1)
        assert CR.rel_err(z_edge, ref) <= EPS64, s
        assert CR.rel_err(P, xc @ Wnode.T + bnode) <= EPS64, s

        # backward: autograd of the oracle's expressions from the aggregate on
        dP = torch.from_numpy(synth.normal(70 + s, tuple(P.shape))).to(dt)
        A = out["agg"].clone().requires_grad_(True)
        z = O.linear(A, Wu, bu)
        z.retain_grad()
        Pn = O.linear(torch.cat((x0, O.relu(z)), 1), Wnode, bnode)
        (Pn * dP).sum().backward()
        got = CR.node_chain_backward(dP, (out["x_new"] > 0).numpy(), Wnode, Wu, dt)
        assert CR.rel_err(got["dZn"], z.grad) <= EPS64 and CR.rel_err(got["dAGG"], A.grad) <= EPS64, s
        assert float(z.grad.abs().max()) > 0 and float(A.grad.abs().max()) > 0


@pytest.mark.parametrize("agg", ["sum", "max"])
def test_node_chain_reference_equals_the_oracle_in_bf16_mode(agg):
    """The oracle's bf16 mode rounds both operands of every Linear product and runs in float32; chain_ref with dtype = float32 and
    round_operands = True multiplies the same rounded operands: 2e-6 covers two float32 summation orders of up to 128 terms
    (the bound the float32 yardstick gets everywhere in the operator tests)."""
    params, W, g = case(64, 1, agg, seed=41)
    Wt = O.to_tensors(W)
    x0, e0, steps, csr = oracle_steps(params, Wt, g, torch.float32)
    N, dn = x0.shape
    Wu, bu = Wt["MPNet.node_model.node_model.0.weight"], Wt["MPNet.node_model.node_model.0.bias"]
    Wnode, bnode = node_weights(Wt, dn, torch.float32)
    P0 = synth.normal(5, (N, Wnode.shape[0]))
    out = CR.node_chain_forward(steps[0]["M"], csr["seg_ptr"], N, agg, Wu, bu, Wnode, P0, torch.float32, round_operands=True)
    with O.precision("bf16"):
        x_new = O.relu(O.linear(out["agg"], Wu, bu))
        # (stage by stage: the oracle's projection product is fed the reference's own x_new, so that a bf16 rounding of x_new that
        # float32 summation noise could turn either way is not carried into P)
        P = torch.from_numpy(P0) + O.linear(out["x_new"], Wnode[:, dn:], None)
    assert CR.rel_err(out["x_new"], x_new) <= 2e-6 and CR.rel_err(out["P_next"], P) <= 2e-6
    # ... and the rounding is really there: the unrounded float32 evaluation differs by bf16's 2^-9 class, not by float32 noise
    plain = CR.node_chain_forward(steps[0]["M"], csr["seg_ptr"], N, agg, Wu, bu, Wnode, P0, torch.float32)
    assert CR.rel_err(plain["x_new"], x_new) > 1e-4


def projections(W, dn, x0, x, dtype):
    """P [N, pw] of one step: [x0 | x] through the packed projection weights (node_weights)."""
    Wnode, bnode = node_weights(W, dn, dtype)
    return torch.cat((x0, x), 1) @ Wnode.T + bnode


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("agg,reattach", [("sum", True), ("mean", False), ("max", True)])
def test_edge_chain_reference_equals_the_oracle_in_float64(L, agg, reattach):
    params, Wn, g = case(64, L, agg, seed=60 + L)
    params["reattach_initial_edges"] = reattach
    Wn = synth.make_weights(params, seed=60 + L)
    dt = torch.float64
    W = O.to_tensors(Wn, dtype=dt)
    x0, e0, steps, csr = oracle_steps(params, W, g, dt)
    N, dn = x0.shape
    de = e0.shape[1]
    ei = torch.from_numpy(g["edge_index"])
    row, col = ei
    perm = torch.from_numpy(csr["perm"])
    d = SR.directions(g["edge_index"])
    e_out, e_in = int((d == 0).sum()), int((d == 1).sum())
    w = CR.edge_weights(W, dn, de, reattach)
    e_prev = e0
    for s, st in enumerate(steps):
        P = projections(W, dn, x0, st["x"], dt)
        out = CR.edge_chain_forward(w, csr, e_out, e_in, P, e0[perm] if reattach else None, e_prev[perm], dt)
        flow = slice(0, e_out + e_in)
        assert CR.rel_err(out["e_new"], st["e_new"][perm]) <= EPS64, s
        assert CR.rel_err(out["logits"], O.classify(st["e_new"], W).view(-1)) <= EPS64, s
        assert CR.rel_err(out["msg"][flow], st["M"][flow]) <= EPS64, s
        assert torch.isnan(out["msg"][e_out + e_in:]).all() and out["msg"].shape[0] - e_out - e_in == 2

        # backward: torch autograd of the oracle's expressions (O.linear / O.relu / its scatter functions) in original edge order,
        # the upstream gradients: of the aggregate, of the logits and of e_new
        first = s == 0
        xc = torch.cat((x0, st["x"]), 1)
        a0 = e0.clone().requires_grad_(True)
        ap = a0 if first else e_prev.clone().requires_grad_(True)
        z1 = O.linear(torch.cat([xc[row], xc[col]] + ([a0] if reattach else []) + [ap], 1), w["W1"], w["b1"])
        z2 = O.linear(O.relu(z1), w["W2"], w["b2"])
        en = O.relu(z2)
        zc = O.linear(en, w["Wc0"], w["bc0"])
        lg = O.linear(O.relu(zc), w["Wc1"], w["bc1"]).view(-1)
        zf = torch.zeros((ei.shape[1], w["Wf0_0"].shape[0]), dtype=dt)
        zm = torch.zeros((ei.shape[1], dn), dtype=dt)
        halves = {}
        for q, mask in ((0, row < col), (1, row > col)):
            f = O.linear(torch.cat([xc[col[mask]], en[mask]], 1), w["Wf0_%d" % q], w["bf0_%d" % q])
            mm = O.linear(O.relu(f), w["Wf1_%d" % q], w["bf1_%d" % q])
            f.retain_grad(); mm.retain_grad()
            halves[q] = (mask, f, mm)
        for t_ in (z1, z2, zc):
            t_.retain_grad()
        AGG = torch.cat([O.AGG[agg](O.relu(halves[1][2]), row[halves[1][0]], N), O.AGG[agg](O.relu(halves[0][2]), row[halves[0][0]], N)], 1)
        dAGG = torch.from_numpy(synth.normal(80 + s, (N, 2 * dn))).to(dt)
        dlog = torch.from_numpy(synth.normal(81 + s, (ei.shape[1],))).to(dt)
        dE_in = torch.from_numpy(synth.normal(82 + s, (ei.shape[1], de))).to(dt)       # sorted order
        dE0_in = torch.from_numpy(synth.normal(83 + s, (ei.shape[1], de))).to(dt)
        dE_orig = torch.empty_like(dE_in)
        dE_orig[perm] = dE_in
        ((AGG * dAGG).sum() + (lg * dlog).sum() + (en * dE_orig).sum()).backward()
        dec = dict(H1=out["z1"] > 0, e_new=out["z2"] > 0, HC=out["zc"] > 0, HF=out["zf"] > 0, msg=out["zm"] > 0)
        _, ARG = CR.aggregate(out["msg"], csr["seg_ptr"], N, agg, dt)
        got = CR.edge_chain_backward(w, csr, N, e_out, e_in, agg, dec, dAGG, ARG, dlog, dE_in, dE0_in, reattach, first, dtype=dt)
        for q in (0, 1):
            mask, f, mm = halves[q]
            pos = torch.nonzero(mask[perm]).view(-1)        # sorted positions of the group, in the order of mask's edges after perm
            ref_m = torch.zeros((ei.shape[1], dn), dtype=dt); ref_m[mask] = mm.grad
            ref_f = torch.zeros((ei.shape[1], f.shape[1]), dtype=dt); ref_f[mask] = f.grad
            assert CR.rel_err(got["dZM"][pos], ref_m[perm][pos]) <= EPS64 and CR.rel_err(got["dZF"][pos], ref_f[perm][pos]) <= EPS64, (s, q)
            assert float(ref_m.abs().max()) > 0 and float(ref_f.abs().max()) > 0
        assert CR.rel_err(got["dZc"], zc.grad[perm]) <= EPS64 and CR.rel_err(got["dZ2"], z2.grad[perm]) <= EPS64, s
        assert CR.rel_err(got["dZ1"], z1.grad[perm]) <= EPS64, s
        if first or reattach:
            assert CR.rel_err(got["dE0"] - dE0_in, a0.grad[perm]) <= EPS64, s
        if not first:
            assert CR.rel_err(got["dEprev"], ap.grad[perm]) <= EPS64, s
        else:
            assert got["dEprev"] is None
        if reattach and not first:
            # skip_e0 leaves out exactly the e0 half
            skipped = CR.edge_chain_backward(w, csr, N, e_out, e_in, agg, dec, dAGG, ARG, dlog, dE_in, dE0_in, reattach, first, True, dtype=dt)
            assert torch.equal(skipped["dE0"], dE0_in) and torch.equal(skipped["dEprev"], got["dEprev"])
        e_prev = st["e_new"]


def test_edge_chain_reference_equals_the_oracle_in_bf16_mode():
    """edge_chain_forward with round_operands = True against the oracle's bf16 mode (float32 by construction): every Linear product
    rounds BOTH operands, the classifier's second layer included.  Compared STAGE BY STAGE (``given``): each stage consumes the
    oracle's own previous stage, because with rounded operands a value within float32 noise of a bf16 rounding boundary rounds either
    way depending on the CPU's summation order, and a whole-chain comparison would carry that 2^-8 flip forward.  Per stage both
    sides multiply identical rounded operands: two float32 summation orders, 2e-6 (the float32 yardstick's bound in the operator
    tests).  The oracle's stages are its own expressions layer by layer, checked bitwise against O.edge_model / O.classify / O.mlp."""
    params, Wn, g = case(64, 1, "sum", seed=71)
    Wt = O.to_tensors(Wn)
    dt = torch.float32
    N = g["x"].shape[0]
    csr = SR.graph_csr(g["edge_index"], N)
    perm = torch.from_numpy(csr["perm"])
    ei = torch.from_numpy(g["edge_index"])
    row, col = ei
    d = SR.directions(g["edge_index"])
    e_out, e_in = int((d == 0).sum()), int((d == 1).sum())
    w = CR.edge_weights(Wt, 64, 32, True)
    with O.precision("bf16"):
        x0 = O.mlp(torch.from_numpy(g["x"]), Wt, "encoder.node_model")
        e0 = O.mlp(torch.from_numpy(g["edge_attr"]), Wt, "encoder.edge_model")
        xc, ec = torch.cat((x0, x0), 1), torch.cat((e0, e0), 1)
        H1 = O.relu(O.linear(torch.cat([xc[row], xc[col], ec], 1), w["W1"], w["b1"]))
        e_new = O.relu(O.linear(H1, w["W2"], w["b2"]))
        assert torch.equal(e_new, O.edge_model(xc, ei, ec, Wt))
        HC = O.relu(O.linear(e_new, w["Wc0"], w["bc0"]))
        logits = O.linear(HC, w["Wc1"], w["bc1"]).view(-1)
        assert torch.equal(logits, O.classify(e_new, Wt).view(-1))
        HF = torch.zeros((ei.shape[1], w["Wf0_0"].shape[0]))
        msg = torch.zeros((ei.shape[1], 64))
        for q, (mask, name) in enumerate(((row < col, "flow_out_model"), (row > col, "flow_in_model"))):
            HF[mask] = O.relu(O.linear(torch.cat([xc[col[mask]], e_new[mask]], 1), w["Wf0_%d" % q], w["bf0_%d" % q]))
            msg[mask] = O.relu(O.linear(HF[mask], w["Wf1_%d" % q], w["bf1_%d" % q]))
            assert torch.equal(msg[mask], O.mlp(torch.cat([xc[col[mask]], e_new[mask]], 1), Wt, "MPNet.node_model." + name))
        # the projections as the oracle's rounded products of the node columns (what the kernels are handed as P)
        Wnode, bnode = node_weights(Wt, 64, dt)
        P = O.linear(xc, Wnode, bnode)
    given = dict(H1=H1[perm], e_new=e_new[perm], HC=HC[perm], HF=HF[perm])
    out = CR.edge_chain_forward(w, csr, e_out, e_in, P, e0[perm], e0[perm], dt, round_operands=True, given=given)
    flow = slice(0, e_out + e_in)
    for k, ref in (("H1", H1[perm]), ("e_new", e_new[perm]), ("HC", HC[perm]), ("HF", HF[perm][flow]), ("msg", msg[perm][flow])):
        got = out[k][flow] if k in ("HF", "msg") else out[k]
        assert CR.rel_err(got, ref) <= 2e-6, k
    assert CR.rel_err(out["logits"], logits) <= 2e-6
    # ... and the rounding matters: fed the same stages, the unrounded float32 evaluation is a bf16-class distance away
    plain = CR.edge_chain_forward(w, csr, e_out, e_in, P, e0[perm], e0[perm], dt, given=given)
    assert CR.rel_err(plain["logits"], logits) > 1e-4 and CR.rel_err(plain["e_new"], e_new[perm]) > 1e-4


def test_aggregate_reference_matches_segment_ref():
    """The aggregation of chain_ref against the sequential reduction tests/segment_ref.py pins to torch_scatter's outputs."""
    params, W, g = case(64, 1, "sum", seed=52)
    N = g["x"].shape[0]
    csr = SR.graph_csr(g["edge_index"], N)
    M = synth.normal(9, (g["edge_index"].shape[1], 8)).astype(np.float64)
    for agg in SR.AGGS:
        got, arg = CR.aggregate(M, csr["seg_ptr"], N, agg, torch.float64)
        ref, rarg = SR.seg_reduce_f64(M, csr["seg_ptr"], 2 * N, agg, nmod=N, off0=8, off1=0)
        # (mean: the kernels multiply by 1 / count, segment_ref divides -- one rounding apart)
        assert np.array_equal(got.numpy(), ref) if agg != "mean" else CR.rel_err(got, ref) <= 1e-15, agg
        if agg == "max":
            assert np.array_equal(arg.numpy(), rarg)
