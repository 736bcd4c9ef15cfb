"""Plain torch restatement of the fused chain operators (test infrastructure only).  The node side, written from the formulas of
include/mpnhip.h (mpnhip_debug_node_chain, mpnhip_debug_node_chain_backward) and the three node-chain lines of csrc/common.h:

    forward   AGG = [agg(flow_in messages) | agg(flow_out messages)],  x' = relu(Wu AGG + bu),  P' = P0 + Wx x'
    backward  dX = dP Wx,  dZn = dX (.) [x_prev > 0],  dAGG = dZn Wu               (Wx = Wnode[:, dn:2 dn])

``dtype``: torch.float64 (the expectation) or torch.float32 (the yardstick of what an fp32 evaluation of the same formula loses).
``round_operands``: both operands of every product are rounded to bfloat16 (round to nearest even); sums, biases, the aggregation
and the ReLU stay in ``dtype`` -- the oracle's "bf16" precision.  The node-chain kernels themselves never round: they take
every fp32 operand as three bf16 pieces (MPNHIP_PREC_FP32_SPLIT), so the GPU tests call this with round_operands = False.

What the kernels feed against what they store (csrc/node_chain.hip):
  * forward: the aggregate row is split into pieces from the SAME fp32 registers that go to agg_out, and the projections are
    computed from the fp32 x' tile that is stored as x_new -- stored and fed values are identical, nothing is rounded between stages;
    sum / mean add a segment's rows in ascending sorted position and mean multiplies by 1 / max(count, 1) (one rounding more
    than a division);
  * backward: dAGG is computed from the fp32 dZn tile that is stored; x_prev is read only for its sign (x > 0).

The per-edge chain (include/mpnhip.h: mpnhip_debug_edge_chain_forward / _backward; the header of csrc/edge_chain.hip and its steps
B1 - B6) is restated by edge_chain_forward / edge_chain_backward below, everything in SORTED edge order.  What the fp32 / split
kernels feed against what they store (csrc/edge_chain.hip): every stage's accumulator tile, after bias and ReLU in place, IS the next
product's operand and is what the save / output rows receive -- identical fp32 values; the split form takes them as three bf16
pieces (nothing rounded to bf16), and its backward keeps every other edge's gradients negated in registers, flipping them back on
every store.  The classifier's second layer is an fp32 fma chain, not a matrix product.  Q0 (hoist_e0) is a separate fp32 GEMM whose
result is the C-in of the first layer: another summation order of the same H1.

The bf16-operand forward kernel (csrc/edge_chain_bf16.hip) rounds BOTH operands of every product to bfloat16 and feeds what it
stores: a finished H1 / HF tile is rounded to bf16 once, and those bf16 values are the rows it keeps AND the next product's operand;
e' is stored as fp32 but consumed as its bf16 rounding (the e16 mirror); the classifier's second layer multiplies bf16(wc2) with the
bf16 rounding of HC in an fp32 fma chain; the ReLU decisions are taken on the rounded values.  tests/test_gpu_chain_ops_bf16.py
therefore evaluates ``product(..., round_operands=True)`` stage by stage on the device's own stored previous stage.

The bf16 backward kernel (csrc/edge_chain_bf16_bwd.hip) mirrors that: a finished dZ tile is rounded to bf16 once, stored so and fed
so; dZc = dlog x bf16(wc2) with the fp32 dlog; dE' is an fp32 accumulator that takes dE_in unrounded; dEprev / dE0 stay fp32.

tests/test_chain_ref_cpu.py pins the forward to oracle/mpn_oracle.py (float64, and the oracle's bf16 mode with round_operands = True)
and the backward to torch autograd of the oracle in float64.  edge_chain_backward with round_operands = True is NOT pinned to the
oracle: torch autograd through the oracle's rounding casts rounds the gradients differently from the kernels (it is the stage formula
the bf16 GPU test evaluates through ``product``, stage by stage)."""
import numpy as np
import torch


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _rnd(t, on):
    return t.bfloat16().to(t.dtype) if on else t


def product(a, b_t, dtype, round_operands=False):
    """a [m, k] times b_t [n, k] transposed, both operands rounded when asked, accumulated in ``dtype``."""
    return _rnd(a.to(dtype), round_operands) @ _rnd(b_t.to(dtype), round_operands).T


def aggregate(M, seg_ptr, N, agg, dtype):
    """[N, 2 dn] = [flow_in | flow_out] over the CSR seg_ptr of the keys dir * N + row (dir 0 flow_out, 1 flow_in), rows of M in
    sorted edge order, added one after the other in ``dtype``; empty segments give 0.  Returns (AGG, arg): arg [N, 2 dn] the
    sorted position a max took (first maximum, -1 elsewhere / for sum and mean)."""
    M = _t(M, dtype)
    dn = M.shape[1]
    out = torch.zeros((N, 2 * dn), dtype=dtype)
    arg = torch.full((N, 2 * dn), -1, dtype=torch.int64)
    for n in range(N):
        for q, c0 in ((0, dn), (1, 0)):
            b, e = int(seg_ptr[q * N + n]), int(seg_ptr[q * N + n + 1])
            if e <= b:
                continue
            rows = M[b:e]
            if agg == "max":
                v, i = rows.max(dim=0)
                # first maximum: torch.max may return any index among ties
                i = (rows == v).to(torch.int64).argmax(dim=0)
                out[n, c0:c0 + dn], arg[n, c0:c0 + dn] = v, i + b
            else:
                acc = torch.zeros(dn, dtype=dtype)
                for r in rows:
                    acc = acc + r
                out[n, c0:c0 + dn] = acc * (torch.ones((), dtype=dtype) / (e - b)) if agg == "mean" else acc
    return out, arg


def node_chain_forward(M, seg_ptr, N, agg, Wu, bu, Wnode, P0, dtype=torch.float64, round_operands=False):
    """dict(agg, z, x_new, P_next): z the node update's pre-activation (its sign is the ReLU decision).  P0 None: no P_next."""
    Wu, bu, Wnode = _t(Wu, dtype), _t(bu, dtype), _t(Wnode, dtype)
    dn = Wu.shape[0]
    AGG, arg = aggregate(M, seg_ptr, N, agg, dtype)
    z = product(AGG, Wu, dtype, round_operands) + bu
    x_new = torch.relu(z)
    P_next = None if P0 is None else _t(P0, dtype) + product(x_new, Wnode[:, dn:2 * dn], dtype, round_operands)
    return dict(agg=AGG, arg=arg, z=z, x_new=x_new, P_next=P_next)


def node_chain_backward(dP, decisions, Wnode, Wu, dtype=torch.float64, round_operands=False):
    """dict(dZn, dAGG) for the ReLU ``decisions`` [N, dn] (bool: x_prev > 0) -- a linear map of dP once they are fixed."""
    Wu, Wnode = _t(Wu, dtype), _t(Wnode, dtype)
    dn = Wu.shape[0]
    dX = product(_t(dP, dtype), Wnode[:, dn:2 * dn].T, dtype, round_operands)
    dZn = dX * torch.as_tensor(np.asarray(decisions)).to(dtype)
    return dict(dZn=dZn, dAGG=product(dZn, Wu.T, dtype, round_operands))


def edge_weights(W, dn, de, reattach_edges):
    """The per-edge modules' weights out of a reference state dict (numpy or torch values) under the names used below; kx is read
    off the edge MLP's input width as the C entry does."""
    g = lambda k: W[k]
    ke = (2 if reattach_edges else 1) * de
    E, F, Cl = "MPNet.edge_model.edge_model.fc_layers.", "MPNet.node_model.flow_%s_model.fc_layers.", "classifier.edge_model.fc_layers."
    w = dict(W1=g(E + "0.weight"), b1=g(E + "0.bias"), W2=g(E + "2.weight"), b2=g(E + "2.bias"),
             Wc0=g(Cl + "0.weight"), bc0=g(Cl + "0.bias"), Wc1=g(Cl + "2.weight"), bc1=g(Cl + "2.bias"))
    for q, name in enumerate(("out", "in")):
        w["Wf0_%d" % q], w["bf0_%d" % q] = g(F % name + "0.weight"), g(F % name + "0.bias")
        w["Wf1_%d" % q], w["bf1_%d" % q] = g(F % name + "2.weight"), g(F % name + "2.bias")
    w["kx"] = (int(w["W1"].shape[1]) - ke) // 2
    return w


def edge_chain_forward(w, csr, e_out, e_in, P, e0, e_prev, dtype=torch.float64, round_operands=False, given=None):
    """One step of the per-edge chain.  w: edge_weights(); csr: segment_ref.graph_csr(); e_out / e_in: the sizes of direction groups
    0 and 1 (the self loops follow); P [N, pw] = [Pr | Pc | Pf_out | Pf_in]; e0 (None without re-attachment) and e_prev [E, de] in
    sorted order.  Returns pre-activations z_* and values: H1, e_new, HC, logits (ORIGINAL order), HF, msg (rows of self loops: NaN,
    the kernels never write them).  ``given`` (stage-by-stage evaluation, for the bf16 mode): a dict with any of H1, e_new, HC, HF
    [E, width]; a stage that is given is what the NEXT product consumes instead of this function's own value of it -- with rounded
    operands a value within float32 noise of a bf16 rounding boundary may round either way, and a whole-chain comparison of two
    float32 evaluations would carry that flip (2^-8 of one hidden unit) into everything behind it."""
    given = given or {}
    fed = lambda k, own: t(given[k]) if k in given else own
    t = lambda a: _t(a, dtype)
    W1, kx = t(w["W1"]), w["kx"]
    he = W1.shape[0]
    hn = w["Wf0_0"].shape[0]
    P, ep = t(P), t(e_prev)
    srow, scol = torch.as_tensor(csr["srow"]), torch.as_tensor(csr["scol"])
    E = ep.shape[0]
    x1 = ep if e0 is None else torch.cat((t(e0), ep), 1)
    z1 = product(x1, W1[:, 2 * kx:], dtype, round_operands) + P[srow, :he] + P[scol, he:2 * he]
    H1 = torch.relu(z1)
    z2 = product(fed("H1", H1), t(w["W2"]), dtype, round_operands) + t(w["b2"])
    e_new = torch.relu(z2)
    zc = product(fed("e_new", e_new), t(w["Wc0"]), dtype, round_operands) + t(w["bc0"])
    HC = torch.relu(zc)
    lg = product(fed("HC", HC), t(w["Wc1"]), dtype, round_operands).reshape(-1) + t(w["bc1"]).reshape(())
    logits = torch.empty(E, dtype=dtype)
    logits[torch.as_tensor(csr["perm"])] = lg
    zf = torch.full((E, hn), float("nan"), dtype=dtype)
    zm = torch.full((E, w["Wf1_0"].shape[0]), float("nan"), dtype=dtype)
    for q, (b, e) in enumerate(((0, e_out), (e_out, e_out + e_in))):
        zf[b:e] = product(fed("e_new", e_new)[b:e], t(w["Wf0_%d" % q])[:, kx:], dtype, round_operands) + P[scol[b:e], 2 * he + q * hn:2 * he + (q + 1) * hn]
        zm[b:e] = product(fed("HF", torch.relu(zf))[b:e], t(w["Wf1_%d" % q]), dtype, round_operands) + t(w["bf1_%d" % q])
    return dict(z1=z1, H1=H1, z2=z2, e_new=e_new, zc=zc, HC=HC, logits=logits, zf=zf, HF=torch.relu(zf), zm=zm, msg=torch.relu(zm))


def edge_chain_backward(w, csr, N, e_out, e_in, agg, dec, dAGG, ARG, dlog, dE_in, dE0_in, reattach_edges, first_step, skip_e0=False,
                        dtype=torch.float64, round_operands=False):
    """B1 - B6 for the decisions ``dec`` = dict(H1, e_new, HC, HF, msg: bool [E, width], sorted order; rows of self loops of HF / msg
    are ignored) and ``ARG`` [N, 2 dn] (max: the sorted position the forward took) -- a linear map of (dAGG, dlog, dE_in, dE0_in)
    once they are fixed.  dlog in ORIGINAL order.  Returns dZM, dZF (self-loop rows NaN), dZc, dZ2, dZ1, dE0 (= dE0_in + ...),
    dEprev (None at the first step)."""
    t = lambda a: _t(a, dtype)
    m = lambda k: torch.as_tensor(np.asarray(dec[k])).to(dtype)
    kx = w["kx"]
    dn, hn, de = w["Wf1_0"].shape[0], w["Wf0_0"].shape[0], w["W2"].shape[0]
    srow = torch.as_tensor(csr["srow"])
    E = srow.shape[0]
    dAGG, dE = t(dAGG), t(dE_in).clone()
    dZM = torch.full((E, dn), float("nan"), dtype=dtype)
    dZF = torch.full((E, hn), float("nan"), dtype=dtype)
    for q, (b, e) in enumerate(((0, e_out), (e_out, e_out + e_in))):
        c0 = dn if q == 0 else 0
        g = dAGG[srow[b:e], c0:c0 + dn]
        if agg == "mean":
            cnt = np.diff(np.asarray(csr["seg_ptr"]))[q * N + np.asarray(csr["srow"][b:e])]
            g = g / torch.as_tensor(np.maximum(cnt, 1)).to(dtype)[:, None]
        elif agg == "max":
            took = torch.as_tensor(np.asarray(ARG))[srow[b:e], c0:c0 + dn] == torch.arange(b, e)[:, None]
            g = g * took.to(dtype)
        dZM[b:e] = g * m("msg")[b:e]
        dZF[b:e] = product(dZM[b:e], t(w["Wf1_%d" % q]).T, dtype, round_operands) * m("HF")[b:e]
        dE[b:e] = dE[b:e] + product(dZF[b:e], t(w["Wf0_%d" % q])[:, kx:].T, dtype, round_operands)
    dl = t(dlog)[torch.as_tensor(csr["perm"])]
    # (the gradient arriving at the logit is NOT rounded: the bf16 kernel multiplies the fp32 dlog with the rounded weight)
    dZc = dl[:, None] * _rnd(t(w["Wc1"]), round_operands).reshape(1, -1) * m("HC")
    dE = dE + product(dZc, t(w["Wc0"]).T, dtype, round_operands)
    dZ2 = dE * m("e_new")
    dZ1 = product(dZ2, t(w["W2"]).T, dtype, round_operands) * m("H1")
    dcat = product(dZ1, t(w["W1"])[:, 2 * kx:].T, dtype, round_operands)
    dE0 = t(dE0_in).clone()
    if reattach_edges:
        d0, dp = dcat[:, :de], dcat[:, de:]
        if not skip_e0:
            dE0 = dE0 + d0
    else:
        dp = dcat
    dEprev = None
    if first_step:
        dE0 = dE0 + dp
    else:
        dEprev = dp
    return dict(dZM=dZM, dZF=dZF, dZc=dZc, dZ2=dZ2, dZ1=dZ1, dE0=dE0, dEprev=dEprev)


def rel_err(got, ref, floor=1e-30):
    """max |got - ref| / max(max |ref|, floor) over ALL elements: one wrong element fails it."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), floor))
