"""The inputs of tests/test_gpu_loss_ops.py as ONE table (every input synthesised from fixed seeds), the float32 CPU evaluation of
each of them (torch for the two losses, a numpy float32 restatement of k_adam's expression order for the optimizer) and the
bounds.  tests/test_loss_ref_cpu.py runs the float32 evaluations of the same table against the bounds without a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import loss_ref as LR
from mpntrackseg_amd import synth

U = LR.U
FIXED = 16 * U   # losses and gradients: the count of roundings in the kernels' expressions (tests/test_gpu_loss_ops.py)


def bound(cpu_ratio):
    """max(16 u, 4 x the float32 CPU ratio of the case)"""
    return max(FIXED, 4.0 * cpu_ratio)


# ------------------------------------------------------------------------------------------------ tracking loss
# (E, L, first_step, positive fraction ("one": a single positive, the LAST edge -- the tail of k_count_pos), weight, logit std)
# E = 16389: E / 4 = 4097 -- k_count_pos' 4 x 1024 unrolled loop runs once, its remainder loop for one thread, one tail element.
PLAIN_CASES = [
    (1, 1, 0, 1.0, 1.0, 3.0), (1, 1, 0, 0.0, 1.0, 3.0), (1, 3, 1, "one", 0.37, 3.0),
    (3, 1, 0, "one", 1.0, 3.0), (3, 3, 3, 0.3, 1.0, 3.0), (3, 3, 0, 0.0, 0.37, 3.0),
    (255, 1, 0, 0.3, 1.0, 3.0), (255, 3, 1, 0.02, 0.37, 3.0),
    (256, 1, 1, 0.3, 1.0, 3.0), (256, 3, 0, 0.02, 1.0, 3.0), (256, 3, 1, 1.0, 0.37, 3.0),
    (257, 1, 0, "one", 0.37, 3.0), (257, 3, 1, 0.3, 1.0, 3.0), (257, 3, 3, 0.02, 1.0, 3.0),
    (4099, 1, 0, 0.02, 1.0, 3.0), (4099, 3, 1, 0.3, 0.37, 3.0), (4099, 3, 0, 0.0, 1.0, 3.0), (4099, 3, 0, "one", 1.0, 3.0),
    (16389, 1, 0, 0.3, 0.37, 3.0), (16389, 3, 1, 0.02, 1.0, 3.0), (16389, 3, 0, 1.0, 1.0, 3.0), (16389, 3, 3, 0.3, 1.0, 3.0),
    (16389, 3, 0, "one", 0.37, 3.0), (16389, 1, 0, 0.0, 1.0, 3.0),
    (4099, 3, 0, 0.3, 1.0, 30.0),   # N(0, 30^2) clipped to |z| <= 60: beyond it the sigmoid leaves the normal float32 range
]
SLICE_CASES = [c for c in PLAIN_CASES if c[0] in (4099, 16389) and c[3] in (0.3, "one") and c[5] == 3.0]


def case_id(c):
    return "-".join(str(x) for x in c)


def make_labels(seed, E, frac):
    if frac == "one":
        y = np.zeros(E, np.float32)
        y[E - 1] = 1.0
        return y
    return (synth.uniform01(seed, E) < frac).astype(np.float32)


def make_logits(seed, L, E, std):
    z = synth.normal(seed, (L, E), std=std)
    return np.clip(z, -60.0, 60.0).astype(np.float32)


def plain_inputs(c):
    """-> dict(logits [L, E], labels [E], first_step, weight)"""
    E, L, first, frac, weight, std = c
    seed = 100 + PLAIN_CASES.index(c)
    return dict(logits=make_logits(seed, L, E, std), labels=make_labels(seed + 1000, E, frac), first_step=first, weight=weight)


def _blocks(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)


def _graph_labels(seed, sizes, fracs):
    return np.concatenate([(synth.uniform01(seed + i, int(m)) < f).astype(np.float32) for i, (m, f) in enumerate(zip(sizes, fracs))])


def _shuffle(seed, *arrays):
    perm = np.argsort(synth.uniform01(seed, arrays[0].shape[-1]), kind="stable")
    return tuple(np.ascontiguousarray(a[..., perm]) for a in arrays)


GRAPH_CASES = ("one", "three", "three_shuffled", "eight_out_of_range", "k1024")


def graph_inputs(tag):
    """-> dict(logits, labels, first_step, weight, edge_graph int32 [E], n_graphs).  The ids lie as a batch gives them (contiguous
    blocks) unless the tag says otherwise."""
    if tag == "one":
        sizes, fracs, first, weight, L = (777,), (0.2,), 0, 0.75, 3
    elif tag in ("three", "three_shuffled"):
        sizes, fracs, first, weight, L = (300, 140, 337), (0.2, 0.0, 0.3), 1, 0.37, 3   # the second graph has no positive label
    elif tag == "eight_out_of_range":
        sizes, fracs, first, weight, L = (257, 1, 400, 255, 3, 512, 90, 470), (0.3, 1.0, 0.02, 0.3, 0.3, 0.1, 0.0, 0.5), 0, 1.0, 3
    else:
        sizes = np.floor(synth.uniform01(7, 1024) * 8).astype(np.int64)   # 0 .. 7 edges: some graphs are empty
        assert (sizes == 0).any() and sizes[-1] > 0
        fracs, first, weight, L = (0.3,) * 1024, 0, 1.0, 3
    K = len(sizes)
    seed = 300 + 10 * GRAPH_CASES.index(tag.replace("_shuffled", ""))
    ids = _blocks(sizes)
    E = ids.shape[0]
    logits, labels = make_logits(seed, L, E, 3.0), _graph_labels(seed + 2000, sizes, fracs)
    if tag == "eight_out_of_range":
        ids = ids.copy()
        ids[[0, 100, 256, 257, 700]] = -1         # 5 edges below the range (one of them the only edge of graph 1)
        ids[[300, 913, 914, 1500, E - 1]] = K     # and 5 above it
    if tag == "three_shuffled":
        logits, labels, ids = _shuffle(5, logits, labels, ids)
    return dict(logits=logits, labels=labels, first_step=first, weight=weight, edge_graph=ids, n_graphs=K)


def extreme_inputs():
    """z in {-100, -88, 88, 100}: E = 8, every value under both labels"""
    z = np.array([[-100, -88, 88, 100, -100, -88, 88, 100]], np.float32)
    y = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.float32)
    return dict(logits=z, labels=y, first_step=0, weight=0.37)


def tracking_ref(inp):
    return LR.tracking_loss_ref(inp["logits"], inp["labels"], inp["first_step"], inp["weight"], inp.get("edge_graph"),
                                inp.get("n_graphs", 1))


def tracking_f32(inp, dtype=torch.float32):
    """The same loss with torch in float32 on the CPU (binary_cross_entropy_with_logits and autograd, graph by graph):
    -> (loss [1 + L], grad [L, E]) as ``dtype`` arrays (float64: the pin of the reference itself)"""
    z = torch.from_numpy(inp["logits"]).to(dtype).requires_grad_(True)
    y = torch.from_numpy(inp["labels"]).to(dtype)
    L, E = z.shape
    first, weight = inp["first_step"], inp["weight"]
    ids = inp.get("edge_graph")
    K = inp.get("n_graphs", 1) if ids is not None else 1
    per_step = torch.zeros(L, dtype=torch.float64)   # (the graphs' float32 losses are added in double, as k_loss_reduce does)
    if first < L:
        for g in range(K):
            if ids is None:
                zg, yg = z[first:], y
            else:
                idx = torch.from_numpy(np.nonzero(ids == g)[0])
                if idx.numel() == 0:
                    continue
                zg, yg = z[first:, idx], y[idx]
            P = yg.sum()
            pw = (yg.shape[0] - P) / P if P else torch.zeros(1, dtype=dtype)   # pl_module.py:92-96
            lg = F.binary_cross_entropy_with_logits(zg, yg.expand_as(zg), pos_weight=pw, reduction="none").mean(1) * weight / K
            per_step = per_step + F.pad(lg, (first, 0)).double()
        per_step.sum().backward()
    grad = z.grad if z.grad is not None else torch.zeros(L, E, dtype=dtype)
    loss = torch.cat([per_step.detach().sum().view(1), per_step.detach()]).to(dtype)
    return loss.numpy(), grad.numpy()


def loss_ratios(loss, grad, ref):
    """(worst gradient ratio, worst loss ratio) of an evaluation against a reference tuple (loss, grad, grad_mag, loss_mag);
    exact zeros where the reference has them (asserted)"""
    rl, rg, gm, lm = ref
    return LR.worst_ratio(grad, rg, gm), LR.worst_ratio(loss, rl, lm)


def check_loss(label, loss, grad, ref, f32):
    """the per-element check of a kernel's (loss, grad) against ``ref`` under max(16 u, 4 x the float32 CPU ratio); prints both.
    ``loss`` None: the gradient alone."""
    rl, rg, gm, lm = ref
    g_gpu, g_cpu = LR.worst_ratio(grad, rg, gm), LR.worst_ratio(f32[1], rg, gm)
    l_gpu, l_cpu = (LR.worst_ratio(loss, rl, lm) if loss is not None else 0.0), LR.worst_ratio(f32[0], rl, lm)
    print("%s: gradient kernel %.2f u, float32 CPU %.2f u (bound %.1f u); loss kernel %.2f u, float32 CPU %.2f u (bound %.1f u)"
          % (label, g_gpu / U, g_cpu / U, bound(g_cpu) / U, l_gpu / U, l_cpu / U, bound(l_cpu) / U))
    assert g_gpu <= bound(g_cpu), (label, "gradient", g_gpu / U)
    assert l_gpu <= bound(l_cpu), (label, "loss", l_gpu / U)
    return g_gpu, l_gpu


def check_tracking(label, loss, grad, logits, labels, first_step, weight, edge_graph=None, n_graphs=1):
    """``check_loss`` for tracking-loss results (numpy) on arbitrary float32 inputs: the older GPU tests call it next to their
    own comparisons"""
    inp = dict(logits=np.asarray(logits, np.float32), labels=np.asarray(labels, np.float32).reshape(-1), first_step=first_step,
               weight=weight)
    if edge_graph is not None:
        inp.update(edge_graph=np.asarray(edge_graph), n_graphs=n_graphs)
    return check_loss(label, loss, grad, tracking_ref(inp), tracking_f32(inp))


def check_mask(label, loss, grads, preds, labels, valid, weight, node_graph=None, n_graphs=1):
    """the same for mask-loss results: preds / grads k arrays of N * P elements each, labels [N, ...]"""
    n = np.asarray(labels).shape[0]
    inp = dict(preds=np.stack([np.asarray(p, np.float32).reshape(n, -1) for p in preds]),
               labels=np.asarray(labels, np.float32).reshape(n, -1), valid=np.asarray(valid).reshape(-1).astype(bool), weight=weight)
    if node_graph is not None:
        inp.update(node_graph=np.asarray(node_graph), n_graphs=n_graphs)
    return check_loss(label, loss, np.stack([np.asarray(g).reshape(n, -1) for g in grads]), mask_ref(inp), mask_f32(inp))


# ------------------------------------------------------------------------------------------------ mask loss
MASK_VALID = np.array([1, 0, 1, 1, 0], bool)   # N = 5 rows, 2 of them not valid
# (k, P): P = 15 scalar; 513 scalar, two chunks; 2048 vector, exactly one chunk of 512 units; 2052 vector, two uneven chunks;
# 3136 the real 56 x 56
MASK_CASES = [(1, 15), (3, 513), (16, 2048), (3, 2052), (1, 3136), (16, 3136), (3, 2048)]
MASK_GRAPHS = np.array([0, 1, 2, 3, 0], np.int32)   # 3 graphs: row 3 (valid) names none of them, graph 1 has no valid row


def mask_inputs(k, P, graphs=False):
    """-> dict(preds [k, 5, P], labels [5, P], valid [5], weight[, node_graph, n_graphs])"""
    seed = 500 + 7 * k + P
    preds = np.clip(synth.normal(seed, (k, 5, P), std=3.0), -60.0, 60.0).astype(np.float32)
    labels = (synth.uniform01(seed + 1, 5 * P).reshape(5, P) < 0.4).astype(np.float32)
    inp = dict(preds=preds, labels=labels, valid=MASK_VALID.copy(), weight=1.5)
    if graphs:
        inp.update(node_graph=MASK_GRAPHS.copy(), n_graphs=3)
    return inp


def mask_ref(inp):
    return LR.mask_loss_ref(inp["preds"], inp["labels"], inp["valid"], inp["weight"], inp.get("node_graph"), inp.get("n_graphs", 1))


def mask_f32(inp, dtype=torch.float32):
    """torch in float32 on the CPU over the valid rows of each graph -> (loss [1 + k], grad [k, N, P]) as ``dtype`` arrays"""
    z = torch.from_numpy(inp["preds"]).to(dtype).requires_grad_(True)
    y = torch.from_numpy(inp["labels"]).to(dtype)
    k = z.shape[0]
    ids = inp.get("node_graph")
    K = inp.get("n_graphs", 1) if ids is not None else 1
    per_step = torch.zeros(k, dtype=torch.float64)
    for g in range(K):
        rows = inp["valid"] & ((ids == g) if ids is not None else True)
        if not rows.any():
            continue
        idx = torch.from_numpy(np.nonzero(rows)[0])
        zg, yg = z[:, idx], y[idx]
        lg = F.binary_cross_entropy_with_logits(zg, yg.expand_as(zg), reduction="none").mean((1, 2)) * inp["weight"] / K
        per_step = per_step + lg.double()
    if per_step.requires_grad:   # (not without a valid row)
        per_step.sum().backward()
    loss = torch.cat([per_step.detach().sum().view(1), per_step.detach()]).to(dtype)
    return loss.numpy(), (z.grad if z.grad is not None else torch.zeros_like(z)).detach().numpy()


# ------------------------------------------------------------------------------------------------ Adam
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
# (t, n, weight decay, gradient scale); at scale 1e-8 sqrt(v) is of the order of eps
ADAM_CASES = [(1, 1, 0.0, 1.0), (1, 4099, 1e-4, 1e-8), (1, 257, 0.0, 1e-8), (2, 255, 1e-4, 1.0), (2, 256, 0.0, 1e-8),
              (10, 257, 0.0, 1.0), (10, 4099, 1e-4, 1e-8), (1000, 4099, 0.0, 1e-8), (1000, 256, 1e-4, 1.0), (1000, 1, 1e-4, 1e-8),
              (100000, 255, 0.0, 1e-8), (100000, 4099, 1e-4, 1.0)]
M_BOUND, V_BOUND = 4 * U, 8 * U


def adam_inputs(c):
    """-> (p, g, m, v) float32 [n]; |g| >= 1e-12 (g^2 stays normal in float32); t = 1: the state is m = v = 0"""
    t, n, wd, scale = c
    seed = 700 + ADAM_CASES.index(c)
    p = synth.normal(seed, (n,))
    g = synth.normal(seed + 1, (n,)).astype(np.float64) * scale
    g = (np.where(g < 0, -1.0, 1.0) * np.maximum(np.abs(g), 1e-12)).astype(np.float32)
    if t == 1:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    m = (synth.normal(seed + 2, (n,)).astype(np.float64) * 0.5 * scale).astype(np.float32)
    v = ((0.25 + synth.uniform01(seed + 3, n)) * scale * scale).astype(np.float32)
    return p, g, m, v


def adam_f32(p, g, m, v, t, lr, b1, b2, eps, wd):
    """k_adam in numpy float32, in the kernel's expression order (bias corrections as 1 - powf(beta, t), as on the host for
    mpnhip_adam_step and on the device for the counted form) -> (p', m', v') float32"""
    f = np.float32
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    bc1 = f(1) - np.power(b1, f(t))
    bc2_sqrt = np.sqrt(f(1) - np.power(b2, f(t)))
    gi = g + wd * p
    mi = b1 * m + (f(1) - b1) * gi
    vi = b2 * v + (f(1) - b2) * gi * gi
    denom = np.sqrt(vi) / bc2_sqrt + eps
    out = p - (lr / bc1) * (mi / denom)
    assert out.dtype == np.float32 and mi.dtype == np.float32 and vi.dtype == np.float32
    return out, mi, vi


def adam_bounds(p, ref):
    """(m, v, p) bounds per element from adam_ref's tuple: 4 u m_mag, 8 u v_mag, ulp32(|p|) + 1e-4 dp"""
    _, _, _, m_mag, v_mag, dp = ref
    return M_BOUND * m_mag, V_BOUND * v_mag, LR.ulp32(p) + 1e-4 * dp


def ratio(err, bnd):
    """max err / bnd; where the bound is 0 the error must be 0"""
    err, bnd = np.asarray(err, np.float64), np.asarray(bnd, np.float64)
    assert not err[bnd == 0].any()
    return float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0


def adam_ratios(got, p, ref):
    """(m, v, p) worst |got - ref| / bound of one step's results ``got`` = (p', m', v')"""
    bm, bv, bp = adam_bounds(p, ref)
    return (ratio(np.abs(got[1] - ref[1]), bm), ratio(np.abs(got[2] - ref[2]), bv), ratio(np.abs(got[0] - ref[0]), bp))


# the guarded form on a FlatAdam: 12 calls, a 1 skips the call
GUARD_SKIPS = (1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0)
GUARD_SHAPES = [(37, 5), (128,), (3, 3), (1,)]
GUARD_WD, GUARD_LR = 1e-4, 1e-3


def guarded_inputs():
    """-> (offsets, n, p0 [n], grads [12, n]): train.FlatBucket's layout (every parameter on a 16-byte boundary, padding zero)"""
    offs, n = [], 0
    for s in GUARD_SHAPES:
        offs.append(n)
        n += (int(np.prod(s)) + 3) // 4 * 4
    p0, grads = np.zeros(n, np.float32), np.zeros((len(GUARD_SKIPS), n), np.float32)
    for i, (s, o) in enumerate(zip(GUARD_SHAPES, offs)):
        m = int(np.prod(s))
        p0[o:o + m] = synth.normal(900 + i, (m,))
        grads[:, o:o + m] = synth.normal(910 + i, (len(GUARD_SKIPS), m)) * (1 + np.arange(len(GUARD_SKIPS), dtype=np.float32))[:, None]
    return offs, n, p0, grads


def guarded_reference(p0, grads):
    """adam_ref iterated over the APPLIED calls only -> per call (p, m, v float64 after the call, (m, v, p) accumulated bounds):
    a skipped call repeats the state; the bounds are the per-step bounds summed over the applied steps (an error of the state
    enters the next step with a factor below 1 for m and v and of 1 for p)."""
    hp = dict(HYPER, lr=GUARD_LR, wd=GUARD_WD)
    p, m, v = p0.astype(np.float64), np.zeros(p0.shape), np.zeros(p0.shape)
    bm, bv, bp = np.zeros(p0.shape), np.zeros(p0.shape), np.zeros(p0.shape)
    t, out = 0, []
    for skip, g in zip(GUARD_SKIPS, grads):
        if not skip:
            t += 1
            ref = LR.adam_ref(p, g, m, v, t, **hp)
            b = adam_bounds(p, ref)
            bm, bv, bp = bm + b[0], bv + b[1], bp + b[2]
            p, m, v = ref[:3]
        out.append((p, m, v, (bm, bv, bp)))
    return out


def guarded_f32(p0, grads):
    """the float32 restatement iterated on its own float32 state -> per call (p, m, v)"""
    hp = dict(HYPER, lr=GUARD_LR, wd=GUARD_WD)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    t, out = 0, []
    for skip, g in zip(GUARD_SKIPS, grads):
        if not skip:
            t += 1
            p, m, v = adam_f32(p, g, m, v, t, **hp)
        out.append((p, m, v))
    return out
