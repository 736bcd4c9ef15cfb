"""The references of the three kernels that end a training step, in numpy float64: the tracking loss (csrc/loss.hip), the
segmentation loss (csrc/train_targets.hip: mpnhip_mask_loss) and the optimizer step (k_adam).  Every function takes the float32
inputs the kernel gets, computes in float64 and returns, next to the result, the MAGNITUDE its error is measured against: the sum
of the absolute values of the operands of the last addition / subtraction of the formula.  Both aten's formulas and the kernels'
cancel there (y = 1 and large z: sg lw - pw y; y = 0 and z << 0: (1 - y) z + softplus terms), so no float32 evaluation keeps a
bound relative to the result itself.  tests/test_loss_ref_cpu.py pins these functions against float64 torch."""
import numpy as np

U = 2.0 ** -24   # unit roundoff of float32


def _f64(a):
    return np.asarray(a, np.float64)


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _softplus_neg(z):
    """log(1 + exp(-z)), aten's stable form"""
    return np.log1p(np.exp(-np.abs(z))) + np.maximum(-z, 0.0)


def tracking_loss_ref(logits, labels, first_step, weight, edge_graph=None, n_graphs=1):
    """pl_module.py:88-107: per step ``weight`` * mean_i [(1 - y) z + lw softplus(-z)] with lw = 1 + (pw - 1) y and
    pw = (E - P) / P (0 without a positive label); steps below ``first_step`` give loss 0 and gradient 0.  With ``edge_graph``
    (csrc/loss.hip's per-graph contract): each of the ``n_graphs`` graphs its own edge count, P, pw and mean, the graph losses
    averaged (a graph without edges contributes 0), the gradient divided by Eg * K; an edge whose id is outside [0, K) belongs to no
    graph: zero gradient, counted nowhere.

    -> (loss [1 + L], grad [L, E], grad_mag [L, E], loss_mag [1 + L]); loss[0] / loss_mag[0]: the sum over the steps."""
    z, y = _f64(logits), _f64(labels).reshape(-1)
    L, E = z.shape
    K = int(n_graphs) if edge_graph is not None else 1
    ids = np.zeros(E, np.int64) if edge_graph is None else np.asarray(edge_graph, np.int64).reshape(-1)
    inside = (ids >= 0) & (ids < K)
    safe = np.where(inside, ids, 0)
    Eg = np.bincount(safe[inside], minlength=K).astype(np.float64)
    Pg = np.bincount(safe[inside], weights=y[inside], minlength=K)
    pwg = np.where(Pg > 0, (Eg - Pg) / np.maximum(Pg, 1.0), 0.0)
    pw = pwg[safe]
    scale = np.where(inside, weight / (np.maximum(Eg[safe], 1.0) * K), 0.0)   # weight / (Eg K) per edge
    lw = 1.0 + (pw - 1.0) * y
    live = (np.arange(L) >= first_step)[:, None].astype(np.float64)
    sp, sg = _softplus_neg(z), _sigmoid(z)
    term = ((1.0 - y) * z + lw * sp) * scale * live
    term_mag = (np.abs((1.0 - y) * z) + lw * sp) * scale * live
    grad = (sg * lw - pw * y) * scale * live
    grad_mag = (sg * lw + pw * y) * scale * live
    loss, loss_mag = np.zeros(1 + L), np.zeros(1 + L)
    loss[1:], loss_mag[1:] = term.sum(1), term_mag.sum(1)
    loss[0], loss_mag[0] = loss[1:].sum(), loss_mag[1:].sum()
    return loss, grad, grad_mag, loss_mag


def mask_loss_ref(preds, labels, valid, weight, node_graph=None, n_graphs=1):
    """mpnhip_mask_loss: per step the plain BCE-with-logits mean over the valid rows of each graph, the graph means averaged
    (a graph without a valid row contributes 0).  preds [k, N, P] (or k arrays of N * P elements), labels [N, P], valid [N].
    Rows that are not valid or whose id is outside [0, K) have gradient exactly 0.

    -> (loss [1 + k], grad [k, N, P], grad_mag [k, N, P] = (sg + y) gs, loss_mag [1 + k])"""
    y = _f64(labels)
    N = y.shape[0]
    y = y.reshape(N, -1)
    P = y.shape[1]
    k = len(preds)
    z = np.stack([_f64(p).reshape(N, P) for p in preds]) if k else np.zeros((0, N, P))
    K = int(n_graphs) if node_graph is not None else 1
    ids = np.zeros(N, np.int64) if node_graph is None else np.asarray(node_graph, np.int64).reshape(-1)
    ok = np.asarray(valid).reshape(-1).astype(bool) & (ids >= 0) & (ids < K)
    safe = np.where(ok, ids, 0)
    cnt = np.bincount(safe[ok], minlength=K).astype(np.float64)
    gs = np.where(ok, weight / (np.maximum(cnt[safe], 1.0) * P * K), 0.0)[None, :, None]
    sp, sg = _softplus_neg(z), _sigmoid(z)
    term = ((1.0 - y) * z + sp) * gs
    term_mag = (np.abs((1.0 - y) * z) + sp) * gs
    grad, grad_mag = (sg - y) * gs, (sg + np.abs(y)) * gs
    loss, loss_mag = np.zeros(1 + k), np.zeros(1 + k)
    loss[1:], loss_mag[1:] = term.sum((1, 2)), term_mag.sum((1, 2))
    loss[0], loss_mag[0] = loss[1:].sum(), loss_mag[1:].sum()
    return loss, grad, grad_mag, loss_mag


def adam_hyper(lr, b1, b2, eps, wd):
    """the five hyper-parameters as the C ABI receives them: rounded to float32 (1 - 0.999 alone differs by 1.3e-5 relative between
    the double and the float32 value of 0.999), as Python floats"""
    return tuple(float(np.float32(x)) for x in (lr, b1, b2, eps, wd))


def adam_ref(p, g, m, v, t, lr, b1, b2, eps, wd):
    """One torch.optim.Adam step (not AdamW: L2 decay joins the gradient), the t-th, in float64 with the float32-rounded
    hyper-parameters.  -> (p', m', v', m_mag, v_mag, dp) with m_mag = |b1 m| + (1 - b1)(|g| + |wd p|),
    v_mag = b2 v + (1 - b2)(|g| + |wd p|)^2 and dp = |p' - p|."""
    lr, b1, b2, eps, wd = adam_hyper(lr, b1, b2, eps, wd)
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    gi = g + wd * p
    ga = np.abs(g) + np.abs(wd * p)
    m1 = b1 * m + (1.0 - b1) * gi
    v1 = b2 * v + (1.0 - b2) * gi * gi
    bc1 = 1.0 - b1 ** float(t)
    bc2 = 1.0 - b2 ** float(t)
    denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    p1 = p - (lr / bc1) * (m1 / denom)
    m_mag = np.abs(b1 * m) + abs(1.0 - b1) * ga
    v_mag = b2 * v + (1.0 - b2) * ga * ga
    return p1, m1, v1, m_mag, v_mag, np.abs(p1 - p)


def ulp32(x):
    """spacing of float32 at |x| (float64 array)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def worst_ratio(got, ref, mag):
    """max |got - ref| / mag over the elements with mag > 0 (0.0 without one); where mag == 0 the reference is exactly 0 and
    ``got`` must be exactly 0 too: asserted here."""
    got, ref, mag = _f64(got), _f64(ref), _f64(mag)
    zero = mag == 0
    assert not ref[zero].any()
    assert not got[zero].any(), "non-zero where the reference is exactly 0"
    assert np.isfinite(got).all()
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / mag[~zero]).max())
