"""CPU ORACLE for the neighbour aggregation of the mask branch (``mpnhip_attention_aggregate`` and its backward,
include/mpnhip.h).  TEST INFRASTRUCTURE ONLY: plain torch ops on the CPU, any floating dtype, differentiable by torch autograd
(no hand-derived gradient anywhere).

The operation, per direction (flow_in: edges with row > col, flow_out: edges with row < col; an edge with row == col is in
neither) and per node n, over the segment S(n) = {edges j of the direction with row_j == n}:

    w_j    = exp(l_j - max_{k in S(n)} l_k) / (sum_{k in S(n)} exp(l_k - max) + 1e-12)
    out[n] = sum_{j in S(n)} w_j * x[col_j]                                   (0 for an empty segment)

which is ``scatter_softmax`` of torch_scatter 2.0.4 (a composite of scatter_max, exp, scatter_add and the 1e-12) followed by
``scatter_add``.  PIN: ``tests/golden/g18_attention.npz`` holds the outputs and the autograd gradients of the reference's own
``TimeAwareAttentionModel.forward`` (``tools/make_golden.py gen_g18``); ``tests/test_oracle_golden.py`` checks this file
against it.
"""
import torch

EPS = 1e-12


def _direction(x2, row, col, logits, mask):
    """One direction: (out [N, F], the direction's weights scattered to edge_index order [E], 0 elsewhere)."""
    n = x2.shape[0]
    ids = mask.nonzero().view(-1)           # ascending: the edges of a segment keep their edge_index order
    r, c, l = row[ids], col[ids], logits[ids]
    mx = torch.full((n,), float("-inf"), dtype=l.dtype).scatter_reduce(0, r, l, reduce="amax", include_self=True)
    ex = (l - mx[r]).exp()
    den = torch.zeros(n, dtype=l.dtype).index_add(0, r, ex) + EPS
    w = ex / den[r]
    out = torch.zeros_like(x2).index_add(0, r, w[:, None] * x2[c])
    return out, torch.zeros_like(logits).index_add(0, ids, w)


def attention_aggregate(x, edge_index, logits, dtype=torch.float64):
    """x [N, ...] (trailing dimensions are flattened to F and restored), edge_index int64 [2, E], logits [E] or [E, 1]
    -> (flow_in, flow_out, weights); ``weights`` [E] in edge_index order, 0 on the edges with row == col.  Everything is
    evaluated in ``dtype``; the result is differentiable with respect to ``x`` and ``logits``."""
    row, col = edge_index[0], edge_index[1]
    x2 = x.to(dtype).reshape(x.shape[0], -1)
    lg = logits.to(dtype).reshape(-1)
    flow_in, w_in = _direction(x2, row, col, lg, row > col)
    flow_out, w_out = _direction(x2, row, col, lg, row < col)
    return flow_in.reshape(x.shape), flow_out.reshape(x.shape), w_in + w_out


def attention_aggregate_with_grads(x, edge_index, logits, grad_in, grad_out, dtype=torch.float64):
    """Forward and torch autograd of ``sum(flow_in * grad_in) + sum(flow_out * grad_out)`` with leaves of ``dtype``:
    dict of numpy arrays flow_in, flow_out, weights, grad_x, grad_logits (all of ``dtype``, shaped like the inputs)."""
    xl = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    ll = torch.as_tensor(logits).to(dtype).clone().requires_grad_(True)
    ei = torch.as_tensor(edge_index)
    flow_in, flow_out, w = attention_aggregate(xl, ei, ll, dtype)
    loss = (flow_in * torch.as_tensor(grad_in).to(dtype).reshape(flow_in.shape)).sum() + \
        (flow_out * torch.as_tensor(grad_out).to(dtype).reshape(flow_out.shape)).sum()
    gx, gl = torch.autograd.grad(loss, [xl, ll], allow_unused=True)
    gx = torch.zeros_like(xl) if gx is None else gx
    gl = torch.zeros_like(ll) if gl is None else gl
    return {"flow_in": flow_in.detach().numpy(), "flow_out": flow_out.detach().numpy(), "weights": w.detach().numpy(),
            "grad_x": gx.numpy(), "grad_logits": gl.numpy()}
