"""Shared fixture of the joint-training tests (tests/test_gpu_joint_train.py, tests/dist_joint_train_check.py): a 32-d model with
the mask branch, two small graphs batched block-diagonally with mask inputs and targets, and the yardstick route to the joint
step's gradient -- ``model(data)`` + ``loss.compute_loss`` + ``.backward()`` (existing code, covered against the reference by the
g6 / g21 fixtures)."""
import numpy as np
import torch

from mpntrackseg_amd import loss as mloss
from mpntrackseg_amd import synth
from mpntrackseg_amd.mpn import MOTMPNet

DEV = torch.device("cuda:0")
N_A, N_B = 40, 28


def model_params(num_class_steps=2, L=3, mask=True):
    p = synth.model_params(32, L, "sum", num_class_steps=num_class_steps, node_in_dim=16)
    if mask:
        p.update(synth.MASK_PARAMS)
    return p


def weights(p):
    W = synth.make_weights(p, seed=7)
    if "mask_model_feats_dict" in p:
        W.update(synth.make_mask_weights(seed=17))
    return W


def fresh(p, W=None):
    W = weights(p) if W is None else W
    m = MOTMPNet(p)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    return m.to(DEV).train()


_cache = {}


def host_batch(which="AB", b_rows="some"):
    """Numpy tensors of graph A (40 nodes, 240 edges), graph B (28, 160) or their block-diagonal batch, built once and never
    modified.  ``b_rows``: 'some' = three of B's rows have a ground-truth mask, 'none' = none has."""
    key = (which, b_rows)
    if key in _cache:
        return _cache[key]
    ga = synth.make_graph(N_A, 240, T=6, seed=41, node_in_dim=16)
    gb = synth.make_graph(N_B, 160, T=5, seed=42, node_in_dim=16)
    n = N_A + N_B
    x_ext = synth.normal(5, (n, 256, 14, 14), stream=1, std=0.5)
    mask_labels = (synth.uniform01(6, n * 56 * 56) < 0.5).astype(np.float32).reshape(n, 1, 56, 56)
    gt = np.zeros(n, bool)
    gt[:N_A] = synth.uniform01(7, N_A) < 0.6
    if b_rows == "some":
        gt[N_A + np.array([1, 9, 20])] = True
    lab = (synth.uniform01(8, 240 + 160) < 0.25).astype(np.float32)
    if which == "AB":
        b = synth.batch_graphs([ga, gb])
        out = dict(x=b["x"], edge_index=b["edge_index"], edge_attr=b["edge_attr"], edge_labels=lab, edge_graph=b["edge_graph"],
                   node_graph=b["batch"].astype(np.int32), n_graphs=2, x_ext=x_ext, mask_labels=mask_labels, mask_gt_ixs=gt)
    else:
        g, rows, edges = (ga, slice(0, N_A), slice(0, 240)) if which == "A" else (gb, slice(N_A, n), slice(240, 400))
        k = g["x"].shape[0]
        out = dict(x=g["x"], edge_index=g["edge_index"], edge_attr=g["edge_attr"], edge_labels=lab[edges],
                   edge_graph=np.zeros(g["edge_index"].shape[1], np.int32), node_graph=np.zeros(k, np.int32), n_graphs=1,
                   x_ext=x_ext[rows], mask_labels=mask_labels[rows], mask_gt_ixs=gt[rows])
    _cache[key] = out
    return out


def device_batch(which="AB", b_rows="some"):
    """The batch as the dict ``TrainingBatches`` delivers (device tensors; ``n_graphs`` an int)."""
    return {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in host_batch(which, b_rows).items()}


class _Obj:
    pass


def yardstick(model, b, loss_weights=None):
    """The existing route on ``model`` (gradients are left in ``p.grad``; zeroed first): returns (loss, outputs)."""
    lw = loss_weights or {"tracking": 1, "segmentation": 1}
    for p in model.parameters():
        p.grad = None
    data, batch = _Obj(), _Obj()
    data.x, data.x_ext, data.edge_index, data.edge_attr = b["x"], b["x_ext"], b["edge_index"], b["edge_attr"]
    batch.edge_labels, batch.mask_labels, batch.mask_gt_ixs = b["edge_labels"], b["mask_labels"], b["mask_gt_ixs"]
    out = model(data)
    loss = mloss.compute_loss(out, batch, lw, edge_graph=b["edge_graph"], node_graph=b["node_graph"], n_graphs=b["n_graphs"])
    loss.backward()
    return loss.detach(), out


def flat_like(step, model):
    """``model``'s ``p.grad`` laid out as ``step``'s flat gradient buffer (float64 numpy, padding zero); parameters are matched by
    name, a parameter without gradient counts as zero."""
    names = dict((id(p), n) for n, p in step.model.named_parameters())
    other = dict(model.named_parameters())
    out = np.zeros(step.bucket.n, np.float64)
    for p in step.bucket.params:
        g = other[names[id(p)]].grad
        if g is not None:
            o = step.bucket.offsets[id(p)]
            out[o:o + p.numel()] = g.detach().double().cpu().numpy().ravel()
    return out


def segments(step):
    """{'mask': slice, 'hot': slice} of the flat buffer."""
    return {"mask": slice(0, step.mask_elems), "hot": slice(step.mask_elems, step.bucket.n)}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))
