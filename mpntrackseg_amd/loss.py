"""Host mirror of the reference's loss (``pl_module/pl_module.py:88-120``: the tracking term over ``csrc/loss.hip``, the
segmentation term over ``csrc/train_targets.hip``) and per-step metrics (``utils/evaluation.py:416-437``) -- the steps
right after the hot path; the logit gradient it returns is the seed of ``mpnhip_backward``."""
import ctypes as C

import torch

from . import capi


def edge_graph_ids(batch, edge_index):
    """Graph id of every edge of a block-diagonal batch (torch_geometric ``Batch.batch`` is per NODE): int32 [E]."""
    return batch.to(torch.int32)[edge_index[0]].contiguous()


def tracking_loss_and_grad(logits, edge_labels, first_step=0, weight=1.0, edge_graph=None, n_graphs=1):
    """logits [L, E] (all steps), edge_labels [E] -> (loss_vec [1 + L] on device: total then per step,
    grad_logits [L, E]).  No host synchronisation.  ``edge_graph`` (int32 [E], with ``n_graphs``): the edges belong to the graphs of
    one block-diagonal batch -- per-graph pos_weight and mean, averaged over the graphs (``mpnhip_tracking_loss_graphs``: the
    reference's accumulate_grad_batches executed in space)."""
    capi.require_device(logits, edge_labels)
    lib = capi.load()
    lg = capi.f32c(logits)
    y = capi.f32c(edge_labels).view(-1)
    L, E = lg.shape
    loss = torch.empty(1 + L, dtype=torch.float32, device=lg.device)
    grad = torch.empty_like(lg)
    if edge_graph is not None:
        capi.require_device(edge_graph)
        eg = edge_graph.to(torch.int32).contiguous().view(-1)
        if eg.numel() != E:
            raise capi.MpnhipError("edge_graph must name the graph of each of the %d edges" % E)
        with torch.cuda.device(lg.device):
            ws = capi.workspace(lib.mpnhip_tracking_loss_graphs_workspace_bytes(L, E, int(n_graphs)), lg.device, "loss")
            capi.check(lib.mpnhip_tracking_loss_graphs(capi.ptr(lg), capi.ptr(y), capi.ptr(eg), int(n_graphs), L, E, int(first_step),
                                                       float(weight), capi.ptr(loss), capi.ptr(grad), capi.ptr(ws), ws.numel(),
                                                       capi.stream_ptr()), "mpnhip_tracking_loss_graphs")
        return loss, grad
    with torch.cuda.device(lg.device):
        ws = capi.workspace(lib.mpnhip_tracking_loss_workspace_bytes(L, E), lg.device, "loss")
        capi.check(lib.mpnhip_tracking_loss(capi.ptr(lg), capi.ptr(y), L, E, int(first_step), float(weight), capi.ptr(loss),
                                            capi.ptr(grad), capi.ptr(ws), ws.numel(), capi.stream_ptr()), "mpnhip_tracking_loss")
    return loss, grad


class _TrackingLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, edge_labels, first_step, weight):
        loss, grad = tracking_loss_and_grad(logits.detach(), edge_labels, first_step, weight)
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


def tracking_loss(classified_edges, edge_labels, weight=1.0):
    """``_compute_loss``'s tracking term for the reference's ``outputs['classified_edges']`` list."""
    lg = torch.stack([t.view(-1) for t in classified_edges])
    return _TrackingLoss.apply(lg, edge_labels, 0, weight)


MASK_LOSS_MAX_STEPS = 16   # steps of one mpnhip_mask_loss call (their pointers travel to the kernel by value)


def _valid_flags(mask_gt_ixs, n, device):
    """``batch.mask_gt_ixs`` as bytes [N]: the reference stores a bool mask (mot_graph.py:281); a tensor of row indices (without
    repetitions) is accepted as well."""
    capi.require_device(mask_gt_ixs)
    ix = mask_gt_ixs.view(-1)
    if ix.dtype == torch.bool or ix.dtype == torch.uint8:
        if ix.numel() != n:
            raise capi.MpnhipError("mask_gt_ixs must flag each of the %d rows" % n)
        return ix.contiguous().view(torch.uint8)
    return torch.zeros(n, dtype=torch.uint8, device=device).index_fill_(0, ix.to(torch.int64), 1)


def mask_loss_and_grad(mask_predictions, mask_labels, mask_gt_ixs, weight=1.0, node_graph=None, n_graphs=1):
    """Segmentation term of ``_compute_loss`` (pl_module.py:108-118) for the list ``outputs['mask_predictions']`` (k tensors
    [N, 1, H, W]) -> (loss_vec [1 + k] on the device: total then per step, [grad_s]: d loss / d mask_predictions[s], zero rows where
    ``mask_gt_ixs`` is not set).  One launch for all steps (16 per call), no host synchronisation.  ``node_graph`` (int32 [N], with
    ``n_graphs``): the rows belong to the graphs of one block-diagonal batch -- per-graph mean over the graph's valid rows, averaged
    over the graphs (``tracking_loss_and_grad``'s rule)."""
    preds = list(mask_predictions)
    capi.require_device(mask_labels, *preds)
    lib = capi.load()
    y = capi.f32c(mask_labels)
    dev = y.device
    n = int(y.shape[0]) if y.dim() else 0
    p = y.numel() // n if n else 0
    zs = []
    for t in preds:
        if t.numel() != y.numel():
            raise capi.MpnhipError("mask_predictions %s do not match mask_labels %s" % (tuple(t.shape), tuple(y.shape)))
        zs.append(capi.f32c(t.detach()))
    valid = _valid_flags(mask_gt_ixs, n, dev)
    ng = None
    if node_graph is not None:
        capi.require_device(node_graph)
        ng = node_graph.to(torch.int32).contiguous().view(-1)
        if ng.numel() != n:
            raise capi.MpnhipError("node_graph must name the graph of each of the %d rows" % n)
    k = len(zs)
    grads = [torch.empty_like(z) for z in zs]
    parts = []
    with torch.cuda.device(dev):
        for a in range(0, max(k, 1), MASK_LOSS_MAX_STEPS):
            zc, gc = zs[a:a + MASK_LOSS_MAX_STEPS], grads[a:a + MASK_LOSS_MAX_STEPS]
            kc = len(zc)
            loss = torch.empty(1 + kc, dtype=torch.float32, device=dev)
            ws = capi.workspace(lib.mpnhip_mask_loss_workspace_bytes(kc, n, p, int(n_graphs)), dev, "mask_loss")
            pa = (C.c_void_p * max(kc, 1))(*[z.data_ptr() for z in zc])
            ga = (C.c_void_p * max(kc, 1))(*[g.data_ptr() for g in gc])
            capi.check(lib.mpnhip_mask_loss(pa, kc, capi.ptr(y), capi.ptr(valid), capi.ptr(ng), int(n_graphs), n, p, float(weight),
                                            capi.ptr(loss), ga, capi.ptr(ws), ws.numel(), capi.stream_ptr()), "mpnhip_mask_loss")
            parts.append(loss)
    if len(parts) == 1:
        return parts[0], grads
    per_step = torch.cat([l[1:] for l in parts])
    return torch.cat([torch.stack([l[0] for l in parts]).sum().view(1), per_step]), grads


class _ComputeLoss(torch.autograd.Function):
    """Both terms over the two native ops; inputs: the k logit tensors, then the mask predictions."""

    @staticmethod
    def forward(ctx, k, edge_labels, mask_labels, mask_gt_ixs, w_track, w_seg, edge_graph, node_graph, n_graphs, *tensors):
        logits, masks = tensors[:k], tensors[k:]
        lg = torch.stack([t.detach().reshape(-1) for t in logits])
        tl, glog = tracking_loss_and_grad(lg, edge_labels, 0, w_track, edge_graph=edge_graph, n_graphs=n_graphs)
        total = tl[0]
        saved = [glog]
        if masks:
            ml, gmask = mask_loss_and_grad(masks, mask_labels, mask_gt_ixs, w_seg, node_graph=node_graph, n_graphs=n_graphs)
            total = total + ml[0]
            saved += gmask
        ctx.k = k
        ctx.shapes = [t.shape for t in tensors]
        ctx.save_for_backward(*saved)
        return total

    @staticmethod
    def backward(ctx, g):
        glog, gmask = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        out = [(glog[s] * g).view(ctx.shapes[s]) for s in range(ctx.k)]
        out += [(gm * g).view(ctx.shapes[ctx.k + i]) for i, gm in enumerate(gmask)]
        return (None,) * 9 + tuple(out)


def compute_loss(outputs, batch, loss_weights, edge_graph=None, node_graph=None, n_graphs=1):
    """``MOTNeuralSolver._compute_loss`` (pl_module.py:88-120): a scalar with autograd into every ``outputs['classified_edges'][s]``
    and every ``outputs['mask_predictions'][s]``; ``batch`` carries ``edge_labels``, ``mask_labels`` and ``mask_gt_ixs``,
    ``loss_weights`` is ``hparams['train_params']['loss_weights']`` ('tracking', 'segmentation').  No host synchronisation (the
    reference's ``if gt_masks.numel()`` is one: without a valid row the native term is exactly 0).  ``edge_graph`` / ``node_graph``
    with ``n_graphs``: a block-diagonal batch, each graph its own means, the graph losses averaged.  Outputs without mask
    predictions give the tracking term alone."""
    logits = list(outputs['classified_edges'])
    masks = list(outputs.get('mask_predictions') or []) if getattr(batch, 'mask_labels', None) is not None else []
    if int(n_graphs) > 1 and (edge_graph is None or (masks and node_graph is None)):
        raise capi.MpnhipError("compute_loss: %d graphs need edge_graph (and node_graph with mask predictions)" % int(n_graphs))
    if masks and len(masks) != len(logits):
        raise capi.MpnhipError("%d mask predictions for %d classified steps" % (len(masks), len(logits)))
    return _ComputeLoss.apply(len(logits), batch.edge_labels, getattr(batch, 'mask_labels', None), getattr(batch, 'mask_gt_ixs', None),
                              float(loss_weights['tracking']), float(loss_weights['segmentation']), edge_graph, node_graph,
                              int(n_graphs), *logits, *masks)


@capi.on_tensor_device
def compute_perform_metrics(graph_out, graph_obj):
    """utils/evaluation.py:416-437: {'accuracy','recall','precision','constr_sr'} of the last step's logits."""
    from .mpn import _prepared
    lib = capi.load()
    lg = capi.f32c(graph_out['classified_edges'][-1].detach().view(-1))
    y = capi.f32c(graph_obj.edge_labels).view(-1)
    capi.require_device(lg, y, graph_obj.edge_index)
    n = int(graph_obj.num_nodes) if hasattr(graph_obj, "num_nodes") and graph_obj.num_nodes is not None else int(graph_obj.x.shape[0])
    g = _prepared(graph_obj.edge_index, n, graph_obj)
    counts = torch.empty(8, dtype=torch.int32, device=lg.device)
    with torch.cuda.device(lg.device):
        capi.check(lib.mpnhip_step_metrics(capi.ptr(g.buf), g.N, g.E, capi.ptr(lg), capi.ptr(y), capi.ptr(counts),
                                           capi.stream_ptr()), "mpnhip_step_metrics")
    tp, fp, tn, fn, vo, vi, co, ci = [float(v) for v in counts.tolist()]  # the reference's .item() syncs, once
    tot = tp + fp + tn + fn
    return {"accuracy": (tp + tn) / tot if tot else float("nan"),
            "recall": tp / (tp + fn) if tp + fn > 0 else 0.0,
            "precision": tp / (tp + fp) if tp + fp > 0 else 0.0,
            "constr_sr": 1.0 - (vo + vi) / (co + ci) if co + ci > 0 else float("nan")}


METRIC_COUNT_NAMES = ("tp", "fp", "tn", "fn", "viol_out", "viol_in", "constr_out", "constr_in")


def step_metric_counts(logits_last, edge_labels, edge_index, num_nodes, edge_graph=None, node_graph=None, n_graphs=1, holder=None,
                       out=None):
    """The eight counts of ``compute_perform_metrics`` for each graph of a block-diagonal batch (``mpnhip_step_metrics_graphs``):
    device int32 [n_graphs, 8], rows ``METRIC_COUNT_NAMES``, no host read.  ``logits_last`` [E] is the last step's logits;
    ``edge_graph`` [E] / ``node_graph`` [N] (int32) may be left out for one graph.  ``out``: an int32 [n_graphs, 8] device buffer to
    fill (a row block of ``train.EpochLog``).  ``metrics_from_counts`` turns the counts into the ratios, on the host."""
    from .mpn import _prepared
    capi.require_device(logits_last, edge_labels, edge_index, edge_graph, node_graph)
    lib = capi.load()
    lg = capi.f32c(logits_last.detach()).view(-1)
    y = capi.f32c(edge_labels).view(-1)
    k = int(n_graphs)
    g = _prepared(edge_index, int(num_nodes), holder)
    if lg.numel() != g.E or y.numel() != g.E:
        raise capi.MpnhipError("step_metric_counts: %d logits and %d labels for %d edges" % (lg.numel(), y.numel(), g.E))
    eg = ng = None
    if edge_graph is not None:
        eg = edge_graph.to(torch.int32).contiguous().view(-1)
        if eg.numel() != g.E:
            raise capi.MpnhipError("edge_graph must name the graph of each of the %d edges" % g.E)
    if node_graph is not None:
        ng = node_graph.to(torch.int32).contiguous().view(-1)
        if ng.numel() != g.N:
            raise capi.MpnhipError("node_graph must name the graph of each of the %d nodes" % g.N)
    if out is None:
        out = torch.empty((max(k, 1), 8), dtype=torch.int32, device=lg.device)
    elif out.dtype != torch.int32 or not out.is_contiguous() or out.numel() != 8 * k or out.device != lg.device:
        raise capi.MpnhipError("step_metric_counts: out must be a contiguous int32 [%d, 8] tensor on %s" % (k, lg.device))
    with torch.cuda.device(lg.device):
        capi.check(lib.mpnhip_step_metrics_graphs(capi.ptr(g.buf), g.N, g.E, capi.ptr(lg), capi.ptr(y), capi.ptr(eg), capi.ptr(ng), k,
                                                  capi.ptr(out), capi.stream_ptr()), "mpnhip_step_metrics_graphs")
    return out


def metrics_from_counts(counts):
    """Per-graph ``{'accuracy', 'recall', 'precision', 'constr_sr'}`` (float64 arrays [n_graphs]) from ``step_metric_counts``' table
    with ``compute_perform_metrics``' formulas: accuracy and constr_sr are NaN without edges / constraints, recall and precision
    0.0 without positives.  Runs on the host (a device tensor is read here, once)."""
    import numpy as np
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    c = c.reshape(-1, 8).astype(np.float64)
    tp, fp, tn, fn, vo, vi, co, ci = (c[:, i] for i in range(8))
    tot = tp + fp + tn + fn
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"accuracy": np.where(tot > 0, (tp + tn) / tot, np.nan),
                "recall": np.where(tp + fn > 0, tp / (tp + fn), 0.0),
                "precision": np.where(tp + fp > 0, tp / (tp + fp), 0.0),
                "constr_sr": np.where(co + ci > 0, 1.0 - (vo + vi) / (co + ci), np.nan)}
