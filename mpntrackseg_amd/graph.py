"""Host mirror of the reference's graph utilities (``src/mot_neural_solver/utils/graph.py``) and of
``MOTGraph.construct_graph_object`` (``data/mot_graph.py:283-317``) over the C ABI -- SURVEY.md section 8 rows f-3/f-4.

Same function names and argument meaning as the reference; tensors live on the HIP device (there is no CPU fallback).
``det_df`` may be a pandas DataFrame or any mapping with the columns the reference reads (``frame``, ``bb_height``,
``bb_width``, ``feet_x``, ``feet_y``)."""
import ctypes as C

import numpy as np
import torch

from . import capi
from .capi import MpnhipError, check, ptr, stream_ptr


def _dev(device=None):
    if not torch.cuda.is_available():
        raise MpnhipError("mpntrackseg_amd.graph needs a HIP device; there is no CPU fallback")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _col(det_df, name, dtype, device):
    v = det_df[name]
    v = v.values if hasattr(v, "values") else v
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v))).to(device=device, dtype=dtype)


@capi.on_tensor_device
def compact(flags):
    """ids (int32, ascending) of the set flags and their number (one host read: the consumers are sized by it)."""
    lib = capi.load()
    n = flags.numel()
    ids = torch.empty(max(n, 1), dtype=torch.int32, device=flags.device)
    count = torch.empty(1, dtype=torch.int32, device=flags.device)
    ws = capi.workspace(lib.mpnhip_compact_workspace_bytes(n), flags.device, "compact")
    check(lib.mpnhip_compact(ptr(flags), n, ptr(ids), ptr(count), ptr(ws), ws.numel(), stream_ptr()), "mpnhip_compact")
    k = int(count.item())
    return ids[:k], k


@capi.on_tensor_device
def gather_rows(src, ids):
    lib = capi.load()
    src = capi.f32c(src)
    src2 = src.view(src.shape[0], -1)
    out = torch.empty((ids.numel(), src2.shape[1]), dtype=torch.float32, device=src.device)
    check(lib.mpnhip_gather_rows(ptr(src2), src2.shape[1], ptr(ids), ids.numel(), src2.shape[1], ptr(out), stream_ptr()),
          "mpnhip_gather_rows")
    return out


@capi.on_tensor_device
def gather_edges(edge_index, ids, node_begin):
    lib = capi.load()
    out = torch.empty((2, ids.numel()), dtype=torch.int64, device=edge_index.device)
    check(lib.mpnhip_gather_edges(ptr(edge_index), edge_index.shape[1], ptr(ids), ids.numel(), int(node_begin), ptr(out),
                                  stream_ptr()), "mpnhip_gather_edges")
    return out


@capi.on_tensor_device
def get_time_valid_conn_ixs(frame_num, max_frame_dist, use_cuda=True, return_undirected=True):
    """utils/graph.py:6-37.  ``frame_num``: int tensor [N]; ``max_frame_dist``: int or ``'max'``.
    Returns int64 ``[2, num_pairs]`` with row < col, on the device (the reference moves it back to the CPU); with
    ``return_undirected=False`` the reference's ``(row, col)`` tuple over ALL ordered pairs (both directions, the row-major
    order of ``torch.where``), on the device as well."""
    assert isinstance(max_frame_dist, (int, np.integer)) or max_frame_dist == 'max'
    lib = capi.load()
    dev = frame_num.device if isinstance(frame_num, torch.Tensor) and frame_num.is_cuda else _dev()
    frames = torch.as_tensor(frame_num).to(device=dev, dtype=torch.int64).contiguous().view(-1)
    n = frames.numel()
    maxd = -1 if max_frame_dist == 'max' else int(max_frame_dist)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nbytes = lib.mpnhip_time_valid_conn_workspace_bytes(n)
    ws = capi.workspace(nbytes, dev, "graph_build")
    count, fill = ((lib.mpnhip_time_valid_conn_count, lib.mpnhip_time_valid_conn_fill) if return_undirected else
                   (lib.mpnhip_time_valid_conn_directed_count, lib.mpnhip_time_valid_conn_directed_fill))
    check(count(ptr(frames), n, maxd, ptr(offsets), ptr(ws), ws.numel(), stream_ptr()), "mpnhip_time_valid_conn_count")
    n_pairs = int(offsets[n].item())  # the one host read: the result has to be allocated
    out = torch.empty((2, n_pairs), dtype=torch.int64, device=dev)
    check(fill(ptr(frames), n, maxd, ptr(offsets), n_pairs, ptr(out), stream_ptr()), "mpnhip_time_valid_conn_fill")
    return out if return_undirected else (out[0], out[1])


@capi.on_tensor_device
def get_knn_mask(pwise_dist, edge_ixs, num_nodes, top_k_nns, use_cuda=True, reciprocal_k_nns=False, symmetric_edges=True):
    """utils/graph.py:40-87.  Returns a bool tensor [num_edges]: True = keep."""
    lib = capi.load()
    capi.require_device(edge_ixs)
    dev = edge_ixs.device
    ei = edge_ixs.to(torch.int64).contiguous()
    d = pwise_dist.to(device=dev, dtype=torch.float32).contiguous().view(-1)
    e = ei.shape[1]
    assert d.numel() == e, "one distance per edge"
    mask = torch.empty(e, dtype=torch.uint8, device=dev)
    nbytes = lib.mpnhip_knn_mask_workspace_bytes(e, 1 if symmetric_edges else 0)
    ws = capi.workspace(nbytes, dev, "knn")
    check(lib.mpnhip_knn_mask(ptr(d), ptr(ei), int(num_nodes), e, int(top_k_nns), 1 if reciprocal_k_nns else 0,
                              1 if symmetric_edges else 0, ptr(mask), ptr(ws), ws.numel(), stream_ptr()), "mpnhip_knn_mask")
    return mask.bool()


EDGE_FEAT_NAMES = ('secs_time_dists', 'norm_feet_x_dists', 'norm_feet_y_dists', 'bb_height_dists', 'bb_width_dists')


@capi.on_tensor_device
def compute_edge_feats_dict(edge_ixs, det_df, fps, use_cuda=True):
    """utils/graph.py:90-124.  Returns the reference's dict: feature name -> tensor [num_edges]."""
    lib = capi.load()
    capi.require_device(edge_ixs)
    dev = edge_ixs.device
    ei = edge_ixs.to(torch.int64).contiguous()
    e = ei.shape[1]
    frame = _col(det_df, 'frame', torch.int64, dev)
    cols = [_col(det_df, k, torch.float32, dev) for k in ('bb_height', 'bb_width', 'feet_x', 'feet_y')]
    out = torch.empty((e, 5), dtype=torch.float32, device=dev)
    check(lib.mpnhip_edge_features(ptr(ei), e, frame.numel(), ptr(frame), C.c_float(float(fps)), ptr(cols[0]), ptr(cols[1]),
                                   ptr(cols[2]), ptr(cols[3]), ptr(out), stream_ptr()), "mpnhip_edge_features")
    return {name: out[:, i] for i, name in enumerate(EDGE_FEAT_NAMES)}


@capi.on_tensor_device
def pairwise_distance(emb, edge_ixs, eps=1e-6):
    """``F.pairwise_distance(emb[edge_ixs[0]], emb[edge_ixs[1]])`` (data/mot_graph.py:298-301) without materialising
    the two gathered [E, dim] operands.  Returns [num_edges]."""
    lib = capi.load()
    capi.require_device(emb, edge_ixs)
    emb = capi.f32c(emb)
    ei = edge_ixs.to(torch.int64).contiguous()
    e = ei.shape[1]
    out = torch.empty(e, dtype=torch.float32, device=emb.device)
    check(lib.mpnhip_pairwise_distance(ptr(emb), emb.shape[1], emb.shape[1], ptr(ei), e, C.c_float(float(eps)), ptr(out),
                                       stream_ptr()), "mpnhip_pairwise_distance")
    return out


@capi.on_tensor_device
def construct_graph(det_df, reid_embeddings, fps, max_frame_dist, edge_feats_to_use, top_k_nns=None, reciprocal_k_nns=True,
                    inference_mode=True):
    """``MOTGraph._get_edge_ixs`` + ``construct_graph_object`` (data/mot_graph.py:195-317) for precomputed embeddings.

    Returns ``dict(edge_index [2, 2P] int64, edge_attr [2P, F], reid_emb_dists [2P, 1])``: the pairs followed by the
    flipped pairs, features duplicated and NOT sign-flipped, exactly as ``mot_graph.py:311-315`` builds them.  In
    training mode (``inference_mode=False``) the kNN pruning happens here (``:206-216``), in inference per window."""
    frames = _col(det_df, 'frame', torch.int64, reid_embeddings.device)
    edge_ixs = get_time_valid_conn_ixs(frames, max_frame_dist)
    if not inference_mode and top_k_nns is not None:
        d = pairwise_distance(reid_embeddings, edge_ixs)
        keep = get_knn_mask(d, edge_ixs, frames.numel(), top_k_nns, reciprocal_k_nns=reciprocal_k_nns, symmetric_edges=False)
        kept, _ = compact(keep.to(torch.uint8))
        edge_ixs = gather_edges(edge_ixs, kept, 0)   # edge_ixs.T[k_nns_mask].T (mot_graph.py:216)
    feats = compute_edge_feats_dict(edge_ixs, det_df, fps)
    cols = [feats[name] for name in edge_feats_to_use if name in feats]
    edge_feats = torch.stack(cols).T if cols else torch.empty((edge_ixs.shape[1], 0), device=edge_ixs.device)
    emb_dists = pairwise_distance(reid_embeddings, edge_ixs).view(-1, 1)
    if 'emb_dist' in edge_feats_to_use:
        edge_feats = torch.cat((edge_feats, emb_dists), dim=1)
    return dict(edge_index=torch.cat((edge_ixs, torch.stack((edge_ixs[1], edge_ixs[0]))), dim=1),
                edge_attr=torch.cat((edge_feats, edge_feats), dim=0),
                reid_emb_dists=torch.cat((emb_dists, emb_dists)))


LABEL_MODES = {'all': 0, 'closest': 1}   # MPNHIP_LABELS_* (include/mpnhip.h); dataset_params['true_edge_labels']


@capi.on_tensor_device
def assign_edge_labels(edge_index, ids, mode='closest', validate=True):
    """``MOTGraph.assign_edge_labels`` (data/mot_graph.py:223-262): float32 ``[E]`` on the device from ``edge_index`` (int64
    [2, E]) and the track id of every node (``graph_df.id``: tensor, array or pandas column; -1 = no track).

    ``'all'``: every edge between two detections of one track.  ``'closest'``: of those, per node only the edge to the nearest
    later and the one to the nearest earlier detection that it HAS an edge to (the reference's ``scatter_min`` over
    ``|row - col|``, taken over the edges that survived the kNN pruning).  Stored duplicates of an active edge are all
    labelled; a self loop is labelled under ``'all'`` only.

    ``validate=True`` reads one device flag and raises ``IndexError`` when an endpoint lies outside ``[0, len(ids))``, as the
    reference's gather would; ``validate=False`` reads nothing back (such an edge gets label 0)."""
    if mode not in LABEL_MODES:
        raise MpnhipError("assign_edge_labels: unknown mode %r ('all' or 'closest')" % (mode,))
    capi.require_device(edge_index)
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise MpnhipError("edge_index must be int64 [2, E] (reference data/mot_graph.py:312)")
    lib = capi.load()
    dev = edge_index.device
    ei = edge_index.contiguous()
    if isinstance(ids, torch.Tensor):
        node_ids = ids.to(device=dev, dtype=torch.int64).contiguous().view(-1)
    else:
        node_ids = _col({'id': ids}, 'id', torch.int64, dev).view(-1)
    e, n = ei.shape[1], node_ids.numel()
    labels = torch.empty(e, dtype=torch.float32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    ws = capi.workspace(lib.mpnhip_edge_labels_workspace_bytes(n), dev, "labels")
    check(lib.mpnhip_edge_labels(ptr(ei), e, ptr(node_ids), n, LABEL_MODES[mode], ptr(labels), ptr(flag), ptr(ws), ws.numel(),
                                 stream_ptr()), "mpnhip_edge_labels")
    if validate and e and int(flag.item()) != 0:
        raise IndexError("index out of range in edge_index: entries must lie in [0, %d) (reference mot_graph.py:230 gathers "
                         "ids[edge_index])" % n)
    return labels


def assign_mask_labels(det_df, seq_info_dict, gt_dir=None):
    """``MOTGraph.assign_mask_labels`` (data/mot_graph.py:264-281): the stored ground-truth RoI masks and the flags of the
    detections that have one, selected on the device.  Returns ``(mask_labels [N, 1, H, W], mask_gt_ixs bool [N])``."""
    import os.path as osp
    from .embeddings import load_precomputed_embeddings
    gt_dir = osp.join('gt', 'gt_mask') if gt_dir is None else gt_dir
    mask_labels = load_precomputed_embeddings(det_df=det_df, seq_info_dict=seq_info_dict, embeddings_dir=osp.join(gt_dir, 'masks'),
                                              embedding_dim='3D')
    mask_gt_ixs = load_precomputed_embeddings(det_df=det_df, seq_info_dict=seq_info_dict,
                                              embeddings_dir=osp.join(gt_dir, 'valid_ixs'))
    return mask_labels, mask_gt_ixs.view(-1).bool()


@capi.on_tensor_device
def merge_undirected(edge_index, attrs=(), num_nodes=None):
    """Functional form of ``to_undirected_graph`` (utils/graph.py:176-186).  ``edge_index`` [2, E] lists every pair in both
    directions; ``attrs``: float tensors [E].  Returns ``(edge_index_u [2, E / 2] int64, [attr_u ...], inverse [E] int32)``:
    the pairs with row < col in lexicographic order (``torch.unique(dim=1)``'s columns), per attribute the mean over each
    pair's directed copies (summed in ascending edge id: the same bits on every call, and for two copies the reference's
    ``(a + b) / 2``), and the reference's ``orig_indices``.  ``num_nodes`` (optional; every id must be below it) limits the
    bits the sort looks at.  Raises like the reference's assertion when E != 2 U."""
    lib = capi.load()
    capi.require_device(edge_index, *attrs)
    dev = edge_index.device
    ei = edge_index.to(torch.int64).contiguous()
    E = ei.shape[1]
    attrs = [capi.f32c(a).view(-1) for a in attrs]
    for a in attrs:
        assert a.numel() == E, "one attribute value per directed edge"
    inverse = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = capi.workspace(lib.mpnhip_undirected_merge_workspace_bytes(E), dev, "undirected")
    check(lib.mpnhip_undirected_merge_sort(ptr(ei), E, 0 if num_nodes is None else int(num_nodes), ptr(inverse), ptr(count), ptr(ws),
                                           ws.numel(), stream_ptr()), "mpnhip_undirected_merge_sort")
    U = int(count.item())  # the one host read: sizes the outputs and serves the reference's check
    if E != 2 * U:
        raise MpnhipError("Some edges were not duplicated (%d directed edges, %d distinct pairs)" % (E, U))
    ei_u = torch.empty((2, U), dtype=torch.int64, device=dev)
    outs = [torch.empty(U, dtype=torch.float32, device=dev) for _ in attrs]
    for i in range(max(len(attrs), 1)):
        a, o = (attrs[i], outs[i]) if attrs else (None, None)
        check(lib.mpnhip_undirected_merge_fill(E, U, ptr(ws), ws.numel(), ptr(ei_u) if i == 0 else None, ptr(a), ptr(o),
                                               stream_ptr()), "mpnhip_undirected_merge_fill")
    return ei_u, outs, inverse


@capi.on_tensor_device
def prune_edges(edge_index, edge_preds, threshold=0.5):
    """Functional form of the pruning in ``to_lightweight_graph`` (utils/graph.py:204-207): the edges with
    ``edge_preds >= threshold`` (NaN is dropped, as in torch).  Returns ``(edge_index_kept [2, K], edge_preds_kept [K],
    kept_ids [K] int32)``."""
    lib = capi.load()
    capi.require_device(edge_index, edge_preds)
    ei = edge_index.to(torch.int64).contiguous()
    p = capi.f32c(edge_preds).view(-1)
    n = p.numel()
    assert ei.shape[1] == n, "one score per edge"
    if n == 0:
        return ei, p, torch.empty(0, dtype=torch.int32, device=p.device)
    flags = torch.empty(n, dtype=torch.uint8, device=p.device)
    check(lib.mpnhip_threshold_flags(ptr(p), n, C.c_float(float(threshold)), ptr(flags), stream_ptr()), "mpnhip_threshold_flags")
    kept, _ = compact(flags)
    return gather_edges(ei, kept, 0), gather_rows(p.view(-1, 1), kept).view(-1), kept


def to_undirected_graph(mot_graph, attrs_to_update=('edge_preds', 'edge_labels')):
    """utils/graph.py:165-186, in place on ``mot_graph.graph_obj``: every pair of directed edges (i, j) / (j, i) becomes one
    edge with i < j; the attributes in ``attrs_to_update`` that the graph has become the mean over the pair.  Returns the
    inverse map (the reference's local ``orig_indices``) for callers that want it."""
    g = mot_graph.graph_obj
    names = [a for a in attrs_to_update if hasattr(g, a)]
    ei_u, outs, inverse = merge_undirected(g.edge_index, [getattr(g, a) for a in names])
    g.edge_index = ei_u
    for a, o in zip(names, outs):
        setattr(g, a, o)
    return inverse


def to_lightweight_graph(mot_graph, attrs_to_del=('reid_emb_dists', 'x', 'edge_attr', 'edge_labels')):
    """utils/graph.py:188-207, in place on ``mot_graph.graph_obj``: ``node_names = arange(num_nodes)``, the attributes in
    ``attrs_to_del`` are deleted, and only the edges with ``edge_preds >= 0.5`` stay."""
    g = mot_graph.graph_obj
    n = int(g.num_nodes)
    try:
        g.num_nodes = n   # (pins the count before ``x`` goes, graph.py:196; containers without a setter keep deriving it)
    except AttributeError:
        pass
    g.node_names = torch.arange(n, device=g.edge_index.device)
    for a in attrs_to_del:
        if hasattr(g, a):
            delattr(g, a)
    g.edge_index, g.edge_preds, _ = prune_edges(g.edge_index, g.edge_preds, 0.5)
