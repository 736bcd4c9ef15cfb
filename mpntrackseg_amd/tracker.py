"""Sliding-window inference over a whole sequence graph: host mirror of ``MPNTracker._predict_edges_and_masks`` and
``MPNTracker._evaluate_graph_in_batches`` (reference ``src/mot_neural_solver/tracker/mpn_tracker.py:96-210``) over the C
ABI -- SURVEY.md section 8 row f-3.

Every window of ``frames_per_graph`` consecutive frames becomes a sub-graph (window selection, per-window kNN pruning,
compaction: ``csrc/tracker.hip``), runs through the hot path (``mpnhip_forward``), and its edge probabilities are
added into the sequence-level accumulators on the device; the result is the per-edge average over the windows an edge
appeared in.  Windows are independent, so several can be evaluated in ONE forward as a block-diagonal graph
(``windows_per_launch``; the sub-graphs do not interact, ``tests/test_gpu_parity.py::test_batched_graphs``), and they
shard round-robin over ranks (``rank`` / ``world_size``) with one final sum of the two accumulators.

``evaluate_sequence`` goes on to the end of ``_evaluate_graph_in_batches`` (``:199-210``): the mask branch of every window
(``MOTMPNet.mask_predictions``, the mask head for the last step only) is accumulated per node and averaged over the windows a
node was in (``node_preds``; a node that was in no window is 0 / 0 = NaN as in the reference, which zeroes NaN for edges
only), the directed scores are merged into one score per undirected pair (``graph.merge_undirected``) and the pairs below
``prune_threshold`` are dropped (``graph.prune_edges``) -- the object the reference hands to its projectors, built on the
device.  ``evaluate_graph_in_batches`` stays the directed edge scores alone.

``track_sequence`` adds the next three lines of ``MPNTracker.track``: the projection of the scores onto trajectories
(``_project_graph_model_output``, ``projectors.py`` here: greedy rounding on the device, or the exact rounding whose linear
program runs on the host), ``assign_ped_ids`` (``_assign_ped_ids``, ``:231-248``: connected components of the rounded graph, a
lock-free union-find in ``csrc/projection.hip``) and ``drop_short_trajectories`` (``tracker/postprocessing.py:14-18``) --
detections in, track ids out.

``to_full_masks`` and ``save_results_to_file`` are the last two steps (``_to_full_masks``, ``:267-298``, and ``save_results_to_file``,
``:398-417``): the RoI masks of the surviving detections are pasted into their frames, made disjoint and thresholded on the device
(``masks.py``, ``csrc/full_masks.hip``: one label per pixel instead of one image per detection), leave it as run boundaries and
become COCO run-length strings on the host (or, with ``strings='device'``, on the device: ``csrc/rle_codec.hip``); the text file
has the MOTS challenge's rows.  ``mots_sequence`` is ``track_sequence`` followed by ``to_full_masks``: detections in, MOTS rows out.  What stays in the reference needs files of its
detector (``_add_tracktor_detects``, and the data-frame work of ``_predict_nan_masks`` around its network call, which is
``rcnn_heads.nan_roi_masks``), or is commented out there (the trajectory interpolation)."""
import collections
import types

import numpy as np
import torch

from . import capi
from .capi import MpnhipError, check, ptr, stream_ptr
from .graph import get_knn_mask, compact as _compact, gather_rows as _gather_rows, gather_edges as _gather_edges


@capi.on_tensor_device
def window_subgraph(edge_index, edge_attr, reid_emb_dists, node_begin, node_end, top_k_nns, reciprocal_k_nns, node_offset=0):
    """Edges of the window [node_begin, node_end) after kNN pruning (mpn_tracker.py:171-178 and :107-112).
    Returns ``(sub_edge_index [2, K] (local ids + node_offset), sub_edge_attr [K, F], window_ids [W] int32, kept_ids [K] int32)``."""
    lib = capi.load()
    E = edge_index.shape[1]
    flags = torch.empty(max(E, 1), dtype=torch.uint8, device=edge_index.device)[:E]
    check(lib.mpnhip_window_flags(ptr(edge_index), E, int(node_begin), int(node_end), ptr(flags), stream_ptr()),
          "mpnhip_window_flags")
    win_ids, n_win = _compact(flags)
    sub_ei = _gather_edges(edge_index, win_ids, node_begin)
    sub_dist = _gather_rows(reid_emb_dists.view(-1, 1), win_ids)
    keep = get_knn_mask(sub_dist, sub_ei, node_end - node_begin, top_k_nns, reciprocal_k_nns=reciprocal_k_nns,
                        symmetric_edges=True)
    kept_ids, _ = _compact(keep.to(torch.uint8))
    sub_ei_k = _gather_edges(sub_ei, kept_ids, -int(node_offset))
    sub_attr = _gather_rows(_gather_rows(edge_attr, win_ids), kept_ids)
    return sub_ei_k, sub_attr, win_ids, kept_ids


def frame_windows(frame_num_per_node, frames_per_graph):
    """Node ranges of the sliding windows (mpn_tracker.py:166-169): detections are ordered by frame, window w spans
    the w-th .. (w + frames_per_graph - 1)-th distinct frame."""
    f = np.asarray(frame_num_per_node.cpu() if isinstance(frame_num_per_node, torch.Tensor) else frame_num_per_node)
    if f.size and (np.diff(f) < 0).any():
        raise MpnhipError("detections must be ordered by frame (MOTGraph sorts them, data/mot_graph.py:145)")
    all_frames = np.unique(f)
    out = []
    for start, end in zip(all_frames, all_frames[frames_per_graph - 1:]):
        out.append((int(np.searchsorted(f, start, side="left")), int(np.searchsorted(f, end, side="right"))))
    return out


@torch.no_grad()
@capi.on_tensor_device
def evaluate_graph_in_batches(model, x, edge_index, edge_attr, reid_emb_dists, frame_num_per_node, frames_per_graph,
                              top_k_nns, reciprocal_k_nns=True, set_pruned_edges_to_inactive=False, windows_per_launch=1,
                              rank=0, world_size=1, reduce_fn=None):
    """``_evaluate_graph_in_batches`` for the edge scores: returns ``final_edge_preds`` [num_edges] of the full graph.

    ``x`` [N, node_in_dim] are the pooled node inputs of the WHOLE sequence (detections ordered by frame), ``edge_index``
    / ``edge_attr`` / ``reid_emb_dists`` its symmetric edge list as ``graph.construct_graph`` builds it.
    ``reduce_fn(tensor)`` sums a tensor over ranks in place (e.g. ``torch.distributed.all_reduce``) when the windows
    are sharded (``rank``, ``world_size``)."""
    capi.require_device(x, edge_index, edge_attr, reid_emb_dists)
    # the weights do not change during one sequence: pack their images once for all its windows
    with model.frozen_weights():
        return _evaluate_windows(model, x, edge_index, edge_attr, reid_emb_dists, frame_num_per_node, frames_per_graph, top_k_nns,
                                 reciprocal_k_nns, set_pruned_edges_to_inactive, windows_per_launch, rank, world_size, reduce_fn)[0]


SequenceResult = collections.namedtuple('SequenceResult', ['final_edge_preds', 'edge_index', 'edge_preds', 'node_preds'])


@torch.no_grad()
@capi.on_tensor_device
def evaluate_sequence(model, x, edge_index, edge_attr, reid_emb_dists, frame_num_per_node, frames_per_graph, top_k_nns,
                      reciprocal_k_nns=True, set_pruned_edges_to_inactive=False, windows_per_launch=1, rank=0, world_size=1,
                      reduce_fn=None, x_ext=None, prune_threshold=0.5):
    """``_evaluate_graph_in_batches`` to its end (mpn_tracker.py:143-210).  Arguments as ``evaluate_graph_in_batches``, plus
    ``x_ext`` [N, C, h, w] (the RoI features of the mask branch; optional) and ``prune_threshold``.  Returns a
    ``SequenceResult``:

    ``final_edge_preds`` [E]         directed, what ``evaluate_graph_in_batches`` returns for the same arguments
    ``edge_index`` [2, K], ``edge_preds`` [K]   undirected (row < col, lexicographic) and pruned at ``prune_threshold``
    ``node_preds`` [N, 1, H, W]      averaged mask probabilities; ``None`` without a mask branch or without ``x_ext``

    With ``rank`` / ``world_size`` the node accumulators are summed by ``reduce_fn`` like the edge accumulators."""
    capi.require_device(x, edge_index, edge_attr, reid_emb_dists, x_ext)
    from .graph import merge_undirected, prune_edges
    if not getattr(model, 'has_mask_branch', False):
        x_ext = None
    with model.frozen_weights():
        final, node_preds = _evaluate_windows(model, x, edge_index, edge_attr, reid_emb_dists, frame_num_per_node, frames_per_graph,
                                              top_k_nns, reciprocal_k_nns, set_pruned_edges_to_inactive, windows_per_launch, rank,
                                              world_size, reduce_fn, x_ext=x_ext)
    ei_u, (preds_u,), _ = merge_undirected(edge_index, [final], num_nodes=x.shape[0])
    ei_k, preds_k, _ = prune_edges(ei_u, preds_u, prune_threshold)
    return SequenceResult(final, ei_k, preds_k, node_preds)


def _accumulate_node_masks(model, x_ext_b, ei_b, logits, group, node_acc):
    """The mask branch of one launch (one window, or several as a block-diagonal batch: the attention aggregation and the
    mask head run once; the holder lets the attention steps share one prepared graph), then one accumulation per window:
    windows overlap in nodes, the stream orders the launches."""
    lib = capi.load()
    masks = model.mask_predictions(x_ext_b, ei_b, logits, holder=types.SimpleNamespace(), last_only=True)[-1]   # mpn_tracker.py:132
    masks = capi.f32c(masks)
    row_len = int(masks[0].numel())
    if node_acc[0] is None:   # the spatial size of the masks is the model's to say
        N = node_acc[2]
        node_acc[0] = torch.zeros((N,) + tuple(masks.shape[1:]), dtype=torch.float32, device=masks.device)
        node_acc[1] = torch.zeros(max(N, 1), dtype=torch.float32, device=masks.device)[:N]
    r0 = 0
    for (n0, n1) in group:
        check(lib.mpnhip_node_mask_accumulate(ptr(masks[r0:r0 + (n1 - n0)]), n1 - n0, row_len, n0, node_acc[2], ptr(node_acc[0]),
                                              ptr(node_acc[1]), stream_ptr()), "mpnhip_node_mask_accumulate")
        r0 += n1 - n0


def _evaluate_windows(model, x, edge_index, edge_attr, reid_emb_dists, frame_num_per_node, frames_per_graph, top_k_nns,
                      reciprocal_k_nns, set_pruned_edges_to_inactive, windows_per_launch, rank, world_size, reduce_fn, x_ext=None):
    """The window loop.  Returns ``(final_edge_preds, node_preds)``; ``node_preds`` is None unless ``x_ext`` is given."""
    lib = capi.load()
    edge_index = edge_index.to(torch.int64).contiguous()
    x = capi.f32c(x)
    E = edge_index.shape[1]
    overall_preds = torch.zeros(max(E, 1), dtype=torch.float32, device=x.device)[:E]
    overall_num = torch.zeros(max(E, 1), dtype=torch.float32, device=x.device)[:E]
    windows = frame_windows(frame_num_per_node, frames_per_graph)[rank::world_size]
    L = max(int(model.num_enc_steps), 1)
    node_acc = [None, None, int(x.shape[0])]   # overall_node_preds, overall_num_node_preds (allocated by the first window), N
    for g0 in range(0, len(windows), max(int(windows_per_launch), 1)):
        group = windows[g0:g0 + max(int(windows_per_launch), 1)]
        parts, node_off = [], 0
        for (n0, n1) in group:
            ei_k, attr_k, win_ids, kept_ids = window_subgraph(edge_index, edge_attr, reid_emb_dists, n0, n1, top_k_nns,
                                                              reciprocal_k_nns, node_offset=node_off)
            parts.append((ei_k, attr_k, win_ids, kept_ids, n0, n1))
            node_off += n1 - n0
        if len(parts) == 1:
            ei_b, attr_b, x_b = parts[0][0], parts[0][1], x[parts[0][4]:parts[0][5]]
        else:
            ei_b = torch.cat([p[0] for p in parts], dim=1)
            attr_b = torch.cat([p[1] for p in parts], dim=0)
            x_b = torch.cat([x[p[4]:p[5]] for p in parts], dim=0)
        if ei_b.shape[1] > 0:
            # (the window's indices were built here, inside [0, n): no error-flag read-back, the host keeps running ahead)
            all_logits = model.hot_path(x_b, ei_b, attr_b, validate=False)
            logits = all_logits[L - 1]  # classified_edges[-1] (mpn_tracker.py:132)
        else:
            logits = torch.empty(0, dtype=torch.float32, device=x.device)
        if x_ext is not None:
            all_logits = all_logits if ei_b.shape[1] > 0 else torch.empty((L, 0), dtype=torch.float32, device=x.device)
            x_ext_b = x_ext[group[0][0]:group[0][1]] if len(group) == 1 else torch.cat([x_ext[n0:n1] for (n0, n1) in group], dim=0)
            _accumulate_node_masks(model, x_ext_b, ei_b, all_logits, group, node_acc)
        e_off = 0
        for (ei_k, attr_k, win_ids, kept_ids, n0, n1) in parts:
            k = kept_ids.numel()
            lg = logits[e_off:e_off + k]
            check(lib.mpnhip_window_accumulate(ptr(lg) if k else None, ptr(kept_ids) if k else None, k, ptr(win_ids),
                                               win_ids.numel(), 1 if set_pruned_edges_to_inactive else 0, ptr(overall_preds),
                                               ptr(overall_num), stream_ptr()), "mpnhip_window_accumulate")
            e_off += k
    if reduce_fn is not None and world_size > 1:
        reduce_fn(overall_preds)
        reduce_fn(overall_num)
    final = torch.empty_like(overall_preds)
    check(lib.mpnhip_average_preds(ptr(overall_preds), ptr(overall_num), E, ptr(final), stream_ptr()), "mpnhip_average_preds")
    if x_ext is None:
        return final, None
    return final, _average_node_masks(model, x_ext, node_acc, reduce_fn if world_size > 1 else None)


def _average_node_masks(model, x_ext, node_acc, reduce_fn):
    """final_node_preds = overall_node_preds / overall_num_node_preds (mpn_tracker.py:209-210)."""
    lib = capi.load()
    N = node_acc[2]
    if node_acc[0] is None:
        # this rank evaluated no window: the accumulators are zeros of the shape the mask head gives
        hw = _mask_output_size(model, x_ext)
        node_acc[0] = torch.zeros((N, 1) + hw, dtype=torch.float32, device=x_ext.device)
        node_acc[1] = torch.zeros(max(N, 1), dtype=torch.float32, device=x_ext.device)[:N]
    if reduce_fn is not None:
        reduce_fn(node_acc[0])
        reduce_fn(node_acc[1])
    out = torch.empty_like(node_acc[0])
    row_len = int(node_acc[0][0].numel()) if N else 0
    check(lib.mpnhip_node_mask_average(ptr(node_acc[0]), ptr(node_acc[1]), N, row_len, ptr(out), stream_ptr()),
          "mpnhip_node_mask_average")
    return out


def _mask_output_size(model, x_ext):
    """(H, W) of ``model.mask_predictor``'s output for RoI features of ``x_ext``'s size, from its convolutions' geometry."""
    mm = model.mask_predictor
    hw = [int(x_ext.shape[2]), int(x_ext.shape[3])]
    for part in (mm.feature_encoder, mm.mask_head, mm.mask_predictor):
        for m in part.modules():
            if isinstance(m, torch.nn.ConvTranspose2d):
                hw = [(v - 1) * m.stride[i] - 2 * m.padding[i] + m.dilation[i] * (m.kernel_size[i] - 1) + m.output_padding[i] + 1
                      for i, v in enumerate(hw)]
            elif isinstance(m, torch.nn.Conv2d):
                hw = [(v + 2 * m.padding[i] - m.dilation[i] * (m.kernel_size[i] - 1) - 1) // m.stride[i] + 1 for i, v in enumerate(hw)]
    return tuple(hw)


@capi.on_tensor_device
def assign_ped_ids(edge_index, edge_preds, num_nodes):
    """``MPNTracker._assign_ped_ids`` (mpn_tracker.py:231-248): int64 [num_nodes] labels of the connected components over the edges
    with ``edge_preds == 1``, numbered as ``scipy.sparse.csgraph.connected_components(directed=False)`` numbers them (by smallest
    node).  Any undirected edge list; no host read."""
    lib = capi.load()
    capi.require_device(edge_index, edge_preds)
    ei = edge_index.to(torch.int64).contiguous()
    p = capi.f32c(edge_preds).view(-1)
    K, N, dev = ei.shape[1], int(num_nodes), ei.device
    if p.numel() != K:
        raise MpnhipError("one score per edge (%d scores, %d edges)" % (p.numel(), K))
    labels = torch.empty(max(N, 1), dtype=torch.int64, device=dev)[:N]
    ws = capi.workspace(lib.mpnhip_connected_components_workspace_bytes(N), dev, "components")
    check(lib.mpnhip_connected_components(ptr(ei), K, N, ptr(p), ptr(labels), None, ptr(ws), ws.numel(), stream_ptr()),
          "mpnhip_connected_components")
    return labels


@capi.on_tensor_device
def drop_short_trajectories(ped_ids, min_track_len):
    """``Postprocessor.drop_short_trajectories`` (tracker/postprocessing.py:14-18) as a mask: bool [N], True for the detections
    whose id occurs at least ``min_track_len`` times.  The ids are not renumbered, as in the reference."""
    lib = capi.load()
    capi.require_device(ped_ids)
    labels = ped_ids.to(torch.int64).contiguous().view(-1)
    N = labels.numel()
    counts = torch.empty(max(N, 1), dtype=torch.int32, device=labels.device)[:N]
    keep = torch.empty(max(N, 1), dtype=torch.uint8, device=labels.device)[:N]
    check(lib.mpnhip_track_lengths(ptr(labels), N, int(min_track_len), ptr(counts), ptr(keep), stream_ptr()), "mpnhip_track_lengths")
    return keep.bool()


TrackResult = collections.namedtuple('TrackResult', ['ped_ids', 'keep', 'edge_index', 'edge_preds', 'node_preds', 'constr_satisf_rate',
                                                     'final_edge_preds'])


@capi.on_tensor_device
def track_sequence(model, x, edge_index, edge_attr, reid_emb_dists, frame_num_per_node, frames_per_graph, top_k_nns,
                   reciprocal_k_nns=True, set_pruned_edges_to_inactive=False, windows_per_launch=1, rank=0, world_size=1,
                   reduce_fn=None, x_ext=None, prune_threshold=0.5, rounding_method='greedy', min_track_len=2, solver=None):
    """``evaluate_sequence``, then ``_project_graph_model_output``, ``_assign_ped_ids`` and ``drop_short_trajectories``
    (mpn_tracker.py:212-248, postprocessing.py:14-18).  Arguments as ``evaluate_sequence``, plus ``rounding_method`` ('greedy' or
    'exact'), ``min_track_len`` and ``solver`` (for 'exact': None, a callable or 'device', see ``projectors.exact_round``).  Returns a
    ``TrackResult``:

    ``ped_ids`` [N] int64            track id of every detection
    ``keep`` [N] bool                False for the detections of tracks shorter than ``min_track_len``
    ``edge_index`` [2, K], ``edge_preds`` [K]   ``evaluate_sequence``'s undirected pruned list with the ROUNDED scores
    ``node_preds``, ``final_edge_preds``        as ``evaluate_sequence`` returns them
    ``constr_satisf_rate``           share of the flow constraints the thresholded scores satisfied before the rounding

    With 'greedy' this adds one host read (the two constraint counters) to ``evaluate_sequence``'s; with 'exact' and
    ``solver='device'`` two (those counters with the sizes of the assignment problems, and the assignment's status), and the
    pipeline stays on the device from the windows to the track ids."""
    from . import projectors
    if rounding_method not in ('greedy', 'exact'):
        raise RuntimeError("Rounding type for projector not understood")
    if rounding_method == 'exact':
        projectors.check_solver(solver)
    seq = evaluate_sequence(model, x, edge_index, edge_attr, reid_emb_dists, frame_num_per_node, frames_per_graph, top_k_nns,
                            reciprocal_k_nns=reciprocal_k_nns, set_pruned_edges_to_inactive=set_pruned_edges_to_inactive,
                            windows_per_launch=windows_per_launch, rank=rank, world_size=world_size, reduce_fn=reduce_fn, x_ext=x_ext,
                            prune_threshold=prune_threshold)
    N = int(x.shape[0])
    if rounding_method == 'greedy':
        rounded, rate = projectors.greedy_round(seq.edge_index, seq.edge_preds, N)
    else:
        rounded, rate = projectors.exact_round(seq.edge_index, seq.edge_preds, N, solver=solver)
    ped_ids = assign_ped_ids(seq.edge_index, rounded, N)
    keep = drop_short_trajectories(ped_ids, min_track_len)
    return TrackResult(ped_ids, keep, seq.edge_index, rounded, seq.node_preds, rate, seq.final_edge_preds)


@capi.on_tensor_device
def to_full_masks(node_preds, boxes, frame_num_per_node, keep, img_shape, mask_threshold=0.5, frames_per_launch=8, strings='host'):
    """``MPNTracker._to_full_masks`` (mpn_tracker.py:267-298): an object array [N] with the COCO run-length string of every kept
    detection's full-frame mask (``None`` for the dropped ones).  Per frame: ``paste_masks_in_image`` of the kept detections' RoI
    masks in node order, ``ensure_unique_masks``, ``>= mask_threshold``, ``rletools.encode`` -- see ``masks.py``.

    ``node_preds`` [N, 1, mh, mw] (device), ``boxes`` [N, 4] (left, top, right, bottom), ``frame_num_per_node`` [N], ``keep`` [N]
    bool, ``img_shape`` = (H, W).  The kept detections are grouped by frame with a stable sort (the identity for frame-ordered
    nodes) and ``frames_per_launch`` frames share a launch: the label workspace is 4 B x H x W x frames_per_launch, and the result
    does not depend on it.  Host reads: ``keep`` once, then per launch the number of run boundaries and the boundaries.

    ``strings``: 'host' turns the boundaries into strings one detection at a time in numpy (``masks.rle_string``); 'device' encodes
    all strings of a launch on the device (``masks.mask_run_strings``) and reads the finished bytes instead of the boundaries.
    The strings are the same."""
    from . import masks as M
    if strings not in ('host', 'device'):
        raise MpnhipError("strings must be 'host' or 'device' (%r)" % (strings,))
    capi.require_device(node_preds)
    N = int(node_preds.shape[0])
    H, W = int(img_shape[0]), int(img_shape[1])
    as_np = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v).reshape(-1)
    keep_h, frame_h = as_np(keep).astype(bool), as_np(frame_num_per_node)
    if keep_h.size != N or frame_h.size != N or len(boxes) != N:
        raise MpnhipError("one box, frame number and keep flag per detection (%d detections)" % N)
    out = np.full(N, None, dtype=object)
    kept = np.flatnonzero(keep_h)
    kept = kept[np.argsort(frame_h[kept], kind="stable")]
    if kept.size == 0:
        return out
    _, first, per_frame = np.unique(frame_h[kept], return_index=True, return_counts=True)
    step = max(int(frames_per_launch), 1)
    for g0 in range(0, first.size, step):
        cnt = per_frame[g0:g0 + step]
        ids = kept[first[g0]:first[g0] + int(cnt.sum())]
        frame_ptr = np.concatenate(([0], np.cumsum(cnt)))
        labels = M.paste_unique_masks(node_preds, boxes, frame_ptr, (H, W), mask_threshold, det_ids=ids)
        if strings == 'device':
            for node, s in zip(ids, M.rle_strings(*M.mask_run_strings(labels, ids.size))):
                out[node] = s
            continue
        pos, counts = M.mask_run_events(labels, ids.size)
        ends = np.cumsum(counts)
        for j, node in enumerate(ids):
            out[node] = M.rle_string(M.rle_counts_from_events(pos[ends[j] - counts[j]:ends[j]], H * W))
    return out


def save_results_to_file(path, frame, ped_ids, label, img_shape, rles, keep):
    """``MPNTracker.save_results_to_file`` (mpn_tracker.py:398-417) without its date-stamped second copy: one row
    ``frame id label img_height img_width rle`` per kept detection, space-separated, no header, sorted by (frame, id), where
    id = ped_id + label * 1000 + 1 (the MOTS id format).  ``label`` is one class id or one per detection; returns the rows."""
    as_np = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)
    frame, ped = as_np(frame).reshape(-1).astype(np.int64), as_np(ped_ids).reshape(-1).astype(np.int64)
    keep = as_np(keep).reshape(-1).astype(bool)
    lab = np.broadcast_to(as_np(label).astype(np.int64).reshape(-1), ped.shape) if np.ndim(as_np(label)) else np.full(ped.shape, int(label), np.int64)
    if not (frame.size == ped.size == keep.size == len(rles)):
        raise MpnhipError("one frame, id, keep flag and run-length string per detection")
    ids = ped + lab * 1000 + 1
    sel = np.flatnonzero(keep)
    sel = sel[np.lexsort((ids[sel], frame[sel]))]
    rows = []
    for i in sel:
        if rles[i] is None:
            raise MpnhipError("detection %d is kept but has no mask" % int(i))
        rows.append("%d %d %d %d %d %s" % (frame[i], ids[i], lab[i], int(img_shape[0]), int(img_shape[1]), rles[i]))
    with open(path, "w") as fh:
        fh.write("".join(r + "\n" for r in rows))
    return rows


@capi.on_tensor_device
def mots_sequence(model, x, edge_index, edge_attr, reid_emb_dists, frame_num_per_node, frames_per_graph, top_k_nns, x_ext, boxes,
                  img_shape, mask_threshold=0.5, frames_per_launch=8, strings='host', **track_args):
    """``track_sequence`` (``track_args``: its remaining keyword arguments), then ``to_full_masks`` (``strings``: its argument):
    ``(TrackResult, rles)``."""
    res = track_sequence(model, x, edge_index, edge_attr, reid_emb_dists, frame_num_per_node, frames_per_graph, top_k_nns, x_ext=x_ext,
                         **track_args)
    if res.node_preds is None:
        raise MpnhipError("mots_sequence needs the mask branch: a model with one and the RoI features x_ext")
    rles = to_full_masks(res.node_preds, boxes, frame_num_per_node, res.keep, img_shape, mask_threshold=mask_threshold,
                         frames_per_launch=frames_per_launch, strings=strings)
    return res, rles


@capi.on_tensor_device
def evaluate_mots_sequence(node_preds, boxes, frame_num_per_node, ped_ids, label, keep, img_shape, gt, seq_length, mask_threshold=0.5,
                           frames_per_launch=8, class_id=2, ignore_class=10, details=False):
    """The MOTS metrics (``compute_mots_metrics``, utils/evaluation.py:87-102) of a tracked sequence against the ground truth
    ``gt`` (a MOTS text file, or what ``mots_eval.load_mots_txt`` returns) over the frames ``0 .. seq_length``: what
    ``mots_eval.evaluate_mots_files`` gives for the rows ``save_results_to_file`` writes for the same arguments, without the
    run-length strings and the text file -- per launch the prediction's label images come straight from
    ``masks.paste_unique_masks`` (every kept detection pastes, as in ``to_full_masks``) and go into the overlap kernel.

    ``node_preds``, ``boxes``, ``frame_num_per_node``, ``keep``, ``img_shape``, ``mask_threshold``, ``frames_per_launch`` as
    ``to_full_masks``; ``ped_ids`` and ``label`` as ``save_results_to_file``: a detection's trajectory is its MOTS id
    ``ped_id + label * 1000 + 1``, and only the detections with ``label == class_id`` are scored.  Returns the dict of
    ``mots_eval.metrics_from_matches``."""
    from . import masks as M, mots_eval as ME
    capi.require_device(node_preds)
    N = int(node_preds.shape[0])
    as_np = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)
    keep_h, frame_h = as_np(keep).reshape(-1).astype(bool), as_np(frame_num_per_node).reshape(-1).astype(np.int64)
    ped = as_np(ped_ids).reshape(-1).astype(np.int64)
    lab = np.broadcast_to(as_np(label).astype(np.int64).reshape(-1), ped.shape) if np.ndim(as_np(label)) else np.full(ped.shape, int(label), np.int64)
    if not (keep_h.size == frame_h.size == ped.size == N == len(boxes)):
        raise MpnhipError("one box, frame number, id and keep flag per detection (%d detections)" % N)
    kept = np.flatnonzero(keep_h)
    kept = kept[np.argsort(frame_h[kept], kind="stable")]
    ids = ped[kept] + lab[kept] * 1000 + 1
    if np.unique(np.stack((frame_h[kept], ids)), axis=1).shape[1] != kept.size:
        raise ValueError("Multiple objects with one track id in a frame")
    scored = lab[kept] == class_id
    traj_ids = np.unique(ids[scored])
    b_traj = np.where(scored, np.searchsorted(traj_ids, ids), -1).astype(np.int64)

    def b_labels(frames, b_ptr, b_entries, hw):
        return M.paste_unique_masks(node_preds, boxes, b_ptr, img_shape, mask_threshold, det_ids=kept[b_entries])
    return ME._evaluate(ME._as_loaded(gt), seq_length, class_id, ignore_class, frames_per_launch, node_preds.device, frame_h[kept], b_traj,
                        traj_ids, b_labels, img_shape, details)


def _pasted_b_side(node_preds, boxes, frame_num_per_node, ped_ids, label, keep, img_shape, mask_threshold):
    """The prediction side of ``hota_eval._pass1`` from a tracked sequence's pasted label images: ``b_side(class_id)`` ->
    (b_frame, b_traj, b_ids, b_labels, img_shape).  Every kept detection pastes; those with ``label == class_id`` are scored."""
    from . import masks as M
    capi.require_device(node_preds)
    N = int(node_preds.shape[0])
    as_np = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)
    keep_h, frame_h = as_np(keep).reshape(-1).astype(bool), as_np(frame_num_per_node).reshape(-1).astype(np.int64)
    ped = as_np(ped_ids).reshape(-1).astype(np.int64)
    lab = np.broadcast_to(as_np(label).astype(np.int64).reshape(-1), ped.shape) if np.ndim(as_np(label)) else np.full(ped.shape, int(label), np.int64)
    if not (keep_h.size == frame_h.size == ped.size == N == len(boxes)):
        raise MpnhipError("one box, frame number, id and keep flag per detection (%d detections)" % N)
    kept = np.flatnonzero(keep_h)
    kept = kept[np.argsort(frame_h[kept], kind="stable")]   # node order inside a frame: the paste order of to_full_masks
    ids = ped[kept] + lab[kept] * 1000 + 1
    if np.unique(np.stack((frame_h[kept], ids)), axis=1).shape[1] != kept.size:
        raise ValueError("Multiple objects with one track id in a frame")

    def b_side(class_id):
        scored = lab[kept] == class_id
        traj_ids = np.unique(ids[scored])
        b_traj = np.where(scored, np.searchsorted(traj_ids, ids), -1).astype(np.int64)

        def b_labels(frames, b_ptr, b_entries, hw):
            return M.paste_unique_masks(node_preds, boxes, b_ptr, img_shape, mask_threshold, det_ids=kept[b_entries])
        return frame_h[kept], b_traj, traj_ids, b_labels, img_shape
    return b_side


@capi.on_tensor_device
def evaluate_hota_sequence(node_preds, boxes, frame_num_per_node, ped_ids, label, keep, img_shape, gt, num_timesteps, mask_threshold=0.5,
                           frames_per_launch=8, class_id=2, ignore_class=10, details=False, assignment="host"):
    """HOTA (``eval_kitti_mots``, utils/evaluation.py:127-135) of a tracked KITTI-MOTS sequence against the ground truth ``gt``
    (a MOTS text file, or what ``mots_eval.load_mots_txt`` returns) over the frames ``0 .. num_timesteps - 1``: what
    ``hota_eval.evaluate_hota_files`` gives for the rows ``save_results_to_file`` writes for the same arguments, without the
    run-length strings and the text file -- the twin of ``evaluate_mots_sequence``, with the prediction's label images straight
    from ``masks.paste_unique_masks`` (every kept detection pastes; only those with ``label == class_id`` are scored).

    The arguments as ``evaluate_mots_sequence``, but ``num_timesteps`` frames instead of its ``seq_length + 1``; ``assignment``
    ('host' or 'device') as ``hota_eval.evaluate_hota_files``.  Returns the dict of ``hota_eval.evaluate_hota_files``."""
    from . import hota_eval as HE
    b_frame, b_traj, traj_ids, b_labels, _ = _pasted_b_side(node_preds, boxes, frame_num_per_node, ped_ids, label, keep, img_shape,
                                                            mask_threshold)(class_id)
    return HE._evaluate(HE._as_loaded(gt), num_timesteps, class_id, ignore_class, frames_per_launch, node_preds.device, b_frame,
                        b_traj, traj_ids, b_labels, img_shape, details, assignment=assignment)


@capi.on_tensor_device
def evaluate_kitti_mots_sequence(node_preds, boxes, frame_num_per_node, ped_ids, label, keep, img_shape, gt, num_timesteps, mask_threshold=0.5,
                                 frames_per_launch=8, classes=("car", "pedestrian"), metrics=("HOTA", "CLEAR", "Identity"),
                                 assignment="host"):
    """HOTA, CLEAR, Identity and Count (``TrackEval/scripts/run_kitti_mots.py``'s defaults) of a tracked KITTI-MOTS sequence
    against the ground truth ``gt`` for every class of ``classes``: what ``kitti_mots_eval.evaluate_sequence_files`` gives for the
    rows ``save_results_to_file`` writes for the same arguments, without the run-length strings and the text file -- next to
    ``evaluate_hota_sequence``, whose arguments it takes; a prediction's class is its ``label`` (1 car, 2 pedestrian).  Returns
    ``{cls: {metric: fields}}``."""
    from . import hota_eval as HE, kitti_mots_eval as KE
    b_side = _pasted_b_side(node_preds, boxes, frame_num_per_node, ped_ids, label, keep, img_shape, mask_threshold)
    return KE._evaluate_classes(HE._as_loaded(gt), num_timesteps, classes, metrics, frames_per_launch, node_preds.device, b_side, None,
                                assignment)
