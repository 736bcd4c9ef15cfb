"""Training batches on the device: ``MOTGraphDataset.__getitem__`` (reference ``data/mot_graph_dataset.py:185-247``) and the
``DataLoader``'s collation for a whole batch of windows at once, over the C ABI (``csrc/train_batch.hip``).

The sequences stay resident on the device (``SequenceStore``); the host decides which rows make each graph and draws the
random numbers (``dataset.py``: a few thousand integers per sequence); one ``build_batch`` call turns ``batch_size`` such
samples into what ``TrainStep`` takes -- a block-diagonal batch in the order of a PyG ``Batch`` of reference graphs.  There is
no CPU fallback.

======================================  =====================================================================
reference, per sample                   here, per batch
======================================  =====================================================================
``_compute_seq_step_sizes``             ``dataset.seq_step_size`` (host)
``_index_dataset``                      ``dataset.index_dataset`` (host, once)
``_construct_graph_df``                 ``dataset.window_rows`` (host: row indices only)
``MOTGraphAugmentor`` draws             ``dataset.draw_augmentation`` (host: positions and ``eps``)
``_wiggle_boxes`` + its IoU assertion   ``mpnhip_augment_boxes`` (gather, wiggle, min IoU) + one flag read
``get_time_valid_conn_ixs``             ``mpnhip_batch_pairs_count`` / ``_fill``
``F.pairwise_distance``, edge features  ``mpnhip_batch_edge_features`` (per-graph fps)
``get_knn_mask``                        ``mpnhip_knn_mask`` over the batch graph + ``mpnhip_compact``
``construct_graph_object`` + collation  ``mpnhip_batch_edge_layout``
``assign_edge_labels``                  ``graph.assign_edge_labels`` over the batch graph
``_load_appearance_data``, mask labels  ``graph.gather_rows`` of the stores' tensors
======================================  =====================================================================
"""
import ctypes as C

import numpy as np
import torch

from . import capi, dataset
from .capi import MpnhipError, check, ptr, stream_ptr
from .graph import EDGE_FEAT_NAMES, assign_edge_labels, compact, gather_rows

BOX_COLUMNS = ('bb_left', 'bb_top', 'bb_right', 'bb_bot', 'bb_width', 'bb_height', 'feet_x', 'feet_y')   # MPNHIP_BOX_COLS


def _np(det_df, name, dtype):
    v = det_df[name]
    v = v.values if hasattr(v, "values") else v
    if isinstance(v, torch.Tensor):
        v = v.cpu().numpy()
    return np.ascontiguousarray(np.asarray(v), dtype=dtype)


class SequenceStore:
    """One processed sequence, resident on the device: the box columns (float64 ``[R, 8]``, ``BOX_COLUMNS``), ``frame`` and
    ``id`` (int64), and in the table's row order the ReID embeddings, ``x``, ``x_ext``, ``mask_labels`` and ``mask_gt_ixs``.
    The host keeps ``frame``, ``id`` and ``detection_id`` (numpy) for the sampler, and ``fps`` / ``step_size``."""

    def __init__(self, det_df, fps, step_size, reid, x, x_ext=None, mask_labels=None, mask_gt_ixs=None, device=None):
        if not torch.cuda.is_available():
            raise MpnhipError("mpntrackseg_amd.train_batch needs a HIP device; there is no CPU fallback")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.fps, self.step_size = float(fps), int(step_size)
        self.frame = _np(det_df, 'frame', np.int64)
        self.id = _np(det_df, 'id', np.int64)
        self.detection_id = _np(det_df, 'detection_id', np.int64)
        n = self.frame.size
        self.boxes = torch.from_numpy(np.stack([_np(det_df, c, np.float64) for c in BOX_COLUMNS], axis=1)).to(dev)
        self.frame_dev = torch.from_numpy(self.frame).to(dev)
        self.id_dev = torch.from_numpy(self.id).to(dev)

        def rows(t, what):
            if t is None:
                return None
            t = torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()
            if t.shape[0] != n:
                raise MpnhipError("SequenceStore: %s has %d rows, the table %d" % (what, t.shape[0], n))
            return t
        self.reid, self.x, self.x_ext = rows(reid, "reid"), rows(x, "x"), rows(x_ext, "x_ext")
        self.mask_labels, self.mask_gt_ixs = rows(mask_labels, "mask_labels"), rows(mask_gt_ixs, "mask_gt_ixs")
        if self.reid is None or self.x is None:
            raise MpnhipError("SequenceStore: the ReID embeddings and x are required")

    def __len__(self):
        return int(self.frame.size)

    @classmethod
    def from_files(cls, det_df, seq_info_dict, dataset_params, device=None):
        """The tensors from the sequence's embedding files, as ``MOTGraph._load_appearance_data`` / ``assign_mask_labels``
        (data/mot_graph.py:153-193, 264-281) load them per graph -- here once, for the whole table (rows sorted by frame and
        ``detection_id``, the files' order).  ``seq_info_dict`` needs ``fps``, ``step_size``, ``seq_path``, ``det_file_name``."""
        import os.path as osp
        from .embeddings import load_precomputed_embeddings
        from .graph import assign_mask_labels
        emb_dir = osp.join('embeddings', seq_info_dict['det_file_name'])
        load = lambda d, dim: load_precomputed_embeddings(det_df=det_df, seq_info_dict=seq_info_dict, embeddings_dir=osp.join(emb_dir, d),
                                                          embedding_dim=dim)
        reid = load(dataset_params['reid_embeddings_dir'], '1D')
        same = dataset_params['reid_embeddings_dir'] == dataset_params['node_core_embeddings_dir']
        x = reid.clone() if same else load(dataset_params['node_core_embeddings_dir'], '3D')
        x_ext = load(dataset_params['node_ext_embeddings_dir'], '3D')
        mask_labels, mask_gt_ixs = assign_mask_labels(det_df, seq_info_dict)
        return cls(det_df, seq_info_dict['fps'], seq_info_dict['step_size'], reid, x, x_ext, mask_labels, mask_gt_ixs.float(), device)


class StoreSet:
    """The stores' tables one after the other, so that one launch spans sequences: node_src = row offset of the store + row.
    Built once per set of stores (``TrainingBatches`` keeps it; ``build_batch`` given a list keeps the last one)."""

    TENSORS = ('reid', 'x', 'x_ext', 'mask_labels', 'mask_gt_ixs')

    def __init__(self, stores):
        self.stores = list(stores)
        if not self.stores:
            raise MpnhipError("StoreSet: no stores")
        self.device = self.stores[0].device
        self.offsets = np.concatenate(([0], np.cumsum([len(s) for s in self.stores]))).astype(np.int64)
        if self.offsets[-1] >= 2 ** 31:
            raise MpnhipError("StoreSet: 2^31 rows or more are not supported")
        one = len(self.stores) == 1
        cat = lambda name: getattr(self.stores[0], name) if one else torch.cat([getattr(s, name) for s in self.stores], dim=0)
        self.boxes, self.frame, self.id = cat('boxes'), cat('frame_dev'), cat('id_dev')
        for name in self.TENSORS:
            have = [getattr(s, name) is not None for s in self.stores]
            if any(have) and not all(have):
                raise MpnhipError("StoreSet: %s is given for some sequences only" % name)
            setattr(self, name, cat(name) if all(have) else None)


_last_set = [None]


def _store_set(stores):
    if isinstance(stores, StoreSet):
        return stores
    stores = list(stores)
    last = _last_set[0]
    if last is None or len(last.stores) != len(stores) or any(a is not b for a, b in zip(last.stores, stores)):
        last = _last_set[0] = StoreSet(stores)
    return last


def attr_columns(edge_feats_to_use):
    """The columns of ``edge_attr`` as ``construct_graph_object`` orders them (data/mot_graph.py:295-307): the geometric features
    in the order of ``edge_feats_to_use``, then the embedding distance if it is named."""
    cols = [EDGE_FEAT_NAMES.index(n) for n in edge_feats_to_use if n in EDGE_FEAT_NAMES]
    return cols + ([len(EDGE_FEAT_NAMES)] if 'emb_dist' in edge_feats_to_use else [])


def augment_boxes(store_set, node_src, graph_ptr, eps=None):
    """``mpnhip_augment_boxes``: gather and wiggle.  ``node_src`` (int32) and ``graph_ptr`` (int32 ``[B + 1]``): numpy, on the
    host; ``eps``: numpy float64 ``[N, 4]`` or None.  Returns a dict of device tensors: ``boxes [N, 8]`` float64, ``cols [N, 4]``
    float32 (bb_height, bb_width, feet_x, feet_y), ``frame``, ``id`` (int64), ``node_graph``, ``graph_ptr`` (int32),
    ``node_src`` (int32), ``min_iou`` (float64 ``[1]``), ``bad_rows`` (int32 ``[1]``).  Nothing is read back."""
    lib = capi.load()
    dev = store_set.device
    node_src = np.ascontiguousarray(node_src, dtype=np.int32)
    graph_ptr = np.ascontiguousarray(graph_ptr, dtype=np.int32)
    n, b = int(node_src.size), int(graph_ptr.size) - 1
    with torch.cuda.device(dev):
        src_dev = torch.from_numpy(node_src).to(dev)
        eps_dev = None
        if eps is not None:
            eps = np.ascontiguousarray(eps, dtype=np.float64)
            if eps.shape != (n, 4):
                raise MpnhipError("augment_boxes: eps must be [N, 4] (%s for %d nodes)" % (eps.shape, n))
            eps_dev = torch.from_numpy(eps).to(dev)
        out = dict(boxes=torch.empty((n, len(BOX_COLUMNS)), dtype=torch.float64, device=dev),
                   cols=torch.empty((n, 4), dtype=torch.float32, device=dev), frame=torch.empty(n, dtype=torch.int64, device=dev),
                   id=torch.empty(n, dtype=torch.int64, device=dev), node_graph=torch.empty(n, dtype=torch.int32, device=dev),
                   graph_ptr=torch.empty(b + 1, dtype=torch.int32, device=dev), node_src=src_dev,
                   min_iou=torch.empty(1, dtype=torch.float64, device=dev), bad_rows=torch.empty(1, dtype=torch.int32, device=dev))
        ws = capi.workspace(lib.mpnhip_augment_boxes_workspace_bytes(), dev, "augment")
        check(lib.mpnhip_augment_boxes(ptr(store_set.boxes), ptr(store_set.frame), ptr(store_set.id), store_set.boxes.shape[0], ptr(src_dev),
                                       graph_ptr.ctypes.data_as(C.c_void_p), b, ptr(eps_dev), n, ptr(out['boxes']), ptr(out['cols']),
                                       ptr(out['frame']), ptr(out['id']), ptr(out['node_graph']), ptr(out['graph_ptr']),
                                       ptr(out['min_iou']), ptr(out['bad_rows']), ptr(ws), ws.numel(), stream_ptr()), "mpnhip_augment_boxes")
    return out


def batch_pairs(frame, node_graph, graph_ptr, max_frame_dist):
    """``get_time_valid_conn_ixs`` inside every graph of the batch: int64 ``[2, P]``, batch-global node indices."""
    lib = capi.load()
    dev = frame.device
    n, b = frame.numel(), graph_ptr.numel() - 1
    if n == 0:
        return torch.empty((2, 0), dtype=torch.int64, device=dev)
    maxd = -1 if max_frame_dist == 'max' else int(max_frame_dist)
    with torch.cuda.device(dev):
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ws = capi.workspace(lib.mpnhip_batch_pairs_workspace_bytes(n), dev, "batch_pairs")
        check(lib.mpnhip_batch_pairs_count(ptr(frame), ptr(node_graph), ptr(graph_ptr), b, n, maxd, ptr(offsets), ptr(ws), ws.numel(),
                                           stream_ptr()), "mpnhip_batch_pairs_count")
        n_pairs = int(offsets[n].item())   # host read 1 of build_batch: the pair count sizes everything per pair
        out = torch.empty((2, n_pairs), dtype=torch.int64, device=dev)
        check(lib.mpnhip_batch_pairs_fill(ptr(frame), ptr(node_graph), ptr(graph_ptr), b, n, maxd, ptr(offsets), n_pairs, ptr(out),
                                          stream_ptr()), "mpnhip_batch_pairs_fill")
    return out


def batch_edge_features(pairs, frame, node_graph, fps, cols, emb, eps=1e-6):
    """``mpnhip_batch_edge_features``: ``(feats [P, 5], emb_dist [P])`` with ``fps [B]`` (float32, device), one per graph."""
    lib = capi.load()
    dev = pairs.device
    p = pairs.shape[1]
    feats = torch.empty((p, 5), dtype=torch.float32, device=dev)
    dist = torch.empty(p, dtype=torch.float32, device=dev)
    emb2 = emb.view(emb.shape[0], -1)
    with torch.cuda.device(dev):
        check(lib.mpnhip_batch_edge_features(ptr(pairs), p, frame.numel(), ptr(frame), ptr(node_graph), ptr(fps), fps.numel(), ptr(cols),
                                             ptr(emb2), emb2.shape[1], emb2.shape[1], C.c_float(float(eps)), ptr(feats), ptr(dist),
                                             stream_ptr()), "mpnhip_batch_edge_features")
    return feats, dist


def batch_edge_layout(pairs, kept, n_kept, node_graph, n_graphs, feats, dist, attr_cols):
    """``mpnhip_batch_edge_layout``: ``(edge_index [2, 2K] int64, edge_attr [2K, F], edge_graph [2K] int32)``; ``kept`` None = all."""
    lib = capi.load()
    dev = pairs.device
    f = len(attr_cols)
    edge_index = torch.empty((2, 2 * n_kept), dtype=torch.int64, device=dev)
    edge_attr = torch.empty((2 * n_kept, f), dtype=torch.float32, device=dev)
    edge_graph = torch.empty(2 * n_kept, dtype=torch.int32, device=dev)
    cols = (C.c_int32 * max(f, 1))(*attr_cols)
    with torch.cuda.device(dev):
        ws = capi.workspace(lib.mpnhip_batch_edge_layout_workspace_bytes(n_graphs), dev, "batch_layout")
        check(lib.mpnhip_batch_edge_layout(ptr(pairs), pairs.shape[1], ptr(kept), n_kept, ptr(node_graph), node_graph.numel(), n_graphs,
                                           ptr(feats), ptr(dist), cols, f, ptr(edge_index), ptr(edge_attr), ptr(edge_graph), ptr(ws),
                                           ws.numel(), stream_ptr()), "mpnhip_batch_edge_layout")
    return edge_index, edge_attr, edge_graph


def _gather(t, ids):
    if t is None:
        return None
    return gather_rows(t, ids).view((ids.numel(),) + tuple(t.shape[1:]))


def build_batch(stores, samples, dataset_params):
    """One training batch from ``samples``: a list of ``(store index, rows, eps)`` -- ``rows`` the table rows of the graph's
    nodes in graph order (``dataset.window_rows`` after ``dataset.draw_augmentation``'s drops), ``eps`` float64 ``[n, 4]`` or None
    for an unaugmented sample (all samples of a batch alike).  ``stores``: a list of ``SequenceStore`` or a ``StoreSet``.

    Returns a dict of device tensors: ``x``, ``x_ext``, ``edge_index`` (int64 ``[2, E]``, batch-global), ``edge_attr``,
    ``edge_labels``, ``mask_labels``, ``mask_gt_ixs`` (bool), ``edge_graph`` / ``node_graph`` (int32), ``n_graphs``, ``graph_ptr``
    (int32 ``[B + 1]``) -- the PyG ``Batch`` of the reference's per-sample graphs, each graph's pairs followed by its flipped
    pairs -- and for inspection ``boxes`` (the augmented float64 columns, ``BOX_COLUMNS``), ``frame``, ``id``, ``min_iou``.

    Raises ``AssertionError`` where the reference's ``assert iou_val.min() >= min_iou`` (augmentation.py:86) fails for any
    graph.  At most three host reads: the pair count, the kept count, and that flag at the end."""
    ss = _store_set(stores)
    dev = ss.device
    samples = list(samples)
    b = len(samples)
    with_eps = [s[2] is not None for s in samples]
    if any(with_eps) and not all(with_eps):
        raise MpnhipError("build_batch: augmented and unaugmented samples in one batch")
    rows = [np.asarray(s[1], dtype=np.int64).reshape(-1) for s in samples]
    for (si, _, _), r in zip(samples, rows):
        if not 0 <= si < len(ss.stores) or (r.size and (r.min() < 0 or r.max() >= len(ss.stores[si]))):
            raise MpnhipError("build_batch: a sample names a store or a row that does not exist")
    node_src = np.concatenate([r + ss.offsets[s[0]] for s, r in zip(samples, rows)]) if b else np.zeros(0, np.int64)
    graph_ptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int32)
    eps = np.concatenate([np.asarray(s[2], np.float64).reshape(-1, 4) for s in samples]) if b and all(with_eps) else None
    n = int(node_src.size)
    nodes = augment_boxes(ss, node_src, graph_ptr, eps)
    with torch.cuda.device(dev):
        fps = torch.tensor([ss.stores[s[0]].fps for s in samples], dtype=torch.float32).to(dev)
        emb = _gather(ss.reid, nodes['node_src'])
        pairs = batch_pairs(nodes['frame'], nodes['node_graph'], nodes['graph_ptr'], dataset_params['max_frame_dist'])
        feats, dist = batch_edge_features(pairs, nodes['frame'], nodes['node_graph'], fps, nodes['cols'], emb)
        kept, n_kept = None, pairs.shape[1]
        if dataset_params['top_k_nns'] is not None and n_kept:
            from .graph import get_knn_mask
            keep = get_knn_mask(dist, pairs, n, dataset_params['top_k_nns'], reciprocal_k_nns=dataset_params['reciprocal_k_nns'],
                                symmetric_edges=False)                       # training: one direction per pair (mot_graph.py:210-218)
            kept, n_kept = compact(keep.to(torch.uint8))                     # host read 2: the kept count sizes the edge tensors
        edge_index, edge_attr, edge_graph = batch_edge_layout(pairs, kept, n_kept, nodes['node_graph'], b, feats, dist,
                                                              attr_columns(dataset_params['edge_feats_to_use']))
        labels = assign_edge_labels(edge_index, nodes['id'], dataset_params.get('true_edge_labels', 'closest'), validate=False)
        gt = _gather(ss.mask_gt_ixs, nodes['node_src'])
        out = dict(x=_gather(ss.x, nodes['node_src']), x_ext=_gather(ss.x_ext, nodes['node_src']), edge_index=edge_index, edge_attr=edge_attr,
                   edge_labels=labels, mask_labels=_gather(ss.mask_labels, nodes['node_src']),
                   mask_gt_ixs=None if gt is None else gt.view(-1) != 0, edge_graph=edge_graph, node_graph=nodes['node_graph'],
                   n_graphs=b, graph_ptr=nodes['graph_ptr'], boxes=nodes['boxes'], frame=nodes['frame'], id=nodes['id'],
                   min_iou=nodes['min_iou'])
        if eps is not None and n:
            # host read 3, where the batch is handed over: the reference's assertion (augmentation.py:86) over all graphs at once
            min_iou = float(nodes['min_iou'].item())
            assert min_iou >= dataset_params['min_iou_bb_wiggling'], \
                "a wiggled box has IoU %r with its original, below min_iou_bb_wiggling" % (min_iou,)
    return out


class TrainingBatches:
    """The reference's ``MOTGraphDataset`` + ``DataLoader`` over device-resident sequences: iterating yields ``build_batch``
    dicts of ``batch_size`` graphs (the last one may be smaller).

    ``rng``: a ``numpy.random.RandomState``; it permutes the samples when ``shuffle`` and supplies every draw of the
    augmentation (``dataset.draw_augmentation``: the reference's calls in the reference's order).  ``len()`` is the number of
    batches; ``n_samples`` the reference's dataset length; ``self[i]`` is sample ``i`` as a batch of one."""

    def __init__(self, stores, dataset_params, batch_size=8, mode='train', rng=None, shuffle=None):
        assert mode in ('train', 'val', 'test')     # mot_graph_dataset.py:22
        self.set = _store_set(stores)
        self.dataset_params = dataset_params
        self.batch_size = int(batch_size)
        self.mode = mode
        self.rng = rng if rng is not None else np.random.RandomState()
        self.shuffle = (mode == 'train') if shuffle is None else bool(shuffle)
        # _index_dataset (mot_graph_dataset.py:146-183): (store, start frame), sequence by sequence
        self.index = [(si, int(f)) for si, s in enumerate(self.set.stores)
                      for f in dataset.index_dataset(s.frame, s.step_size, dataset_params['frames_per_graph'], dataset_params['min_detects'])]

    @property
    def n_samples(self):
        return len(self.index)

    def __len__(self):
        return (len(self.index) + self.batch_size - 1) // self.batch_size

    def sample(self, i):
        """The host part of ``get_from_frame_and_seq`` for sample ``i``: ``(store index, rows, eps)``."""
        si, start = self.index[i]
        s, p = self.set.stores[si], self.dataset_params
        step = dataset.draw_step_size(self.rng, s.step_size, p, self.mode)
        rows = dataset.window_rows(s.frame, s.detection_id, start, step, p['frames_per_graph'], p['max_detects'])
        _, kept, eps = dataset.draw_augmentation(self.rng, s.id[rows], step, p, self.mode, draw_step=False)
        if eps is not None and kept.size == 0:
            # (the reference's iou_val.min() of no box, augmentation.py:86)
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        return si, rows[kept], eps

    def __getitem__(self, i):
        return build_batch(self.set, [self.sample(i)], self.dataset_params)

    def __iter__(self):
        order = self.rng.permutation(len(self.index)) if self.shuffle else np.arange(len(self.index))
        for k in range(0, len(order), self.batch_size):
            yield build_batch(self.set, [self.sample(int(i)) for i in order[k:k + self.batch_size]], self.dataset_params)
