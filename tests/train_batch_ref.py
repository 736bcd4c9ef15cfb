"""numpy restatement of the device operators of ``csrc/train_batch.hip`` (TEST INFRASTRUCTURE): wiggle + IoU, pairs inside the
graphs of a batch, edge features with a per-graph fps, the kNN pruning over the batch graph, and the PyG-``Batch`` layout.
``tests/test_train_batch_cpu.py`` pins it to the reference's own samples (tests/golden/g25_train_samples.npz); the GPU tests
compare the kernels with it where they do not compare with the reference directly."""
import numpy as np

from training_targets_ref import edge_labels

BOX_COLUMNS = ('bb_left', 'bb_top', 'bb_right', 'bb_bot', 'bb_width', 'bb_height', 'feet_x', 'feet_y')
LEFT, TOP, RIGHT, BOT, W, H, FX, FY = range(8)
EDGE_FEAT_NAMES = ('secs_time_dists', 'norm_feet_x_dists', 'norm_feet_y_dists', 'bb_height_dists', 'bb_width_dists')


def iou_pairs(a, b):
    """utils/iou.py:33-59 for boxes ``[n, 4]`` = left, top, right, bot (float64)."""
    xA, yA = np.maximum(a[:, 0], b[:, 0]), np.maximum(a[:, 1], b[:, 1])
    xB, yB = np.minimum(a[:, 2], b[:, 2]), np.minimum(a[:, 3], b[:, 3])
    inter = np.maximum(0, xB - xA + 1) * np.maximum(0, yB - yA + 1)
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    area_b = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    return inter / (area_a + area_b - inter)


def augment_boxes(boxes, node_src, eps):
    """``(out_boxes [N, 8] float64, cols [N, 4] float32, min_iou)``: augmentation.py:71-86 on the rows ``node_src`` of ``boxes``
    (``[R, 8]``, ``BOX_COLUMNS``); ``eps`` None: the rows as they are, min_iou = inf."""
    b = np.array(boxes, np.float64)[np.asarray(node_src, np.int64)]
    min_iou = np.inf
    if eps is not None:
        old = b.copy()
        eps = np.asarray(eps, np.float64).reshape(-1, 4)
        b[:, TOP] = old[:, TOP] + old[:, H] * eps[:, 0]
        b[:, BOT] = old[:, BOT] + old[:, H] * eps[:, 1]
        b[:, LEFT] = old[:, LEFT] + old[:, W] * eps[:, 2]
        b[:, RIGHT] = old[:, RIGHT] + old[:, W] * eps[:, 3]
        b[:, H] = b[:, BOT] - b[:, TOP]
        b[:, W] = b[:, RIGHT] - b[:, LEFT]
        if b.shape[0]:
            min_iou = iou_pairs(b[:, :4], old[:, :4]).min()
    cols = b[:, [H, W, FX, FY]].astype(np.float32)
    return b, cols, min_iou


def batch_pairs(frame, graph_ptr, max_frame_dist):
    """int64 ``[2, P]``: per graph the pairs of utils/graph.py:6-37 (ascending row, then col), node offsets added."""
    frame = np.asarray(frame, np.int64)
    out = []
    for g in range(len(graph_ptr) - 1):
        f = frame[graph_ptr[g]:graph_ptr[g + 1]]
        d = np.abs(f.reshape(-1, 1) - f.reshape(1, -1))
        cond = d > 0
        if max_frame_dist != 'max':
            cond &= d <= max_frame_dist
        row, col = np.nonzero(cond)
        m = row < col
        out.append(np.stack((row[m], col[m])) + graph_ptr[g])
    return np.concatenate(out, axis=1).astype(np.int64) if out else np.zeros((2, 0), np.int64)


def batch_edge_features(pairs, frame, node_graph, fps, cols, emb, eps=1e-6):
    """``(feats [P, 5], emb_dist [P])`` in float32, one rounded operation at a time (utils/graph.py:104-122, F.pairwise_distance)."""
    r, c = pairs
    f32 = np.float32
    t = np.asarray(frame).astype(f32) / np.asarray(fps, f32)[np.asarray(node_graph)]
    h, w, fx, fy = (cols[:, i] for i in range(4))
    mean_h = (h[r] + h[c]) / f32(2)
    feats = np.stack([t[c] - t[r], (fx[c] - fx[r]) / mean_h, (fy[c] - fy[r]) / mean_h, np.log(h[c] / h[r]), np.log(w[c] / w[r])],
                     axis=1).astype(f32)
    d = emb[r].astype(f32) - emb[c].astype(f32) + f32(eps)
    return feats.reshape(-1, 5), np.sqrt((d * d).sum(axis=1, dtype=f32)).astype(f32)


def knn_mask(dist, pairs, n_nodes, top_k, reciprocal):
    """utils/graph.py:40-87 with ``symmetric_edges=False``; ties in distance rank by column (a stable argsort)."""
    dm = np.full((n_nodes, n_nodes), np.inf, np.float32)
    dm[pairs[0], pairs[1]] = dist
    dm[pairs[1], pairs[0]] = dist
    order = np.argsort(dm, axis=1, kind='stable')
    ranking = np.zeros((n_nodes, n_nodes), np.int64)
    ranking[np.arange(n_nodes).reshape(-1, 1), order] = np.arange(n_nodes).reshape(1, -1)
    in_k = ranking < top_k
    in_k = (in_k & in_k.T) if reciprocal else (in_k | in_k.T)
    return in_k[pairs[0], pairs[1]]


def batch_edge_layout(pairs, kept, node_graph, n_graphs, feats, dist, attr_cols):
    """``(edge_index [2, 2K], edge_attr [2K, F], edge_graph [2K])``: per graph its kept pairs, then its flipped pairs."""
    pairs = pairs[:, kept]
    table = np.concatenate((feats, dist.reshape(-1, 1)), axis=1)[kept][:, attr_cols]
    g_of = np.asarray(node_graph)[pairs[0]] if pairs.shape[1] else np.zeros(0, np.int64)
    ei, ea, eg = [], [], []
    for g in range(n_graphs):
        sel = g_of == g
        p = pairs[:, sel]
        ei += [p, p[::-1]]
        ea += [table[sel], table[sel]]
        eg.append(np.full(2 * p.shape[1], g, np.int32))
    if not ei:
        return np.zeros((2, 0), np.int64), np.zeros((0, len(attr_cols)), np.float32), np.zeros(0, np.int32)
    return np.concatenate(ei, axis=1).astype(np.int64), np.concatenate(ea).astype(np.float32), np.concatenate(eg)


def attr_columns(edge_feats_to_use):
    cols = [EDGE_FEAT_NAMES.index(n) for n in edge_feats_to_use if n in EDGE_FEAT_NAMES]
    return cols + ([5] if 'emb_dist' in edge_feats_to_use else [])


SEQS = ("A", "B")
N_TRAIN, N_SAMPLES = 6, 8   # g25: six augmented 'train' samples, then two 'val' samples


def fixture(z):
    """``(params, tables, samples)`` of g25_train_samples.npz: the dataset_params of tools/make_golden_train_batch.py, per sequence
    its table (``boxes [R, 8]``, ``frame``, ``id``, ``detection_id``, ``reid``, ``x``, ``fps``, ``mov_camera``, ``step_size``) and per
    recorded sample a dict: ``seed, seq, start, train, step_size, rows`` (table rows, graph order), ``eps`` (None: 'val')."""
    params = {k: z[f"params:{k}"].item() for k in ("frames_per_graph", "max_detects", "min_detects", "max_frame_dist", "top_k_nns",
                                                   "p_change_fps_step", "min_ids_to_drop_perc", "max_ids_to_drop_perc",
                                                   "min_detects_to_drop_perc", "max_detects_to_drop_perc", "min_iou_bb_wiggling")}
    params.update(reciprocal_k_nns=bool(z["params:reciprocal_k_nns"]), edge_feats_to_use=list(EDGE_FEAT_NAMES) + ["emb_dist"],
                  true_edge_labels="closest", augment=True,
                  target_fps_dict={"moving": int(z["params:target_fps"][0]), "static": int(z["params:target_fps"][1])})
    tables = []
    for n in SEQS:
        fps, mov, step = (int(v) for v in z[f"{n}:info"])
        det = z[f"{n}:detection_id"]
        assert np.array_equal(np.sort(det), np.arange(det.size))
        tables.append(dict(boxes=np.stack([z[f"{n}:{c}"] for c in BOX_COLUMNS], axis=1), frame=z[f"{n}:frame"], id=z[f"{n}:id"],
                           detection_id=det, reid=z[f"{n}:reid"][det], x=z[f"{n}:x"][det], fps=fps, mov_camera=bool(mov), step_size=step,
                           row_of=np.argsort(det)))
    samples = []
    for k in range(N_SAMPLES):
        seed, seq, start, train = (int(v) for v in z[f"s{k}:args"])
        samples.append(dict(seed=seed, seq=seq, start=start, train=bool(train), step_size=int(z[f"s{k}:step_size"]),
                            rows=tables[seq]["row_of"][z[f"s{k}:detection_id"]], eps=z[f"s{k}:eps"] if train else None))
    return params, tables, samples


def build_batch(tables, samples, params):
    """``tables``: per sequence a dict with ``boxes [R, 8]``, ``frame``, ``id``, ``reid``, ``fps``; ``samples``: (table, rows, eps)."""
    ptr = np.concatenate(([0], np.cumsum([len(s[1]) for s in samples]))).astype(np.int64)
    b = len(samples)
    node_graph = np.repeat(np.arange(b), np.diff(ptr))
    parts = [augment_boxes(tables[t]['boxes'], rows, eps) for t, rows, eps in samples]
    boxes = np.concatenate([p[0] for p in parts])
    cols = np.concatenate([p[1] for p in parts])
    min_iou = min([p[2] for p in parts] + [np.inf])
    cat = lambda name: np.concatenate([np.asarray(tables[t][name])[np.asarray(rows, np.int64)] for t, rows, _ in samples])
    frame, ids, emb = cat('frame'), cat('id'), cat('reid')
    fps = np.array([tables[t]['fps'] for t, _, _ in samples], np.float32)
    pairs = batch_pairs(frame, ptr, params['max_frame_dist'])
    feats, dist = batch_edge_features(pairs, frame, node_graph, fps, cols, emb)
    kept = np.arange(pairs.shape[1])
    if params['top_k_nns'] is not None and pairs.shape[1]:
        kept = np.nonzero(knn_mask(dist, pairs, len(frame), params['top_k_nns'], params['reciprocal_k_nns']))[0]
    ei, ea, eg = batch_edge_layout(pairs, kept, node_graph, b, feats, dist, attr_columns(params['edge_feats_to_use']))
    return dict(boxes=boxes, cols=cols, min_iou=min_iou, frame=frame, id=ids, edge_index=ei, edge_attr=ea, edge_graph=eg,
                edge_labels=edge_labels(ei, ids, params['true_edge_labels']), node_graph=node_graph.astype(np.int32),
                graph_ptr=ptr.astype(np.int32))
