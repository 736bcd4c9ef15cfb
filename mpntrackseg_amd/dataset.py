"""Host side of the training sampler: which windows exist, which rows a window holds and every random draw of one training
sample -- exact restatements of the reference's ``MOTGraphDataset`` (``data/mot_graph_dataset.py``),
``MOTGraph._construct_graph_df`` (``data/mot_graph.py:108-147``) and ``MOTGraphAugmentor`` (``data/augmentation.py``).

numpy only: nothing here reads the device.  The host keeps ``frame``, ``id`` and ``detection_id`` of every sequence (a few
thousand integers); everything that touches boxes, embeddings or edges happens in ``train_batch.py`` on the device."""
import numpy as np


def seq_step_size(fps, mov_camera, target_fps_dict):
    """``MOTGraphDataset._compute_seq_step_sizes`` (mot_graph_dataset.py:97-113) for one sequence: every how many frames a
    sequence recorded at ``fps`` is sampled to reach the target rate of its camera type (Python's ``round``: half to even)."""
    target_fps = target_fps_dict['moving' if mov_camera else 'static']
    if fps <= target_fps:
        return 1
    return round(fps / target_fps)


def index_dataset(frame, step_size, frames_per_graph, min_detects):
    """``MOTGraphDataset._index_dataset`` (mot_graph_dataset.py:146-183) for one sequence: the valid start frames (int64), in the
    reference's order -- residue class ``start_frame in range(step_size)`` by residue class, ascending inside one.

    A populated frame ``f`` of a residue class is valid when ``f <= max_f - (frames_per_graph - 1) * step_size`` (``max_f``: the
    class's last populated frame, :172) and its ``frames_per_graph`` strided frames hold at least ``min_detects`` detections in
    more than one populated frame (:176-180).  The reference loops over the frames with ``isin``; here one prefix sum over the
    class's per-frame counts answers every window."""
    assert isinstance(frames_per_graph, (int, np.integer)) and frames_per_graph > 0     # :156
    assert isinstance(min_detects, (int, np.integer)) and min_detects > 0               # :157
    frame = np.asarray(frame, dtype=np.int64).reshape(-1)
    step = int(step_size)
    out = []
    for start_frame in range(step):
        sel = frame[np.mod(frame - start_frame, step) == 0]                             # :167 (pandas' mod: never negative)
        if sel.size == 0:
            continue                                                                    # (max() is NaN: no f passes :175)
        k = (sel - start_frame) // step                                                 # position inside the class
        k0 = int(k.min())
        counts = np.bincount(k - k0)                                                    # detections per class position (:171)
        n = counts.size
        dets = np.concatenate(([0], np.cumsum(counts)))
        populated = np.concatenate(([0], np.cumsum(counts > 0)))
        first = np.nonzero(counts)[0]                                                   # the populated positions, ascending
        first = first[first <= (n - 1) - (frames_per_graph - 1)]                        # :172, :175
        last = np.minimum(first + frames_per_graph, n)
        ok = (dets[last] - dets[first] >= min_detects) & (populated[last] - populated[first] > 1)   # :179
        out.append((first[ok] + k0) * step + start_frame)
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)


def window_rows(frame, detection_id, start_frame, step_size, frames_per_graph, max_detects, end_frame=None,
                ensure_end_is_in=False):
    """``MOTGraph._construct_graph_df`` (mot_graph.py:108-147): the row indices (int64) of the sequence's table that make the
    graph starting at ``start_frame``, in the graph's order -- sorted by ``(frame, detection_id)`` (:145).

    Without ``end_frame``: the frames ``np.arange(start_frame, frame.max(), step_size)`` -- the sequence's last frame is never
    in (:132) -- cut to the first ``frames_per_graph`` (unless ``'max'``, :135-136), and of their populated frames the prefix
    whose cumulative detection count stays within ``max_detects`` (unless None, :139-142).  With ``end_frame``: every
    ``step_size``-th frame up to and including it, plus ``end_frame`` itself with ``ensure_end_is_in`` (:123-128)."""
    frame = np.asarray(frame, dtype=np.int64).reshape(-1)
    detection_id = np.asarray(detection_id).reshape(-1)
    if end_frame is not None:
        valid_frames = np.arange(start_frame, end_frame + 1, step_size)
        if ensure_end_is_in and (end_frame not in valid_frames):
            valid_frames = np.asarray(valid_frames.tolist() + [end_frame])
    else:
        valid_frames = np.arange(start_frame, frame.max() if frame.size else start_frame, step_size)
        if frames_per_graph != 'max':
            valid_frames = valid_frames[:frames_per_graph]
        if max_detects is not None:
            populated, counts = np.unique(frame[np.isin(frame, valid_frames)], return_counts=True)
            valid_frames = populated[np.cumsum(counts) <= max_detects]
    rows = np.nonzero(np.isin(frame, valid_frames))[0]
    order = np.lexsort((detection_id[rows], frame[rows]))       # sort_values(by=['frame', 'detection_id'])
    return rows[order].astype(np.int64)


def wiggle_max_eps(min_iou):
    """The largest relative shift of a box side (augmentation.py:62-65)."""
    upper_bound_inside_box = (1 - np.sqrt(min_iou)) / 2
    upper_bound_outside_box = 0.5 * (1 / np.sqrt(min_iou) - 1)
    return min(upper_bound_inside_box, upper_bound_outside_box)


def augments(dataset_params, mode):
    """``MOTGraphDataset.augment`` (mot_graph_dataset.py:26)."""
    return bool(dataset_params['augment']) and mode == 'train'


def draw_step_size(rng, step_size, dataset_params, mode):
    """The step-size change of ``get_from_frame_and_seq`` (mot_graph_dataset.py:207-209): one ``rng.rand()`` only if augmenting
    and ``step_size > 1``, a second one only if the first fell below ``p_change_fps_step``."""
    if augments(dataset_params, mode) and step_size > 1:
        if rng.rand() < dataset_params['p_change_fps_step']:
            step_size = np.round(step_size * (0.5 + rng.rand())).astype(int)
    return int(step_size)


def draw_augmentation(rng, ids, step_size, dataset_params, mode, draw_step=True):
    """Every random draw of one training sample, from ``rng`` (a ``numpy.random.RandomState``) with the reference's calls in
    the reference's order, so that ``RandomState(seed)`` gives the sample the reference draws after ``np.random.seed(seed)``.

    ``ids``: the track id of every row of the window (``graph_df.id``), or -- the window depends on the drawn step size -- a
    callable ``ids(step_size)`` that returns them for the step size drawn here.  ``draw_step=False`` skips the step-size draw
    (it was made with ``draw_step_size``).  Returns ``(step_size, kept, eps)``: the new step size, the positions (int64,
    ascending) of the window's rows that survive ``_drop_ids`` and ``_drop_detections``, and ``eps [len(kept), 4]`` (float64)
    for the top, bottom, left and right side of every survivor (``_wiggle_boxes``).  With ``mode != 'train'`` or augmentation
    off nothing is drawn: all positions, ``eps`` None."""
    if draw_step:
        step_size = draw_step_size(rng, step_size, dataset_params, mode)
    if callable(ids):
        ids = ids(step_size)
    ids = np.asarray(ids).reshape(-1)
    if not augments(dataset_params, mode):
        return int(step_size), np.arange(ids.size, dtype=np.int64), None
    # _drop_ids (augmentation.py:13-24).  all_ids is literally the reference's expression: the order of a set of numpy integers
    # is what choice() permutes, so it must be built the same way -- pandas' unique() lists the ids by first appearance
    _, first = np.unique(ids, return_index=True)
    all_ids = list(set(ids[np.sort(first)]) - {-1})
    ids_to_drop_perc = rng.uniform(dataset_params['min_ids_to_drop_perc'], dataset_params['max_ids_to_drop_perc'])
    num_ids_to_drop = np.round(ids_to_drop_perc * len(all_ids)).astype(int)
    ids_to_drop = rng.choice(all_ids, num_ids_to_drop, replace=False)
    kept = np.nonzero(~np.isin(ids, ids_to_drop))[0]
    # _drop_detections (:26-39): positions of the re-indexed table
    all_detects = np.arange(kept.size)
    detects_to_drop_perc = rng.uniform(dataset_params['min_detects_to_drop_perc'], dataset_params['max_detects_to_drop_perc'])
    num_detects_to_drop = np.round(detects_to_drop_perc * len(all_detects)).astype(int)
    detects_to_drop = rng.choice(all_detects, num_detects_to_drop, replace=False)
    kept = np.delete(kept, detects_to_drop)
    # _wiggle_boxes (:62-68)
    max_eps = wiggle_max_eps(dataset_params['min_iou_bb_wiggling'])
    eps = rng.uniform(-max_eps, max_eps, 4 * kept.size).reshape(-1, 4)
    return int(step_size), kept.astype(np.int64), eps
