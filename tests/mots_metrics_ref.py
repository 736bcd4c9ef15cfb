"""numpy restatements of the three operators of ``csrc/mots_eval.hip`` (``mpnhip_paint_label_runs``, ``mpnhip_label_overlap``,
``mpnhip_mots_frame_match``) with the argument contracts of ``include/mpnhip.h``, the same call signatures as the wrappers in
``mpntrackseg_amd/mots_eval.py`` (so that the host side of the evaluation runs over them without a device), and the helpers
the MOTS-metrics tests share: the g22 fixture's id images as MOTS text files and as lists."""
import os

import numpy as np

from mpntrackseg_amd import masks as M
from mpntrackseg_amd.mots_eval import METRIC_NAMES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_mots_metrics.npz")
SCENES = ("cases", "crowded")
LDS_CELLS = 4096   # csrc/mots_eval.hip OV_LDS_CELLS: a frame's table of at most this many cells is counted in LDS


def frame_of(ptr, e):
    """the frame f with ptr[f] <= e < ptr[f + 1], or -1"""
    f = int(np.searchsorted(ptr[:-1], e, "right")) - 1
    return f if f >= 0 and e < ptr[f + 1] else -1


def paint_label_runs(run_entry, run_begin, run_end, frame_ptr, n_entries, hw, device=None):
    ptr = np.asarray(frame_ptr, np.int64).reshape(-1)
    labels = np.full((ptr.size - 1, int(hw)), -1, np.int32)
    for e, b, en in zip(np.asarray(run_entry).reshape(-1), np.asarray(run_begin).reshape(-1), np.asarray(run_end).reshape(-1)):
        if not (0 <= e < n_entries and 0 <= b < en <= hw):
            continue
        f = frame_of(ptr, e)
        if f >= 0:
            labels[f, b:en] = e
    return labels


def table_offsets(a_ptr, b_ptr):
    a, b = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    return np.concatenate(([0], np.cumsum((np.diff(a) + 1) * (np.diff(b) + 1)))).astype(np.int64)


def label_overlap(labels_a, labels_b, a_ptr, b_ptr):
    a_ptr, b_ptr = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    tp = table_offsets(a_ptr, b_ptr)
    table = np.zeros(int(tp[-1]), np.int32)
    F = a_ptr.size - 1
    hw = np.asarray(labels_a).size // F if F else 0
    la, lb = np.asarray(labels_a).reshape(F, hw).astype(np.int64), np.asarray(labels_b).reshape(F, hw).astype(np.int64)
    for f in range(F):
        na, nb = a_ptr[f + 1] - a_ptr[f], b_ptr[f + 1] - b_ptr[f]
        ia, ib = la[f] - a_ptr[f], lb[f] - b_ptr[f]
        ia = np.where((ia >= 0) & (ia < na), ia + 1, 0)
        ib = np.where((ib >= 0) & (ib < nb), ib + 1, 0)
        np.add.at(table, tp[f] + ia * (nb + 1) + ib, 1)
    return table, tp


def frame_match(table, table_ptr, a_ptr, b_ptr, a_ignore, a_traj, b_traj, n_a_traj, n_b_traj):
    a_ptr, b_ptr = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    table = np.asarray(table).astype(np.int64)
    n_a, n_b = int(a_ptr[-1]), int(b_ptr[-1])
    out = {"match_b": np.full(n_a, -1, np.int32), "inter": np.zeros(n_a, np.int32), "uni": np.zeros(n_a, np.int32),
           "b_matched": np.zeros(n_b, bool), "b_ignored": np.zeros(n_b, bool), "b_area": np.zeros(n_b, np.int32),
           "id_match": np.zeros((int(n_a_traj), int(n_b_traj)), np.int32)}
    for f in range(a_ptr.size - 1):
        a0, b0 = int(a_ptr[f]), int(b_ptr[f])
        na, nb = int(a_ptr[f + 1]) - a0, int(b_ptr[f + 1]) - b0
        t = table[table_ptr[f]:table_ptr[f] + (na + 1) * (nb + 1)].reshape(na + 1, nb + 1)
        A, B = t.sum(axis=1), t.sum(axis=0)
        ign = np.asarray(a_ignore[a0:a0 + na]).astype(bool)
        out["b_area"][b0:b0 + nb] = B[1:]
        out["b_ignored"][b0:b0 + nb] = 2 * t[1:][ign].sum(axis=0)[1:] > B[1:]
        for ia in np.flatnonzero(~ign):
            for ib in range(nb):
                i = int(t[ia + 1, ib + 1])
                u = int(A[ia + 1] + B[ib + 1]) - i
                if 2 * i > u and out["match_b"][a0 + ia] < 0:
                    out["match_b"][a0 + ia], out["inter"][a0 + ia], out["uni"][a0 + ia] = b0 + ib, i, u
                    out["b_matched"][b0 + ib] = True
                ta, tb = int(a_traj[a0 + ia]), int(b_traj[b0 + ib])
                if 2 * i >= u and u > 0 and 0 <= ta < n_a_traj and 0 <= tb < n_b_traj:
                    out["id_match"][ta, tb] += 1
    return out


# ------------------------------------------------------------------------------------------------ id images (the g22 fixture)
def id_image_rows(ids):
    """the MOTS rows of id images [F, H, W] (id = class * 1000 + instance, 0 = background): frame f = image f, ascending ids"""
    F, H, W = ids.shape
    rows = []
    for f in range(F):
        for obj in np.unique(ids[f]):
            if obj == 0:
                continue
            flat = (ids[f] == obj).T.reshape(-1)   # column-major
            edges = np.flatnonzero(np.diff(np.concatenate(([0], flat.astype(np.int8), [0]))))
            rle = M.rle_string(M.rle_counts_from_events(edges[edges < H * W], H * W))   # (no event at the image's end)
            rows.append("%d %d %d %d %d %s" % (f, obj, obj // 1000, H, W, rle))
    return rows


def write_txt(path, rows):
    with open(path, "w") as fh:
        fh.write("".join(r + "\n" for r in rows))
    return path


def id_image_lists(ids, classes):
    """label images [F, W * H] int32 (column-major) of the objects of ``classes`` in id images, with their list: ``(labels, ptr,
    entry_id)`` -- entries in (frame, ascending id) order"""
    F, H, W = ids.shape
    labels = np.full((F, W * H), -1, np.int32)
    ptr, entry_id = [0], []
    for f in range(F):
        flat = ids[f].T.reshape(-1)
        for obj in np.unique(flat):
            if obj != 0 and obj // 1000 in classes:
                labels[f, flat == obj] = len(entry_id)
                entry_id.append(int(obj))
        ptr.append(len(entry_id))
    return labels, np.asarray(ptr, np.int64), np.asarray(entry_id, np.int64)


def label_runs(labels):
    """the runs (entry, begin, end) of label images [F, hw], in (frame, position) order"""
    ent, beg, end = [], [], []
    for f in range(labels.shape[0]):
        row = np.concatenate(([-1], labels[f], [-1]))
        cuts = np.flatnonzero(row[1:] != row[:-1])
        for b, e in zip(cuts[:-1], cuts[1:]):
            if labels[f, b] >= 0:
                ent.append(labels[f, b]); beg.append(b); end.append(e)
    return np.asarray(ent, np.int32), np.asarray(beg, np.int32), np.asarray(end, np.int32)


def scene_lists(ids_gt, ids_pred, class_id=2, ignore_class=10):
    """both sides of a scene as the operators take them: a dict with labels_a / labels_b, a_ptr / b_ptr, a_ignore, a_traj /
    b_traj and the trajectory counts (ground truth: the objects of class_id and the ignore region; prediction: class_id)"""
    la, a_ptr, a_id = id_image_lists(ids_gt, (class_id, ignore_class))
    lb, b_ptr, b_id = id_image_lists(ids_pred, (class_id,))
    a_ignore = (a_id // 1000 == ignore_class).astype(np.uint8)
    gt_ids, tr_ids = np.unique(a_id[a_ignore == 0]), np.unique(b_id)
    a_traj = np.where(a_ignore == 0, np.searchsorted(gt_ids, a_id), -1).astype(np.int32)
    return {"labels_a": la, "labels_b": lb, "a_ptr": a_ptr, "b_ptr": b_ptr, "a_ignore": a_ignore, "a_traj": a_traj,
            "b_traj": np.searchsorted(tr_ids, b_id).astype(np.int32), "n_a_traj": gt_ids.size, "n_b_traj": tr_ids.size,
            "gt_ids": gt_ids, "tr_ids": tr_ids}


# ------------------------------------------------------------------------------------------------ the fixture's scenes
def scene_files(gold, scene, tmp_path):
    gt = write_txt(str(tmp_path / (scene + "_gt.txt")), id_image_rows(gold[scene + ":gt"]))
    pred = write_txt(str(tmp_path / (scene + "_pred.txt")), id_image_rows(gold[scene + ":pred"]))
    return pred, gt, int(gold[scene + ":seq_length"])


def assert_metrics_equal(m, gold, scene):
    """every registered metric, the per-frame counts and the matched-id sequences of ``m`` (``details=True``) against the fixture"""
    names = [k.split(":")[2] for k in gold if k.startswith(scene + ":m:")]
    assert sorted(names) == sorted(METRIC_NAMES)
    for k in names:
        want, got = float(gold["%s:m:%s" % (scene, k)]), float(m[k])
        if want == int(want) and k not in ("total_cost",):
            assert got == want, (k, got, want)
        else:
            assert abs(got - want) <= 1e-12 * abs(want), (k, got, want)
    np.testing.assert_array_equal(m["per_frame"], gold[scene + ":per_frame"])
    ids, ptr, flat = gold[scene + ":traj_ids"], gold[scene + ":traj_ptr"], gold[scene + ":traj_matched"]
    assert sorted(m["trajectories"]) == list(ids)
    for j, g in enumerate(ids):
        assert m["trajectories"][int(g)] == list(flat[ptr[j]:ptr[j + 1]]), g


def ellipse_labels(rng, F, H, W, per_frame, r_lo=2.0, r_hi=9.0):
    """label images [F, W * H] int32 (column-major) of per_frame[f] random ellipses in frame f (a later one only takes free
    pixels; one that finds none keeps its entry with no pixel) and their ptr"""
    labels = np.full((F, H, W), -1, np.int32)
    ptr = np.concatenate(([0], np.cumsum(per_frame))).astype(np.int64)
    for f in range(F):
        for e in range(int(ptr[f]), int(ptr[f + 1])):
            cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(r_lo, r_hi), rng.uniform(r_lo, r_hi)
            y0, y1, x0, x1 = max(int(cy - ry), 0), min(int(cy + ry) + 1, H), max(int(cx - rx), 0), min(int(cx + rx) + 1, W)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            win = labels[f, y0:y1, x0:x1]
            win[(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0) & (win < 0)] = e
    return np.ascontiguousarray(labels.transpose(0, 2, 1)).reshape(F, W * H), ptr
