"""numpy restatements of the operators of ``csrc/clear_identity.hip`` with the argument contracts of ``include/mpnhip.h`` and the
call signatures of the wrappers in ``mpntrackseg_amd/kitti_mots_eval.py``, written from TrackEval's ``clear.py:67-121`` and
``identity.py:53-61`` frame by frame.  ``hota_ref``'s operators are re-exported, so the module serves as ``_ops`` of
``kitti_mots_eval.evaluate_sequence_files`` and the host side of the evaluation runs without a device.  Plus the helpers the
tests share: the g24 fixture's scenes as MOTS text files and the comparison of a result with the fixture."""
import os

import numpy as np

import hota_ref as HR
import mots_metrics_ref as R
from hota_ref import (accumulate_alignment, accumulators, alpha_accumulate, association, frame_scores, frame_similarity,  # noqa: F401
                      label_overlap, paint_label_runs)
from mpntrackseg_amd import hota_eval as HE, kitti_mots_eval as KE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_clear_identity.npz")
SCENES = ("cases", "crowded", "association", "clear")
CLASSES = ("car", "pedestrian")
EPS = np.finfo("float").eps
STATE_KEYS = ("prev_tracker_id", "prev_timestep_tracker_id", "gt_id_count", "gt_matched_count", "gt_frag_count", "counters")


# ------------------------------------------------------------------------------------------------ Identity
def identity_accumulators(n_gt_ids, n_tr_ids, device=None):
    G, T = int(n_gt_ids), int(n_tr_ids)
    return {"n_gt": G, "n_tr": T, "potential_count": np.zeros(G * T, np.int32)}


def identity_accumulate(S, a_traj, b_traj, acc):
    at, bt, ka, kb = HR._kept(S, a_traj, b_traj, acc)
    pc = acc["potential_count"].reshape(acc["n_gt"], acc["n_tr"])
    for f, a0, na, b0, nb in HR._frames(S):
        sim = HR._block(S, "sim", f, na, nb)
        mask = np.greater_equal(sim, 0.5) & ka[a0:a0 + na][:, np.newaxis] & kb[b0:b0 + nb][np.newaxis, :]
        ia, ib = np.nonzero(mask)
        np.add.at(pc, (at[a0 + ia], bt[b0 + ib]), 1)


def identity_table(acc):
    return acc["potential_count"].reshape(acc["n_gt"], acc["n_tr"]).copy()


def identity_sums(acc, match_b):
    pc = acc["potential_count"].reshape(acc["n_gt"], acc["n_tr"])
    mb = np.asarray(match_b).reshape(-1).astype(np.int64)
    return int(sum(int(pc[g, t]) for g, t in enumerate(mb) if 0 <= t < acc["n_tr"]))


def identity_kit(table, gt_id_count, tracker_id_count):
    """identity.py:63-85 as it stands: the (G + T) x (G + T) problem with 1e10 walls -> (IDTP, IDFN, IDFP)"""
    from scipy.optimize import linear_sum_assignment
    table = np.asarray(table, np.float64)
    G, T = table.shape
    fp_mat, fn_mat = np.zeros((G + T, G + T)), np.zeros((G + T, G + T))
    fp_mat[G:, :T] = 1e10
    fn_mat[:G, T:] = 1e10
    for g in range(G):
        fn_mat[g, :T] = gt_id_count[g]
        fn_mat[g, T + g] = gt_id_count[g]
    for t in range(T):
        fp_mat[:G, t] = tracker_id_count[t]
        fp_mat[t + G, t] = tracker_id_count[t]
    fn_mat[:G, :T] -= table
    fp_mat[:G, :T] -= table
    r, c = linear_sum_assignment(fn_mat + fp_mat)
    idfn, idfp = int(fn_mat[r, c].sum()), int(fp_mat[r, c].sum())
    return int(np.sum(gt_id_count)) - idfn, idfn, idfp


# ------------------------------------------------------------------------------------------------ CLEAR
def clear_accumulators(n_gt_ids, device=None):
    G = int(n_gt_ids)
    return {"n_gt": G, "prev_tracker_id": np.full(G, -1, np.int32), "prev_timestep_tracker_id": np.full(G, -1, np.int32),
            "gt_id_count": np.zeros(G, np.int32), "gt_matched_count": np.zeros(G, np.int32), "gt_frag_count": np.zeros(G, np.int32),
            "counters": np.zeros(4, np.int64), "motp_sum": np.zeros(1, np.float64), "status": []}


def clear_frame_candidates(S, a_traj, b_traj, n_gt_ids, n_tr_ids):
    at, bt, ka, kb = HR._kept(S, a_traj, b_traj, {"n_gt": int(n_gt_ids), "n_tr": int(n_tr_ids)})
    a_cand, b_cand = np.full((S["n_a"], 2), -1, np.int32), np.full((S["n_b"], 2), -1, np.int32)
    status = 0
    for f, a0, na, b0, nb in HR._frames(S):
        sim = HR._block(S, "sim", f, na, nb)
        elig = ~(sim < 0.5 - EPS) & ka[a0:a0 + na][:, np.newaxis] & kb[b0:b0 + nb][np.newaxis, :]   # clear.py:81
        for ia in range(na):
            cols = np.flatnonzero(elig[ia])
            a_cand[a0 + ia, :min(cols.size, 2)] = b0 + cols[:2]
            status |= 1 if cols.size > 2 else 0
        for ib in range(nb):
            rows = np.flatnonzero(elig[:, ib])
            b_cand[b0 + ib, :min(rows.size, 2)] = a0 + rows[:2]
            status |= 1 if rows.size > 2 else 0
        if (elig & (elig.sum(axis=1, keepdims=True) >= 2) & (elig.sum(axis=0, keepdims=True) >= 2)).any():
            status |= 2
    return {"a_cand": a_cand.reshape(-1), "b_cand": b_cand.reshape(-1), "status": np.array([status], np.int32)}


def clear_sequence_scan(S, a_traj, b_traj, cand, n_tr_ids, acc):
    """clear.py:67-114 with the assignment replaced by the rule for pairs and stars"""
    G = acc["n_gt"]
    at, bt, ka, kb = HR._kept(S, a_traj, b_traj, {"n_gt": G, "n_tr": int(n_tr_ids)})
    a_cand, b_cand = np.asarray(cand["a_cand"]).reshape(-1, 2), np.asarray(cand["b_cand"]).reshape(-1, 2)
    prev, prev_ts, cnt = acc["prev_tracker_id"], acc["prev_timestep_tracker_id"], acc["counters"]
    match_b = np.full(S["n_a"], -1, np.int32)
    for f, a0, na, b0, nb in HR._frames(S):
        rows, cols = a0 + np.flatnonzero(ka[a0:a0 + na]), b0 + np.flatnonzero(kb[b0:b0 + nb])
        if rows.size == 0:
            cnt[2] += cols.size
            continue
        if cols.size == 0:
            cnt[1] += rows.size
            np.add.at(acc["gt_id_count"], at[rows], 1)
            continue
        sim = HR._block(S, "sim", f, na, nb)
        matched = []
        for a in rows:
            c0, c1 = a_cand[a]
            if c0 < 0:
                continue
            if c1 >= 0:                                    # a row star: the later arm wins only by continuity
                m = c1 if bt[c1] == prev_ts[at[a]] else c0
            else:
                d0, d1 = b_cand[c0]
                if d1 < 0:                                 # a single pair
                    m = c0
                else:                                      # a column star
                    m = c0 if a == (d1 if prev_ts[at[d1]] == bt[c0] else d0) else -1
            if m >= 0:
                matched.append((a, m))
        now = np.full(G, -1, np.int32)
        total = 0.0
        for a, m in matched:
            g, t = at[a], bt[m]
            match_b[a] = m
            cnt[3] += 1 if prev[g] >= 0 and prev[g] != t else 0
            prev[g] = t
            now[g] = t
            acc["gt_matched_count"][g] += 1
            total += sim[a - a0, m - b0]
        np.add.at(acc["gt_id_count"], at[rows], 1)
        acc["gt_frag_count"] += (prev_ts < 0) & (now >= 0)
        prev_ts[:] = now
        cnt[0] += len(matched)
        cnt[1] += rows.size - len(matched)
        cnt[2] += cols.size - len(matched)
        if matched:
            acc["motp_sum"][0] += total
    acc["status"].append(cand["status"])
    return match_b


def clear_track_summary(acc):
    KE.check_clear_status(acc["status"])
    c, m, fr = acc["gt_id_count"], acc["gt_matched_count"], acc["gt_frag_count"]
    ratio = m[c > 0] / c[c > 0]
    mt = int(np.sum(np.greater(ratio, 0.8)))
    pt = int(np.sum(np.greater_equal(ratio, 0.2))) - mt
    res = {k: int(v) for k, v in zip(("CLR_TP", "CLR_FN", "CLR_FP", "IDSW"), acc["counters"])}
    res.update(MT=mt, PT=pt, ML=acc["n_gt"] - mt - pt, Frag=int(np.sum(fr[fr > 0] - 1)), MOTP_sum=float(acc["motp_sum"][0]))
    return res


# ------------------------------------------------------------------------------------------------ the fixture's scenes
def golds():
    """(g24, g23, g22): g24 stores only the new scene's id images"""
    return dict(np.load(GOLDEN)), dict(np.load(HR.GOLDEN)), dict(np.load(R.GOLDEN))


def scene_images(gold, gold23, gold22, scene):
    src = next(g for g in (gold, gold23, gold22) if scene + ":gt" in g)
    return src[scene + ":gt"], src[scene + ":pred"], int(gold[scene + ":num_timesteps"])


def scene_files(gold, gold23, gold22, scene, tmp_path):
    gt, pred, T = scene_images(gold, gold23, gold22, scene)
    return (R.write_txt(str(tmp_path / (scene + "_pred.txt")), R.id_image_rows(pred)),
            R.write_txt(str(tmp_path / (scene + "_gt.txt")), R.id_image_rows(gt)), T)


def scene_lists(gt, pred, cls):
    """``mots_metrics_ref.scene_lists`` for the class plus the scored flags (every prediction of the list is of the class)"""
    L = R.scene_lists(gt, pred, class_id=KE.CLASS_IDS[cls])
    L["b_scored"] = np.ones(L["b_traj"].size, np.uint8)
    return L


INTEGER_FIELDS = {"HOTA": HE.INTEGER_ARRAY_FIELDS, "CLEAR": KE.CLEAR_INTEGER_FIELDS, "Identity": KE.IDENTITY_INTEGER_FIELDS,
                  "Count": KE.COUNT_FIELDS}
FLOAT_FIELDS = {"HOTA": HE.FLOAT_ARRAY_FIELDS + HE.FLOAT_FIELDS, "CLEAR": KE.CLEAR_FLOAT_FIELDS, "Identity": KE.IDENTITY_FLOAT_FIELDS,
                "Count": ()}


def assert_metrics_equal(res, gold, prefix):
    """{metric: fields} against the fixture's ``prefix:metric:field``: every field the kit recorded is there; the integer fields
    and counts exactly, the float fields within 1e-9 relative, absolute where the value is 0"""
    for metric in ("HOTA", "CLEAR", "Identity", "Count"):
        want = {k.split(":")[-1]: v for k, v in gold.items() if k.startswith("%s:%s:" % (prefix, metric))}
        assert want and set(want) <= set(res[metric]), (prefix, metric, sorted(set(want) - set(res[metric])))
        assert set(want) >= set(INTEGER_FIELDS[metric]) - {"Frames"} and set(want) >= set(FLOAT_FIELDS[metric]), (prefix, metric)
        for k, v in want.items():
            if k in INTEGER_FIELDS[metric]:
                assert np.array_equal(np.asarray(res[metric][k], np.float64), np.asarray(v, np.float64)), (prefix, metric, k, res[metric][k], v)
            else:
                HR.close(res[metric][k], v, "%s:%s:%s" % (prefix, metric, k))


def assert_same_bits(x, y, what=""):
    """two nested results: the same keys and the same bits"""
    assert sorted(x) == sorted(y), what
    for k in x:
        if isinstance(x[k], dict):
            assert_same_bits(x[k], y[k], "%s:%s" % (what, k))
        else:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), (what, k, x[k], y[k])
