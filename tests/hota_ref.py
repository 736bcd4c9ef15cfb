"""numpy restatements of the five operators of ``csrc/hota.hip`` with the argument contracts of ``include/mpnhip.h`` and the call
signatures of the wrappers in ``mpntrackseg_amd/hota_eval.py`` (so that the host side of the evaluation runs over them without a
device), written from TrackEval's ``kitti_mots.py:299-387`` and ``hota.py:47-112`` frame by frame; plus the two operators of
``mots_metrics_ref`` the evaluation needs, and the helpers the HOTA tests share (the g23 fixture's scenes as MOTS text files)."""
import os

import numpy as np

import mots_metrics_ref as R
from mots_metrics_ref import label_overlap, paint_label_runs  # noqa: F401  (the evaluation takes them from its ops)
from mpntrackseg_amd import hota_eval as HE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_hota.npz")
SCENES = ("cases", "crowded", "association")
EPS = np.finfo("float").eps
ALPHAS = np.arange(0.05, 0.99, 0.05)
FIELDS = HE.FLOAT_ARRAY_FIELDS + HE.INTEGER_ARRAY_FIELDS + HE.FLOAT_FIELDS


def sim_offsets(a_ptr, b_ptr):
    a, b = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    return np.concatenate(([0], np.cumsum(np.diff(a) * np.diff(b)))).astype(np.int64)


def _frames(S):
    for f in range(S["F"]):
        a0, b0 = int(S["a_ptr"][f]), int(S["b_ptr"][f])
        yield f, a0, int(S["a_ptr"][f + 1]) - a0, b0, int(S["b_ptr"][f + 1]) - b0


def _block(S, key, f, na, nb):
    return S[key][S["sim_ptr"][f]:S["sim_ptr"][f] + na * nb].reshape(na, nb)


def frame_similarity(table, table_ptr, a_ptr, b_ptr, a_ignore, b_scored):
    a_ptr, b_ptr = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    table = np.asarray(table).astype(np.int64)
    ignore, scored = np.asarray(a_ignore).reshape(-1).astype(bool), np.asarray(b_scored).reshape(-1).astype(bool)
    sp = sim_offsets(a_ptr, b_ptr)
    n_a, n_b = int(a_ptr[-1]), int(b_ptr[-1])
    S = {"F": a_ptr.size - 1, "n_a": n_a, "n_b": n_b, "a_ptr": a_ptr, "b_ptr": b_ptr, "sim_ptr": sp, "sim_cells": int(sp[-1]),
         "sim": np.zeros(int(sp[-1]), np.float64), "b_removed": np.zeros(n_b, np.uint8), "row_sum": np.zeros(n_a, np.float64),
         "col_sum": np.zeros(n_b, np.float64)}
    for f, a0, na, b0, nb in _frames(S):
        t = table[table_ptr[f]:table_ptr[f] + (na + 1) * (nb + 1)].reshape(na + 1, nb + 1)
        A, B = t.sum(axis=1), t.sum(axis=0)
        ign, sc = ignore[a0:a0 + na], scored[b0:b0 + nb]
        sim = _block(S, "sim", f, na, nb)
        matched = np.zeros(nb, bool)
        for ia in np.flatnonzero(~ign):
            first = True
            for ib in np.flatnonzero(sc):
                i = int(t[ia + 1, ib + 1])
                u = int(A[ia + 1] + B[ib + 1]) - i
                if i > 0:
                    sim[ia, ib] = float(i) / float(u)
                    if 2 * i >= u and first:      # eligible: not (sim < 0.5 - eps); the earliest in the list is the match
                        matched[ib], first = True, False
        removed = sc & ~matched & (2 * t[1:][ign].sum(axis=0)[1:] > B[1:])
        kept = sc & ~removed
        S["b_removed"][b0:b0 + nb] = removed
        for ia in np.flatnonzero(~ign):
            S["row_sum"][a0 + ia] = sim[ia, kept].sum()
        for ib in np.flatnonzero(kept):
            S["col_sum"][b0 + ib] = sim[:, ib].sum()
    S["b_removed_host"] = S["b_removed"].astype(bool)
    return S


def accumulators(n_gt_ids, n_tr_ids, device=None):
    G, T = int(n_gt_ids), int(n_tr_ids)
    return {"n_gt": G, "n_tr": T, "potential": np.zeros(G * T, np.float64), "gt_count": np.zeros(G, np.int32),
            "tr_count": np.zeros(T, np.int32), "tp": np.zeros(ALPHAS.size, np.int64), "loca": np.zeros(ALPHAS.size, np.float64),
            "matches_count": np.zeros(ALPHAS.size * G * T, np.int32)}


def _kept(S, a_traj, b_traj, acc):
    at, bt = np.asarray(a_traj).reshape(-1).astype(np.int64), np.asarray(b_traj).reshape(-1).astype(np.int64)
    return at, bt, (at >= 0) & (at < acc["n_gt"]), (bt >= 0) & (bt < acc["n_tr"]) & ~np.asarray(S["b_removed"]).astype(bool)


def accumulate_alignment(S, a_traj, b_traj, acc):
    at, bt, ka, kb = _kept(S, a_traj, b_traj, acc)
    pot = acc["potential"].reshape(acc["n_gt"], acc["n_tr"])
    for f, a0, na, b0, nb in _frames(S):
        rows, cols = np.flatnonzero(ka[a0:a0 + na]), np.flatnonzero(kb[b0:b0 + nb])
        sim = _block(S, "sim", f, na, nb)[rows][:, cols]
        denom = S["col_sum"][b0 + cols][np.newaxis, :] + S["row_sum"][a0 + rows][:, np.newaxis] - sim
        sim_iou = np.zeros_like(sim)
        mask = denom > 0 + EPS
        sim_iou[mask] = sim[mask] / denom[mask]
        pot[at[a0 + rows][:, np.newaxis], bt[b0 + cols][np.newaxis, :]] += sim_iou
        np.add.at(acc["gt_count"], at[a0 + rows], 1)
        np.add.at(acc["tr_count"], bt[b0 + cols], 1)


def frame_scores(S, a_traj, b_traj, acc):
    at, bt, ka, kb = _kept(S, a_traj, b_traj, acc)
    pot = acc["potential"].reshape(acc["n_gt"], acc["n_tr"])
    score = np.zeros(S["sim_cells"], np.float64)
    out = {"sim_ptr": S["sim_ptr"], "score": score}
    for f, a0, na, b0, nb in _frames(S):
        rows, cols = np.flatnonzero(ka[a0:a0 + na]), np.flatnonzero(kb[b0:b0 + nb])
        if rows.size == 0 or cols.size == 0:
            continue
        g, t = at[a0 + rows][:, np.newaxis], bt[b0 + cols][np.newaxis, :]
        gas = pot[g, t] / (acc["gt_count"][g].astype(np.float64) + acc["tr_count"][t].astype(np.float64) - pot[g, t])
        blk = _block(out, "score", f, na, nb)
        blk[np.ix_(rows, cols)] = gas * _block(S, "sim", f, na, nb)[rows][:, cols]
    return score


def alpha_accumulate(S, a_traj, b_traj, match_b, alphas, acc):
    at, bt, ka, kb = _kept(S, a_traj, b_traj, acc)
    mb = np.asarray(match_b).reshape(-1).astype(np.int64)
    mc = acc["matches_count"].reshape(ALPHAS.size, acc["n_gt"], acc["n_tr"])
    for f, a0, na, b0, nb in _frames(S):
        sim = _block(S, "sim", f, na, nb)
        for k, alpha in enumerate(np.asarray(alphas, np.float64)):
            total = 0.0
            for ia in range(na):
                b = mb[a0 + ia]
                if ka[a0 + ia] and b0 <= b < b0 + nb and kb[b] and sim[ia, b - b0] >= alpha - EPS:
                    acc["tp"][k] += 1
                    total += sim[ia, b - b0]
                    mc[k, at[a0 + ia], bt[b]] += 1
            acc["loca"][k] += total


def association(acc):
    G, T = acc["n_gt"], acc["n_tr"]
    gc, tc = acc["gt_count"].astype(np.float64).reshape(G, 1), acc["tr_count"].astype(np.float64).reshape(1, T)
    ass = np.zeros((ALPHAS.size, 3), np.float64)
    for k in range(ALPHAS.size):
        mc = acc["matches_count"].reshape(ALPHAS.size, G, T)[k].astype(np.float64)
        ass[k] = (np.sum(mc * (mc / np.maximum(1, gc + tc - mc))), np.sum(mc * (mc / np.maximum(1, gc))),
                  np.sum(mc * (mc / np.maximum(1, tc))))
    return {"ass": ass, "tp": acc["tp"].copy(), "loca": acc["loca"].copy()}


# ------------------------------------------------------------------------------------------------ the fixture's scenes
def scene_images(gold, gold22, scene):
    """(ground-truth id images, prediction id images, num_timesteps): g23 stores only the new scene's, the others are g22's"""
    src = gold if scene + ":gt" in gold else gold22
    return src[scene + ":gt"], src[scene + ":pred"], int(gold[scene + ":num_timesteps"])


def scene_files(gold, gold22, scene, tmp_path):
    gt, pred, T = scene_images(gold, gold22, scene)
    return (R.write_txt(str(tmp_path / (scene + "_pred.txt")), R.id_image_rows(pred)),
            R.write_txt(str(tmp_path / (scene + "_gt.txt")), R.id_image_rows(gt)), T)


def loaded(ids, tmp_path, name):
    """id images through a MOTS text file and ``load_mots_txt``"""
    from mpntrackseg_amd.mots_eval import load_mots_txt
    return load_mots_txt(R.write_txt(str(tmp_path / (name + ".txt")), R.id_image_rows(ids)))


def close(got, want, what=""):
    """sums against numpy: 1e-9 relative, absolute where the value is 0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (np.abs(got - want) <= 1e-9 * np.where(want == 0, 1.0, np.abs(want))).all(), (what, got, want)


def assert_hota_equal(res, gold, prefix):
    """every field of a result against the fixture: the integer fields and the counts exactly, the others within 1e-9"""
    for k in HE.INTEGER_ARRAY_FIELDS + HE.COUNT_FIELDS:
        if prefix + ":" + k in gold:
            assert np.array_equal(np.asarray(res[k], np.float64), np.asarray(gold[prefix + ":" + k], np.float64)), (k, res[k])
    for k in HE.FLOAT_ARRAY_FIELDS + HE.FLOAT_FIELDS:
        close(res[k], gold[prefix + ":" + k], k)


def assert_kept_ids(res, gold, scene):
    ptr, ids = gold[scene + ":kept_ptr"], gold[scene + ":kept_ids"]
    for f in range(ptr.size - 1):
        assert sorted(res["kept_tracker_ids"].get(f, [])) == sorted(ids[ptr[f]:ptr[f + 1]].tolist()), f


def small_frames():
    """the 3-frame 37 x 29 case of the MOTS tests (an ignore region, a pair at IoU exactly 0.5, a prediction mostly inside the
    ignore region, a miss) as rectangles [y0, y1) x [x0, x1) with a trajectory index (-1: ignore); its lists for the operators"""
    H, W = 37, 29
    a = [[(2, 10, 2, 7, 0), (14, 17, 10, 12, 1), (0, H, 22, W, -1)],
         [(2, 10, 2, 7, 0), (20, 30, 3, 9, 2)],
         [(5, 12, 5, 12, 1), (14, 22, 2, 7, 2), (0, H, 22, W, -1)]]
    b = [[(3, 11, 2, 7, 0), (15, 18, 10, 12, 1), (26, 32, 20, 26, 2)],
         [(2, 10, 3, 8, 3), (0, 5, 20, 25, 1)],
         [(5, 12, 5, 12, 0), (30, 35, 2, 7, 2)]]

    def side(frames):
        lab = np.full((len(frames), H, W), -1, np.int32)
        ptr, traj = [0], []
        for f, rects in enumerate(frames):
            for y0, y1, x0, x1, t in rects:
                lab[f, y0:y1, x0:x1] = len(traj)
                traj.append(t)
            ptr.append(len(traj))
        return np.ascontiguousarray(lab.transpose(0, 2, 1)).reshape(len(frames), H * W), np.asarray(ptr, np.int64), np.asarray(traj, np.int32)
    la, a_ptr, a_traj = side(a)
    lb, b_ptr, b_traj = side(b)
    return {"labels_a": la, "labels_b": lb, "a_ptr": a_ptr, "b_ptr": b_ptr, "a_ignore": (a_traj < 0).astype(np.uint8), "a_traj": a_traj,
            "b_traj": b_traj, "b_scored": np.ones(b_traj.size, np.uint8), "n_a_traj": 3, "n_b_traj": 4}


def scene_lists(ids_gt, ids_pred):
    """``mots_metrics_ref.scene_lists`` plus the scored flags (every prediction of the list is of the evaluated class)"""
    L = R.scene_lists(ids_gt, ids_pred)
    L["b_scored"] = np.ones(L["b_traj"].size, np.uint8)
    return L
