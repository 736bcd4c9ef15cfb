"""HOTA of a KITTI-MOTS sequence: host mirror of ``eval_kitti_mots`` (reference ``src/mot_neural_solver/utils/evaluation.py:127-135``
-> ``TrackEval/scripts/run_kitti_mots.py:47-90``), i.e. the ``KittiMOTS`` dataset's ``get_preprocessed_seq_data``
(``trackeval/datasets/kitti_mots.py:299-387``) and ``HOTA.eval_sequence`` / ``combine_sequences``
(``trackeval/metrics/hota.py:25-129``) for one class, over the C ABI (``csrc/hota.hip``).

A frame is one int32 label per pixel on either side, and all its mask intersections are one table of ``mots_eval.label_overlap``
-- the pixel work of ``mots_eval``, run once per frame.  Everything HOTA does with the tables stays on the device: the IoU block
of every frame and the predictions the preprocessing removes (``frame_similarity``), the global alignment of the ids
(``accumulate_alignment``), the cells of the per-frame assignment problems (``frame_scores``), the counts per alpha
(``alpha_accumulate``) and the association sums (``association``).  The assignment itself is, by default
(``assignment='host'``), ``scipy.optimize.linear_sum_assignment`` on the host, as the IDF1 assignment of ``mots_eval`` is: per
launch the score cells come down in one copy and the chosen prediction of every ground-truth entry goes up in one.  With
``assignment='device'`` it is ``assignment.linear_sum_assignment_batched`` on the score block as it lies, one problem per frame:
no score cell comes down and no match goes up, only the solver's status per frame, once per sequence.  Where a frame's optimum
is not unique the two may choose different pairs of the same total.  ``pycocotools`` is not needed.

The alignment needs every frame before the first assignment, so each launch's similarity block stays on the device between the
two passes: 8 B x (sum over the frames of objects x predictions), plus 8 B per entry -- about 3 MB for a thousand frames of
twenty objects a side.

An empty mask has similarity 0 with everything (the kit's 0 / 0 = NaN fails its own range assertion).

One deliberate difference: a ground-truth mask split EXACTLY in half by two predictions is eligible (IoU 0.5) with both, and the
preprocessing matches one of them; the kit's choice follows scipy's tie order, here the prediction earlier in the list is the
matched one.  Among disjoint masks it cannot change a result: eligibility with both puts each half wholly inside the object,
away from the ignore region, so the unmatched half is kept either way.

Ids are not renumbered: ``num_tracker_ids`` counts the prediction ids that keep a detection after the removal, which is all the
kit's contiguous renumbering (``kitti_mots.py:359-373``) shows in the result."""
import ctypes as C
import sys

import numpy as np
import torch

from . import capi
from .capi import MpnhipError, check, ptr, stream_ptr
from .mots_eval import CLASS_ID, IGNORE_CLASS, _Side, _as_loaded, _buf, _i32, _image_size, label_overlap, paint_label_runs  # noqa: F401

ALPHAS = np.arange(0.05, 0.99, 0.05)   # hota.py:17 -- these very doubles go to the device
N_ALPHAS = ALPHAS.size
FLOAT_ARRAY_FIELDS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA", "RHOTA")
INTEGER_ARRAY_FIELDS = ("HOTA_TP", "HOTA_FN", "HOTA_FP")
FLOAT_FIELDS = ("HOTA(0)", "LocA(0)", "HOTALocA(0)")
COUNT_FIELDS = ("num_gt_dets", "num_tracker_dets", "num_gt_ids", "num_tracker_ids")


# ------------------------------------------------------------------------------------------------ operators (device)
def sim_offsets(a_ptr, b_ptr):
    """``sim_ptr`` [F + 1] (int64, host) of two lists: frame f owns ``na_f * nb_f`` cells."""
    a, b = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    if a.size != b.size or a.size < 1:
        raise MpnhipError("a_ptr and b_ptr need one entry per frame plus one")
    return np.concatenate(([0], np.cumsum(np.diff(a) * np.diff(b)))).astype(np.int64)


def _u8(v, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.uint8)).to(dev)


def _workspace(lib, S, n_gt, n_tr, dev):
    need = lib.mpnhip_hota_workspace_bytes(S["n_a"], S["n_b"], S["F"], int(n_gt), int(n_tr))
    if need == 0:
        raise MpnhipError("%d x %d ids x %d alphas, or %d frames x %d ids (2^31 cells or more) is not supported"
                          % (n_gt, n_tr, N_ALPHAS, S["F"], n_gt + n_tr))
    return capi.workspace(need, dev, "hota_eval")


@capi.on_tensor_device
def frame_similarity(table, table_ptr, a_ptr, b_ptr, a_ignore, b_scored):
    """One launch's similarities and removals from its table (``mpnhip_hota_frame_similarity``): a dict with ``sim`` (float64,
    device; frame f owns ``na_f x nb_f`` cells at ``sim_ptr[f]``), ``sim_ptr`` (int64, host), ``b_removed`` (uint8, device),
    ``b_removed_host`` (bool), ``row_sum`` / ``col_sum`` (float64, device) and the lists -- what the other operators take."""
    lib = capi.load()
    capi.require_device(table)
    dev = table.device
    ap, bp = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    tp = np.ascontiguousarray(np.asarray(table_ptr, np.int64).reshape(-1))
    F, n_a, n_b = ap.size - 1, int(ap[-1]), int(bp[-1])
    if bp.size != F + 1 or tp.size != F + 1:
        raise MpnhipError("a_ptr, b_ptr and table_ptr need one entry per frame plus one")
    sp = sim_offsets(ap, bp)
    ign, sc = _u8(a_ignore, dev), _u8(b_scored, dev)
    if ign.numel() != n_a or sc.numel() != n_b:
        raise MpnhipError("one ignore flag per a-entry, one scored flag per b-entry")
    S = {"F": F, "n_a": n_a, "n_b": n_b, "a_ptr": ap, "b_ptr": bp, "sim_ptr": sp, "sim_cells": int(sp[-1]),
         "_a_ptr": _i32(ap, dev), "_b_ptr": _i32(bp, dev), "_sim_ptr": torch.from_numpy(sp).to(dev),
         "sim": _buf(int(sp[-1]), torch.float64, dev), "b_removed": _buf(n_b, torch.uint8, dev),
         "row_sum": _buf(n_a, torch.float64, dev), "col_sum": _buf(n_b, torch.float64, dev)}
    ws = _workspace(lib, S, 0, 0, dev)
    tp_dev = torch.from_numpy(tp).to(dev)   # (named: it lives until the call returns)
    check(lib.mpnhip_hota_frame_similarity(ptr(table), int(tp[-1]), ptr(tp_dev), ptr(S["_a_ptr"]), n_a, ptr(S["_b_ptr"]), n_b, F, ptr(ign),
                                           ptr(sc), ptr(S["_sim_ptr"]), S["sim_cells"], ptr(S["sim"]), ptr(S["b_removed"]),
                                           ptr(S["row_sum"]), ptr(S["col_sum"]), ptr(ws), ws.numel(), stream_ptr()),
          "mpnhip_hota_frame_similarity")
    S["b_removed_host"] = S["b_removed"].cpu().numpy().astype(bool)
    return S


def accumulators(n_gt_ids, n_tr_ids, device):
    """The zeroed accumulators of a sequence on ``device``: ``potential`` [G, T] (float64), ``gt_count`` [G], ``tr_count`` [T]
    (int32), ``tp`` [19] (int64), ``loca`` [19] (float64) and ``matches_count`` [19, G, T] (int32)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise MpnhipError("mpntrackseg_amd runs on a HIP device only (%s); there is no CPU fallback" % dev)
    G, T = int(n_gt_ids), int(n_tr_ids)
    if G * T * N_ALPHAS >= 1 << 31:
        raise MpnhipError("a matches_count of %d x %d x %d (2^31 cells or more) is not supported" % (N_ALPHAS, G, T))
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)[:n]
    return {"n_gt": G, "n_tr": T, "potential": z(G * T, torch.float64), "gt_count": z(G, torch.int32), "tr_count": z(T, torch.int32),
            "tp": z(N_ALPHAS, torch.int64), "loca": z(N_ALPHAS, torch.float64), "matches_count": z(N_ALPHAS * G * T, torch.int32)}


def _traj(S, a_traj, b_traj, dev):
    at, bt = _i32(a_traj, dev), _i32(b_traj, dev)
    if at.numel() != S["n_a"] or bt.numel() != S["n_b"]:
        raise MpnhipError("one trajectory index per a-entry and per b-entry")
    return at, bt


def accumulate_alignment(S, a_traj, b_traj, acc):
    """+ the launch ``S`` into ``acc``'s ``potential``, ``gt_count`` and ``tr_count`` (``mpnhip_hota_accumulate_alignment``).
    ``a_traj`` / ``b_traj``: index of every entry's id, -1 for an entry that takes no part."""
    lib = capi.load()
    dev = S["sim"].device
    with torch.cuda.device(dev):
        at, bt = _traj(S, a_traj, b_traj, dev)
        ws = _workspace(lib, S, acc["n_gt"], acc["n_tr"], dev)
        check(lib.mpnhip_hota_accumulate_alignment(ptr(S["sim"]), S["sim_cells"], ptr(S["_sim_ptr"]), ptr(S["_a_ptr"]), S["n_a"],
                                                   ptr(S["_b_ptr"]), S["n_b"], S["F"], ptr(at), ptr(bt), ptr(S["b_removed"]),
                                                   ptr(S["row_sum"]), ptr(S["col_sum"]), acc["n_gt"], acc["n_tr"], ptr(acc["potential"]),
                                                   ptr(acc["gt_count"]), ptr(acc["tr_count"]), ptr(ws), ws.numel(), stream_ptr()),
              "mpnhip_hota_accumulate_alignment")


def frame_scores(S, a_traj, b_traj, acc, host=True):
    """The score cells of the launch ``S`` (the layout of ``sim``; ``mpnhip_hota_frame_scores``) as a host array, or with
    ``host=False`` as the device tensor."""
    lib = capi.load()
    dev = S["sim"].device
    with torch.cuda.device(dev):
        at, bt = _traj(S, a_traj, b_traj, dev)
        score = _buf(S["sim_cells"], torch.float64, dev)
        check(lib.mpnhip_hota_frame_scores(ptr(S["sim"]), S["sim_cells"], ptr(S["_sim_ptr"]), ptr(S["_a_ptr"]), S["n_a"], ptr(S["_b_ptr"]),
                                           S["n_b"], S["F"], ptr(at), ptr(bt), ptr(S["b_removed"]), acc["n_gt"], acc["n_tr"],
                                           ptr(acc["potential"]), ptr(acc["gt_count"]), ptr(acc["tr_count"]), ptr(score), stream_ptr()),
              "mpnhip_hota_frame_scores")
        return score.cpu().numpy() if host else score


def alpha_accumulate(S, a_traj, b_traj, match_b, alphas, acc):
    """+ the assignment ``match_b`` [n_a] (index into the launch's b-list, or -1) of the launch ``S`` into ``acc``'s ``tp``,
    ``loca`` and ``matches_count`` (``mpnhip_hota_alpha_accumulate``)."""
    lib = capi.load()
    dev = S["sim"].device
    al = np.ascontiguousarray(np.asarray(alphas, np.float64).reshape(-1))
    if al.size != N_ALPHAS:
        raise MpnhipError("%d alphas" % N_ALPHAS)
    with torch.cuda.device(dev):
        at, bt = _traj(S, a_traj, b_traj, dev)
        mb = _i32(match_b, dev)
        if mb.numel() != S["n_a"]:
            raise MpnhipError("one match per a-entry")
        ws = _workspace(lib, S, acc["n_gt"], acc["n_tr"], dev)
        check(lib.mpnhip_hota_alpha_accumulate(ptr(S["sim"]), S["sim_cells"], ptr(S["_sim_ptr"]), ptr(S["_a_ptr"]), S["n_a"],
                                               ptr(S["_b_ptr"]), S["n_b"], S["F"], ptr(at), ptr(bt), ptr(S["b_removed"]), ptr(mb),
                                               al.ctypes.data_as(C.c_void_p), acc["n_gt"], acc["n_tr"], ptr(acc["tp"]), ptr(acc["loca"]),
                                               ptr(acc["matches_count"]), ptr(ws), ws.numel(), stream_ptr()),
              "mpnhip_hota_alpha_accumulate")


def association(acc):
    """What the host needs of ``acc``, as host arrays: ``ass`` [19, 3] (the AssA, AssRe and AssPr numerators,
    ``mpnhip_hota_association``), ``tp`` [19] and ``loca`` [19]."""
    lib = capi.load()
    dev = acc["tp"].device
    with torch.cuda.device(dev):
        out = _buf(N_ALPHAS * 3, torch.float64, dev)
        need = lib.mpnhip_hota_workspace_bytes(0, 0, 0, acc["n_gt"], acc["n_tr"])
        ws = capi.workspace(need, dev, "hota_eval")
        check(lib.mpnhip_hota_association(ptr(acc["matches_count"]), ptr(acc["gt_count"]), ptr(acc["tr_count"]), acc["n_gt"], acc["n_tr"],
                                          ptr(out), ptr(ws), ws.numel(), stream_ptr()), "mpnhip_hota_association")
        return {"ass": out.cpu().numpy().reshape(N_ALPHAS, 3), "tp": acc["tp"].cpu().numpy(), "loca": acc["loca"].cpu().numpy()}


# ------------------------------------------------------------------------------------------------ the kit's bookkeeping (host)
def _compute_final_fields(res):
    """hota.py:166-179"""
    res["DetRe"] = res["HOTA_TP"] / np.maximum(1, res["HOTA_TP"] + res["HOTA_FN"])
    res["DetPr"] = res["HOTA_TP"] / np.maximum(1, res["HOTA_TP"] + res["HOTA_FP"])
    res["DetA"] = res["HOTA_TP"] / np.maximum(1, res["HOTA_TP"] + res["HOTA_FN"] + res["HOTA_FP"])
    res["HOTA"] = np.sqrt(res["DetA"] * res["AssA"])
    res["RHOTA"] = np.sqrt(res["DetRe"] * res["AssA"])
    res["HOTA(0)"] = res["HOTA"][0]
    res["LocA(0)"] = res["LocA"][0]
    res["HOTALocA(0)"] = res["HOTA(0)"] * res["LocA(0)"]
    return res


def hota_from_accumulators(tp, loca, ass, num_gt_dets, num_tracker_dets, num_gt_ids, num_tracker_ids):
    """The rest of ``HOTA.eval_sequence`` (hota.py:28-45, :103-117) from the sums of a sequence: ``tp`` [19], ``loca`` [19] (the
    sums of the matched similarities), ``ass`` [19, 3] (the AssA, AssRe and AssPr numerators; all three ignored when a side has
    no detection) and the four counts after preprocessing.  Returns TrackEval's fields (float64 arrays [19] and scalars) and
    the counts."""
    res = {f: np.zeros(N_ALPHAS, np.float64) for f in FLOAT_ARRAY_FIELDS + INTEGER_ARRAY_FIELDS}
    res.update({f: 0 for f in FLOAT_FIELDS})
    res.update(num_gt_dets=int(num_gt_dets), num_tracker_dets=int(num_tracker_dets), num_gt_ids=int(num_gt_ids),
               num_tracker_ids=int(num_tracker_ids))
    if num_tracker_dets == 0 or num_gt_dets == 0:   # :36-45
        res["HOTA_FN" if num_tracker_dets == 0 else "HOTA_FP"] = (num_gt_dets if num_tracker_dets == 0 else num_tracker_dets) * np.ones(N_ALPHAS)
        res["LocA"] = np.ones(N_ALPHAS, np.float64)
        res["LocA(0)"] = 1.0
        return res
    tp, ass = np.asarray(tp).astype(np.float64).reshape(N_ALPHAS), np.asarray(ass, np.float64).reshape(N_ALPHAS, 3)
    res["HOTA_TP"], res["HOTA_FN"], res["HOTA_FP"] = tp, num_gt_dets - tp, num_tracker_dets - tp
    res["AssA"], res["AssRe"], res["AssPr"] = (ass[:, j] / np.maximum(1, tp) for j in range(3))
    res["LocA"] = np.maximum(1e-10, np.asarray(loca, np.float64).reshape(N_ALPHAS)) / np.maximum(1e-10, tp)
    return _compute_final_fields(res)


def combine_hota(results):
    """``HOTA.combine_sequences`` (hota.py:119-129) over the results of several sequences -- the ``COMBINED_SEQ`` row the
    reference reports; the four counts are summed."""
    results = list(results)
    res = {f: sum(r[f] for r in results) for f in INTEGER_ARRAY_FIELDS + COUNT_FIELDS}
    for f in ("AssRe", "AssPr", "AssA"):
        res[f] = sum(r[f] * r["HOTA_TP"] for r in results) / np.maximum(1.0, res["HOTA_TP"])
    res["LocA"] = np.maximum(1e-10, sum(r["LocA"] * r["HOTA_TP"] for r in results)) / np.maximum(1e-10, res["HOTA_TP"])
    return _compute_final_fields(res)


def assign_frames(S, a_traj, b_traj, score):
    """The assignment of every frame of the launch ``S`` (hota.py:88) over its kept entries: ``match_b`` [n_a] (int64) -- the
    b-entry (index into the launch's list) chosen for every a-entry, or -1.  ``score``: the host array of ``frame_scores``."""
    from scipy.optimize import linear_sum_assignment
    a_traj, b_traj = np.asarray(a_traj).reshape(-1), np.asarray(b_traj).reshape(-1)
    match_b = np.full(S["n_a"], -1, np.int64)
    kept_b = (b_traj >= 0) & ~S["b_removed_host"]
    for f in range(S["F"]):
        a0, a1, b0, b1 = int(S["a_ptr"][f]), int(S["a_ptr"][f + 1]), int(S["b_ptr"][f]), int(S["b_ptr"][f + 1])
        rows, cols = np.flatnonzero(a_traj[a0:a1] >= 0), np.flatnonzero(kept_b[b0:b1])
        if rows.size and cols.size:
            cells = score[S["sim_ptr"][f]:S["sim_ptr"][f + 1]].reshape(a1 - a0, b1 - b0)
            r, c = linear_sum_assignment(-cells[rows][:, cols])
            match_b[a0 + rows[r]] = b0 + cols[c]
    return match_b


def assign_frames_device(S, a_traj, b_traj, score_dev):
    """``assign_frames`` without the host: ``match_b`` [n_a] (int32, device) from the device tensor of ``frame_scores``, one
    problem of ``assignment.linear_sum_assignment_batched`` per frame over the score block as it lies.  Nothing is read back here:
    the solver's status per frame stays on the device as ``S["assign_status"]`` ([F] int32; an unsolved frame has only -1 in
    ``match_b``) for ``check_assignment_status``."""
    from . import assignment
    dev = score_dev.device
    with torch.cuda.device(dev):
        at, bt = _traj(S, a_traj, b_traj, dev)
        match_b, _, status = assignment.linear_sum_assignment_batched(score_dev, S["_sim_ptr"], S["_a_ptr"], S["_b_ptr"], at >= 0,
                                                                      (bt >= 0) & (S["b_removed"] == 0), maximize=True)
        S["assign_status"] = status
    return match_b


def check_assignment_status(launches):
    """One read for a sequence: raises ``MpnhipError`` if ``assign_frames_device`` left a frame of the launches (dicts of
    ``frame_similarity``) unsolved -- more than ``assignment.MAX_SIDE`` kept entries on a side, scores that are not finite."""
    from . import assignment
    status = [S["assign_status"] for S in launches if S.get("assign_status") is not None]
    if status:
        assignment.raise_on_status(torch.cat(status), "hota_eval.assign_frames_device")


# ------------------------------------------------------------------------------------------------ sequences
def _check_frames(frames, num_timesteps, what):
    bad = np.unique(frames[(frames < 0) | (frames >= num_timesteps)])
    if bad.size:   # kitti_mots.py:194-204
        raise ValueError("%s data contains the following invalid timesteps: %s" % (what, ", ".join(str(int(v)) for v in bad)))


def _pass1(gt_rows, num_timesteps, class_id, ignore_class, frames_per_launch, device, b_frame, b_traj, b_ids, b_labels, img_shape, ops):
    """The first pass over the launches of a sequence for one class: the pixel work, the removals and the global alignment.
    Returns what every metric of the class consumes (``kitti_mots_eval`` shares it between HOTA, CLEAR and Identity): ``acc``
    (the accumulators), ``launches`` ([(S, a_traj, b_traj)], the similarity blocks on the device), ``counts`` (the kit's
    num_gt_dets, num_tracker_dets, num_gt_ids, num_tracker_ids after the preprocessing), ``b_traj`` and ``b_kept`` per b-entry."""
    _check_frames(gt_rows["frame"], num_timesteps, "Ground-truth")
    _check_frames(b_frame, num_timesteps, "Tracking")
    b_traj = np.asarray(b_traj, np.int64)
    a = _Side(gt_rows, np.isin(gt_rows["class_id"], (class_id, ignore_class)), (class_id,))
    a_size = _image_size(a)
    if img_shape is not None and a_size is not None and a_size != (int(img_shape[0]), int(img_shape[1])):
        raise ValueError("the ground truth's image size %s is not the prediction's %s" % (a_size, tuple(img_shape)))
    H, W = (int(v) for v in (img_shape if img_shape is not None else (a_size or (0, 0))))
    hw = H * W
    a_ignore = a.class_id == ignore_class
    acc = ops.accumulators(a.ids.size, int(np.asarray(b_ids).size), device)
    b_removed = np.zeros(b_frame.size, bool)
    frames = np.union1d(a.frame, b_frame)
    step = max(int(frames_per_launch), 1)
    launches = []
    for g0 in range(0, frames.size if hw else 0, step):
        fl = frames[g0:g0 + step]
        a_ptr, a_entries, (re_, rb, ren) = a.launch(fl)
        b_lo, b_hi = np.searchsorted(b_frame, fl, "left"), np.searchsorted(b_frame, fl, "right")
        b_ptr = np.concatenate(([0], np.cumsum(b_hi - b_lo))).astype(np.int64)
        b_entries = np.concatenate([np.arange(x, y) for x, y in zip(b_lo, b_hi)]).astype(np.int64)
        labels_a = ops.paint_label_runs(re_, rb, ren, a_ptr, a_entries.size, hw, device)
        labels_b = b_labels(fl, b_ptr, b_entries, hw).reshape(fl.size, hw)
        table, tp = ops.label_overlap(labels_a, labels_b, a_ptr, b_ptr)
        at, bt = a.traj[a_entries], b_traj[b_entries]
        S = ops.frame_similarity(table, tp, a_ptr, b_ptr, a_ignore[a_entries], bt >= 0)
        ops.accumulate_alignment(S, at, bt, acc)
        b_removed[b_entries] = S["b_removed_host"]
        launches.append((S, at, bt))
    b_kept = (b_traj >= 0) & ~b_removed
    counts = (int((a.traj >= 0).sum()), int(b_kept.sum()), int(a.ids.size), int(np.unique(b_traj[b_kept]).size))
    return {"acc": acc, "launches": launches, "counts": counts, "b_traj": b_traj, "b_kept": b_kept}


def _pass2(P, ops, assignment):
    """The second pass over the launches of ``_pass1``: the assignments and the counts per alpha; HOTA's fields."""
    acc, launches, counts = P["acc"], P["launches"], P["counts"]
    if counts[0] == 0 or counts[1] == 0:
        return hota_from_accumulators(None, None, None, *counts)
    for S, at, bt in launches:
        if assignment == "device":
            match_b = ops.assign_frames_device(S, at, bt, ops.frame_scores(S, at, bt, acc, host=False))
        else:
            match_b = assign_frames(S, at, bt, ops.frame_scores(S, at, bt, acc))
        ops.alpha_accumulate(S, at, bt, match_b, ALPHAS, acc)
    if assignment == "device":
        check_assignment_status([S for S, _, _ in launches])   # (before the sums are read: no silent fallback)
    out = ops.association(acc)
    return hota_from_accumulators(out["tp"], out["loca"], out["ass"], *counts)


def _check_assignment(assignment):
    if assignment not in ("host", "device"):
        raise ValueError("assignment is 'host' or 'device' (%r)" % (assignment,))


def _evaluate(gt_rows, num_timesteps, class_id, ignore_class, frames_per_launch, device, b_frame, b_traj, b_ids, b_labels,
              img_shape, details=False, ops=None, assignment="host"):
    """The two passes over the launches of a sequence.  The b-side as in ``mots_eval._evaluate``: its frames' entries
    (``b_frame`` ascending, ``b_traj``; -1: an entry that only occupies pixels) and ``b_labels(frames, b_ptr, b_entries, hw)``
    -> the label images of ascending ``frames``.  ``ops``: the operators (this module's and ``mots_eval``'s two; the tests' numpy
    restatements have no device to run on).  ``assignment``: ``'host'`` (``assign_frames``) or ``'device'``
    (``ops.assign_frames_device``)."""
    ops = ops or sys.modules[__name__]
    _check_assignment(assignment)
    P = _pass1(gt_rows, num_timesteps, class_id, ignore_class, frames_per_launch, device, b_frame, b_traj, b_ids, b_labels, img_shape, ops)
    res = _pass2(P, ops, assignment)
    if details:   # {frame: the prediction ids the preprocessing keeps, ascending}
        ids = np.asarray(b_ids, np.int64)
        res["kept_tracker_ids"] = {int(f): sorted(int(v) for v in ids[P["b_traj"][(b_frame == f) & P["b_kept"]]]) for f in np.unique(b_frame)}
    return res


def evaluate_hota_files(pred_txt, gt_txt, num_timesteps, class_id=CLASS_ID, ignore_class=IGNORE_CLASS, frames_per_launch=8,
                        device="cuda", details=False, _ops=None, assignment="host"):
    """``eval_kitti_mots`` for one sequence and one class: HOTA of the MOTS result file ``pred_txt`` against the ground truth
    ``gt_txt`` (paths, or what ``mots_eval.load_mots_txt`` returns) over the frames ``0 .. num_timesteps - 1``; a row of
    another frame is refused.  Ground-truth rows of ``class_id`` are the objects and those of ``ignore_class`` the frames'
    ignore regions; prediction rows of ``class_id`` are scored; every other row only occupies pixels.

    Returns TrackEval's fields: ``HOTA``, ``DetA``, ``AssA``, ``DetRe``, ``DetPr``, ``AssRe``, ``AssPr``, ``LocA``, ``RHOTA``,
    ``HOTA_TP``, ``HOTA_FN``, ``HOTA_FP`` (float64 [19], one per alpha of ``ALPHAS``), the scalars ``HOTA(0)``, ``LocA(0)``,
    ``HOTALocA(0)``, and ``num_gt_dets``, ``num_tracker_dets``, ``num_gt_ids``, ``num_tracker_ids`` after the preprocessing.
    ``frames_per_launch`` frames share a launch (the label workspace is 2 x 4 B x H x W x frames_per_launch; the similarity
    blocks of ALL launches stay on the device until the end, see the module's docstring), and the result does not depend on it.
    ``details``: also ``kept_tracker_ids`` ({frame: the prediction ids left after the preprocessing}).  ``assignment``: where
    the frames' assignment problems are solved -- ``'host'`` (scipy, the default) or ``'device'`` (``assign_frames_device``: no
    copy of score cells or matches; a frame with more than ``assignment.MAX_SIDE`` kept entries on a side raises); any other
    value is a ``ValueError``."""
    gt, pred = _as_loaded(gt_txt), _as_loaded(pred_txt)
    _check_frames(pred["frame"], num_timesteps, "Tracking")
    b = _Side(pred, pred["class_id"] == class_id, (class_id,))

    def b_labels(frames, b_ptr, b_entries, hw):
        _, entries, (re_, rb, ren) = b.launch(frames)
        return (_ops or sys.modules[__name__]).paint_label_runs(re_, rb, ren, b_ptr, entries.size, hw, device)
    return _evaluate(gt, num_timesteps, class_id, ignore_class, frames_per_launch, device, b.frame, b.traj, b.ids, b_labels,
                     _image_size(b), details, ops=_ops, assignment=assignment)
