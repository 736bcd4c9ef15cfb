"""The table ``TrackEval/scripts/run_kitti_mots.py`` prints by default, without leaving the device: HOTA, CLEAR, Identity and
Count for the classes car and pedestrian, per sequence, over all sequences (``COMBINED_SEQ``) and over the classes
(``cls_comb_cls_av``, ``cls_comb_det_av``) -- ``trackeval/eval.py:84-112`` with ``metrics/hota.py``, ``clear.py``,
``identity.py`` and ``count.py``, over the C ABI (``csrc/hota.hip``, ``csrc/clear_identity.hip``).

Each class of a sequence runs HOTA's first pass once (``hota_eval._pass1``: the pixel work, the predictions the preprocessing
removes, the alignment counts); the per-frame IoU blocks it leaves on the device are what all three metrics consume:

* HOTA: ``hota_eval._pass2``, the same bits as ``hota_eval.evaluate_hota_files``.
* Identity: ``identity_accumulate`` counts the potential matches ``[G, T]``.  The kit's ``(G + T) x (G + T)`` assignment with
  1e10 walls equals the rectangular problem "maximise the sum of the counts over a complete assignment of min(G, T) pairs" (a
  pair with count 0 costs what leaving both unmatched costs), solved with scipy on the table copied down once
  (``assignment='host'``) or with ``assignment.linear_sum_assignment_batched`` on the device (``'device'``; more than
  ``assignment.MAX_SIDE`` ids on a side raises); ``identity_sums`` reads IDTP off the table.
* CLEAR: among the disjoint masks of label images the per-frame assignment is degenerate -- a component of eligible cells is
  a single pair or a star of three entries (the argument is in ``clear_identity.hip``) -- so ``clear_frame_candidates`` finds the
  partners of every entry for all frames in parallel and ``clear_sequence_scan`` walks the frames in order.

One deliberate difference, beside HOTA's: a star WITHOUT continuity (an object split exactly in half by two predictions, or a
prediction that is exactly the union of two equal objects, none of them continuing the previous frame's match) is decided by
scipy's tie order in the kit and by list order here (the earlier entry wins).  It can change later IDSW / Frag, never
CLR_TP / CLR_FN / CLR_FP.

Out of scope: printing, summary files, plots, super categories, J&F."""
import sys

import numpy as np
import torch

from . import capi, hota_eval as HE
from .capi import MpnhipError, check, ptr, stream_ptr
from .hota_eval import (accumulate_alignment, accumulators, alpha_accumulate, assign_frames_device, association,  # noqa: F401
                        frame_scores, frame_similarity, label_overlap, paint_label_runs)
from .mots_eval import IGNORE_CLASS, _Side, _as_loaded, _buf, _i32, _image_size

CLASS_IDS = {"car": 1, "pedestrian": 2}   # kitti_mots.py:63
METRICS = ("HOTA", "CLEAR", "Identity")   # run_kitti_mots.py:52; Count is always evaluated (eval.py:38)
CLEAR_INTEGER_FIELDS = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag", "CLR_Frames")
CLEAR_FLOAT_FIELDS = ("MOTA", "MOTP", "MODA", "CLR_Re", "CLR_Pr", "MTR", "PTR", "MLR", "sMOTA", "CLR_F1", "FP_per_frame", "MOTAL", "MOTP_sum")
CLEAR_FIELDS = CLEAR_FLOAT_FIELDS + CLEAR_INTEGER_FIELDS
CLEAR_SUMMED_FIELDS = CLEAR_INTEGER_FIELDS + ("MOTP_sum",)
IDENTITY_INTEGER_FIELDS = ("IDTP", "IDFN", "IDFP")
IDENTITY_FLOAT_FIELDS = ("IDF1", "IDR", "IDP")
IDENTITY_FIELDS = IDENTITY_FLOAT_FIELDS + IDENTITY_INTEGER_FIELDS
COUNT_INTEGER_FIELDS = ("Dets", "GT_Dets", "IDs", "GT_IDs")
COUNT_FIELDS = COUNT_INTEGER_FIELDS + ("Frames",)
HOTA_FLOAT_FIELDS = HE.FLOAT_FIELDS + HE.FLOAT_ARRAY_FIELDS


# ------------------------------------------------------------------------------------------------ operators (device)
def _workspace(lib, S, n_gt, n_tr, dev):
    need = lib.mpnhip_clear_identity_workspace_bytes(S["n_a"], S["n_b"], S["F"], int(n_gt), int(n_tr))
    if need == 0:
        raise MpnhipError("%d x %d ids (2^31 cells or more) are not supported" % (n_gt, n_tr))
    return capi.workspace(need, dev, "kitti_mots_eval")


def _zeros(n, dtype, dev, fill=0):
    return torch.full((max(n, 1),), fill, dtype=dtype, device=dev)[:n]


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise MpnhipError("mpntrackseg_amd runs on a HIP device only (%s); there is no CPU fallback" % dev)
    return dev


def identity_accumulators(n_gt_ids, n_tr_ids, device):
    """The zeroed accumulator of a sequence's Identity metric: ``potential_count`` [G, T] (int32)."""
    dev, G, T = _device(device), int(n_gt_ids), int(n_tr_ids)
    if G * T >= 1 << 31:
        raise MpnhipError("a potential_count of %d x %d (2^31 cells or more) is not supported" % (G, T))
    return {"n_gt": G, "n_tr": T, "potential_count": _zeros(G * T, torch.int32, dev)}


def clear_accumulators(n_gt_ids, device):
    """The state of a sequence's CLEAR scan before its first launch: ``prev_tracker_id`` / ``prev_timestep_tracker_id`` [G]
    (int32, -1), ``gt_id_count`` / ``gt_matched_count`` / ``gt_frag_count`` [G] (int32, 0), ``counters`` [4] (int64: CLR_TP,
    CLR_FN, CLR_FP, IDSW), ``motp_sum`` [1] (float64) and the status words of its launches."""
    dev, G = _device(device), int(n_gt_ids)
    acc = {"n_gt": G, "counters": _zeros(4, torch.int64, dev), "motp_sum": _zeros(1, torch.float64, dev), "status": []}
    for k in ("prev_tracker_id", "prev_timestep_tracker_id"):
        acc[k] = _zeros(G, torch.int32, dev, -1)
    for k in ("gt_id_count", "gt_matched_count", "gt_frag_count"):
        acc[k] = _zeros(G, torch.int32, dev)
    return acc


def _sim_args(S):
    return (ptr(S["sim"]), S["sim_cells"], ptr(S["_sim_ptr"]), ptr(S["_a_ptr"]), S["n_a"], ptr(S["_b_ptr"]), S["n_b"], S["F"])


def identity_accumulate(S, a_traj, b_traj, acc):
    """+ the launch ``S`` (a dict of ``hota_eval.frame_similarity``) into ``acc``'s ``potential_count``
    (``mpnhip_identity_accumulate``)."""
    lib = capi.load()
    dev = S["sim"].device
    with torch.cuda.device(dev):
        at, bt = HE._traj(S, a_traj, b_traj, dev)
        check(lib.mpnhip_identity_accumulate(*_sim_args(S), ptr(at), ptr(bt), ptr(S["b_removed"]), acc["n_gt"], acc["n_tr"],
                                             ptr(acc["potential_count"]), stream_ptr()), "mpnhip_identity_accumulate")


def identity_table(acc):
    """``potential_count`` [G, T] as a host array: the one copy of ``assignment='host'``"""
    return acc["potential_count"].cpu().numpy().reshape(acc["n_gt"], acc["n_tr"])


def identity_assign_host(table):
    """The reduced Identity assignment on the host: ``match_b`` [G] (int32; the column chosen for every row of ``table``, or -1)
    of a complete assignment of min(G, T) pairs that maximises the sum of the counts."""
    from scipy.optimize import linear_sum_assignment
    table = np.asarray(table)
    match_b = np.full(table.shape[0], -1, np.int32)
    if table.size:
        r, c = linear_sum_assignment(table, maximize=True)
        match_b[r] = c
    return match_b


def identity_assign_device(acc):
    """The same on the device: one problem of ``assignment.linear_sum_assignment_batched`` over the table converted to float64
    where it lies.  ``match_b`` [G] (int32, device).  Raises ``MpnhipError`` if the solver refuses the problem (more than
    ``assignment.MAX_SIDE`` ids on a side): nothing falls back."""
    from . import assignment
    G, T = acc["n_gt"], acc["n_tr"]
    dev = acc["potential_count"].device
    with torch.cuda.device(dev):
        if G * T == 0:
            return _zeros(G, torch.int32, dev, -1)
        match_b, _, status = assignment.linear_sum_assignment_batched(acc["potential_count"].to(torch.float64), [0, G * T], [0, G], [0, T],
                                                                      maximize=True)
        assignment.raise_on_status(status, "kitti_mots_eval.identity_assign_device")
    return match_b


def identity_sums(acc, match_b):
    """IDTP (int) of the assignment ``match_b`` [G] (``mpnhip_identity_sums``): one read."""
    lib = capi.load()
    dev = acc["potential_count"].device
    with torch.cuda.device(dev):
        mb = _i32(match_b, dev)
        if mb.numel() != acc["n_gt"]:
            raise MpnhipError("one match per ground-truth id")
        out = _buf(1, torch.int64, dev)
        check(lib.mpnhip_identity_sums(ptr(acc["potential_count"]), ptr(mb), acc["n_gt"], acc["n_tr"], ptr(out), stream_ptr()),
              "mpnhip_identity_sums")
        return int(out.cpu()[0])


def clear_frame_candidates(S, a_traj, b_traj, n_gt_ids, n_tr_ids):
    """The candidates of the launch ``S`` (``mpnhip_clear_frame_candidates``): a dict with ``a_cand`` [n_a, 2], ``b_cand``
    [n_b, 2] (int32, device; entries of the other list or -1) and ``status`` [1] (int32, device; read by
    ``check_clear_status``)."""
    lib = capi.load()
    dev = S["sim"].device
    with torch.cuda.device(dev):
        at, bt = HE._traj(S, a_traj, b_traj, dev)
        C = {"a_cand": _buf(2 * S["n_a"], torch.int32, dev), "b_cand": _buf(2 * S["n_b"], torch.int32, dev),
             "status": _buf(1, torch.int32, dev)}
        check(lib.mpnhip_clear_frame_candidates(*_sim_args(S), ptr(at), ptr(bt), ptr(S["b_removed"]), int(n_gt_ids), int(n_tr_ids),
                                                ptr(C["a_cand"]), ptr(C["b_cand"]), ptr(C["status"]), stream_ptr()),
              "mpnhip_clear_frame_candidates")
    return C


def clear_sequence_scan(S, a_traj, b_traj, cand, n_tr_ids, acc):
    """The frames of the launch ``S`` in order into the state ``acc`` of ``clear_accumulators`` (``mpnhip_clear_sequence_scan``).
    ``cand``: the dict of ``clear_frame_candidates``.  Returns ``match_b`` [n_a] (int32, device)."""
    lib = capi.load()
    dev = S["sim"].device
    with torch.cuda.device(dev):
        at, bt = HE._traj(S, a_traj, b_traj, dev)
        ac, bc = _i32(cand["a_cand"], dev), _i32(cand["b_cand"], dev)
        if ac.numel() != 2 * S["n_a"] or bc.numel() != 2 * S["n_b"]:
            raise MpnhipError("two candidates per a-entry and per b-entry")
        ws = _workspace(lib, S, acc["n_gt"], n_tr_ids, dev)
        match_b = _buf(S["n_a"], torch.int32, dev)
        check(lib.mpnhip_clear_sequence_scan(*_sim_args(S), ptr(at), ptr(bt), ptr(S["b_removed"]), ptr(ac), ptr(bc), acc["n_gt"],
                                             int(n_tr_ids), ptr(acc["prev_tracker_id"]), ptr(acc["prev_timestep_tracker_id"]),
                                             ptr(acc["gt_id_count"]), ptr(acc["gt_matched_count"]), ptr(acc["gt_frag_count"]),
                                             ptr(acc["counters"]), ptr(acc["motp_sum"]), ptr(match_b), ptr(ws), ws.numel(), stream_ptr()),
              "mpnhip_clear_sequence_scan")
        if cand.get("status") is not None:
            acc["status"].append(cand["status"])
    return match_b


def check_clear_status(status):
    """Raises ``MpnhipError`` if a status word of ``clear_frame_candidates`` (a list of them) is not 0: an entry with three or more
    eligible partners, or a component larger than a star -- masks that overlap on one side, not label images."""
    status = list(status)
    if status and all(isinstance(s, torch.Tensor) for s in status):
        status = [torch.cat([s.view(-1) for s in status]).cpu().numpy()]   # one read for the sequence
    st = np.concatenate([np.asarray(s).reshape(-1) for s in status]) if status else np.zeros(0, int)
    bad = np.flatnonzero(st)
    if bad.size:
        raise MpnhipError("clear_frame_candidates: launch %d of %d: status %d (bit 0: an entry with three or more eligible partners, "
                          "bit 1: a component larger than a star): the masks of a side overlap" % (bad[0], st.size, st[bad[0]]))


def clear_track_summary(acc):
    """What the host needs of a sequence's CLEAR state, as host values (one read after ``mpnhip_clear_track_summary``):
    ``CLR_TP``, ``CLR_FN``, ``CLR_FP``, ``IDSW``, ``MT``, ``PT``, ``ML``, ``Frag`` (int) and ``MOTP_sum`` (float).  Raises where a
    launch's candidates were refused."""
    lib = capi.load()
    dev = acc["counters"].device
    with torch.cuda.device(dev):
        out = _buf(4, torch.int64, dev)
        check(lib.mpnhip_clear_track_summary(ptr(acc["gt_id_count"]), ptr(acc["gt_matched_count"]), ptr(acc["gt_frag_count"]), acc["n_gt"],
                                             ptr(out), stream_ptr()), "mpnhip_clear_track_summary")
        check_clear_status(acc["status"])
        ints = torch.cat((acc["counters"], out)).cpu().numpy()
        res = {k: int(v) for k, v in zip(("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag"), ints)}
        res["MOTP_sum"] = float(acc["motp_sum"].cpu()[0])
    return res


# ------------------------------------------------------------------------------------------------ the kit's bookkeeping (host)
def _clear_final_fields(res):
    """clear.py:166-185"""
    num_gt_ids = res["MT"] + res["ML"] + res["PT"]
    res["MTR"] = res["MT"] / np.maximum(1.0, num_gt_ids)
    res["MLR"] = res["ML"] / np.maximum(1.0, num_gt_ids)
    res["PTR"] = res["PT"] / np.maximum(1.0, num_gt_ids)
    res["CLR_Re"] = res["CLR_TP"] / np.maximum(1.0, res["CLR_TP"] + res["CLR_FN"])
    res["CLR_Pr"] = res["CLR_TP"] / np.maximum(1.0, res["CLR_TP"] + res["CLR_FP"])
    res["MODA"] = (res["CLR_TP"] - res["CLR_FP"]) / np.maximum(1.0, res["CLR_TP"] + res["CLR_FN"])
    res["MOTA"] = (res["CLR_TP"] - res["CLR_FP"] - res["IDSW"]) / np.maximum(1.0, res["CLR_TP"] + res["CLR_FN"])
    res["MOTP"] = res["MOTP_sum"] / np.maximum(1.0, res["CLR_TP"])
    res["sMOTA"] = (res["MOTP_sum"] - res["CLR_FP"] - res["IDSW"]) / np.maximum(1.0, res["CLR_TP"] + res["CLR_FN"])
    res["CLR_F1"] = res["CLR_TP"] / np.maximum(1.0, res["CLR_TP"] + 0.5 * res["CLR_FN"] + 0.5 * res["CLR_FP"])
    res["FP_per_frame"] = res["CLR_FP"] / np.maximum(1.0, res["CLR_Frames"])
    safe_log_idsw = np.log10(res["IDSW"]) if res["IDSW"] > 0 else res["IDSW"]
    res["MOTAL"] = (res["CLR_TP"] - res["CLR_FP"] - safe_log_idsw) / np.maximum(1.0, res["CLR_TP"] + res["CLR_FN"])
    return res


def _identity_final_fields(res):
    """identity.py:128-135"""
    res["IDR"] = res["IDTP"] / np.maximum(1.0, res["IDTP"] + res["IDFN"])
    res["IDP"] = res["IDTP"] / np.maximum(1.0, res["IDTP"] + res["IDFP"])
    res["IDF1"] = res["IDTP"] / np.maximum(1.0, res["IDTP"] + 0.5 * res["IDFP"] + 0.5 * res["IDFN"])
    return res


def clear_from_sums(sums, num_gt_dets, num_tracker_dets, num_gt_ids, num_timesteps):
    """``CLEAR.eval_sequence`` around the frame loop (clear.py:40-53, :122-127): the early returns when a side has no detection
    (``sums`` is not looked at), else the final fields from the sums of ``clear_track_summary``."""
    res = {f: 0 for f in CLEAR_FIELDS}
    if num_tracker_dets == 0:
        res.update(CLR_FN=int(num_gt_dets), ML=int(num_gt_ids), MLR=1.0)
        return res
    if num_gt_dets == 0:
        res.update(CLR_FP=int(num_tracker_dets), MLR=1.0)
        return res
    res.update(sums)
    res["CLR_Frames"] = int(num_timesteps)
    return _clear_final_fields(res)


def identity_from_sums(idtp, num_gt_dets, num_tracker_dets):
    """``Identity.eval_sequence`` around the assignment (identity.py:35-45, :83-88).  ``idtp``: None where a side is empty."""
    res = {f: 0 for f in IDENTITY_FIELDS}
    if num_tracker_dets == 0:
        res["IDFN"] = int(num_gt_dets)
        return res
    if num_gt_dets == 0:
        res["IDFP"] = int(num_tracker_dets)
        return res
    res.update(IDTP=int(idtp), IDFN=int(num_gt_dets) - int(idtp), IDFP=int(num_tracker_dets) - int(idtp))
    return _identity_final_fields(res)


def _combine_sum(results, field):
    return sum(r[field] for r in results)


def _combine_metric(name, results, how):
    """one metric's ``combine_sequences`` / ``combine_classes_det_averaged`` (how = 'sum') or ``combine_classes_class_averaged``
    with ignore_empty_classes=False (how = 'mean') over a list of its results"""
    mean = lambda fields: {f: np.mean([r[f] for r in results], axis=0) for f in fields}
    if name == "HOTA":
        if how == "sum":   # hota.py:119-129, :153-163
            return HE.combine_hota(results)
        res = {f: _combine_sum(results, f) for f in HE.INTEGER_ARRAY_FIELDS + HE.COUNT_FIELDS}   # hota.py:131-151
        res.update(mean(HOTA_FLOAT_FIELDS))
        return res
    if name == "CLEAR":
        if how == "sum":   # clear.py:130-144
            return _clear_final_fields({f: _combine_sum(results, f) for f in CLEAR_SUMMED_FIELDS})
        res = {f: _combine_sum(results, f) for f in CLEAR_INTEGER_FIELDS}   # clear.py:146-163
        res.update(mean(CLEAR_FLOAT_FIELDS))
        return res
    if name == "Identity":
        if how == "sum":   # identity.py:111-125
            return _identity_final_fields({f: _combine_sum(results, f) for f in IDENTITY_INTEGER_FIELDS})
        res = {f: _combine_sum(results, f) for f in IDENTITY_INTEGER_FIELDS}   # identity.py:91-109
        res.update(mean(IDENTITY_FLOAT_FIELDS))
        return res
    if name == "Count":    # count.py:25-44 (Frames is not combined)
        return {f: _combine_sum(results, f) for f in COUNT_INTEGER_FIELDS}
    raise ValueError("unknown metric %r" % (name,))


def _combine(results, how):
    results = list(results.values()) if isinstance(results, dict) else list(results)
    if not results:
        raise ValueError("nothing to combine")
    return {name: _combine_metric(name, [r[name] for r in results], how) for name in results[0]}


def combine_sequences(results):
    """``combine_sequences`` of every metric over the sequences of one class: ``results`` = {seq: {metric: fields}} (or a list of
    the inner dicts) -> {metric: fields}, the ``COMBINED_SEQ`` row."""
    return _combine(results, "sum")


def combine_classes_class_averaged(results):
    """``combine_classes_class_averaged`` (ignore_empty_classes=False) of every metric: {cls: {metric: fields}} -> {metric: fields},
    the ``cls_comb_cls_av`` row: integer fields summed, float fields averaged over the classes."""
    return _combine(results, "mean")


def combine_classes_det_averaged(results):
    """``combine_classes_det_averaged`` of every metric: {cls: {metric: fields}} -> {metric: fields}, the ``cls_comb_det_av`` row."""
    return _combine(results, "sum")


# ------------------------------------------------------------------------------------------------ sequences
def _check_names(classes, metrics):
    classes, metrics = tuple(classes), tuple(metrics)
    for c in classes:
        if c not in CLASS_IDS:
            raise ValueError("class %r: KITTI-MOTS has %s" % (c, ", ".join(sorted(CLASS_IDS))))
    for m in metrics:
        if m not in METRICS:
            raise ValueError("metric %r: one of %s (Count is always evaluated)" % (m, ", ".join(METRICS)))
    return classes, metrics


def _class_metrics(P, metrics, num_timesteps, ops, assignment):
    """every requested metric of one class from its first pass ``P``"""
    acc, launches = P["acc"], P["launches"]
    n_gt_dets, n_tr_dets, n_gt_ids, n_tr_ids = P["counts"]
    G, T = acc["n_gt"], acc["n_tr"]
    dev = acc["potential"].device if isinstance(acc["potential"], torch.Tensor) else None
    empty = n_gt_dets == 0 or n_tr_dets == 0
    out = {}
    if "HOTA" in metrics:
        out["HOTA"] = HE._pass2(P, ops, assignment)
    if "CLEAR" in metrics:
        sums = None
        if not empty:
            state = ops.clear_accumulators(G, dev)
            for S, at, bt in launches:
                ops.clear_sequence_scan(S, at, bt, ops.clear_frame_candidates(S, at, bt, G, T), T, state)
            sums = ops.clear_track_summary(state)
        out["CLEAR"] = clear_from_sums(sums, n_gt_dets, n_tr_dets, n_gt_ids, num_timesteps)
    if "Identity" in metrics:
        idtp = None
        if not empty:
            table = ops.identity_accumulators(G, T, dev)
            for S, at, bt in launches:
                ops.identity_accumulate(S, at, bt, table)
            match_b = ops.identity_assign_device(table) if assignment == "device" else identity_assign_host(ops.identity_table(table))
            idtp = ops.identity_sums(table, match_b)
        out["Identity"] = identity_from_sums(idtp, n_gt_dets, n_tr_dets)
    out["Count"] = {"Dets": n_tr_dets, "GT_Dets": n_gt_dets, "IDs": n_tr_ids, "GT_IDs": n_gt_ids, "Frames": int(num_timesteps)}
    return out


def _evaluate_classes(gt_rows, num_timesteps, classes, metrics, frames_per_launch, device, b_side, ops, assignment):
    """``b_side(class_id)`` -> the b-side of ``hota_eval._pass1`` for the class: (b_frame, b_traj, b_ids, b_labels, img_shape)"""
    ops = ops or sys.modules[__name__]
    HE._check_assignment(assignment)
    classes, metrics = _check_names(classes, metrics)
    out = {}
    for cls in classes:
        b_frame, b_traj, b_ids, b_labels, img_shape = b_side(CLASS_IDS[cls])
        P = HE._pass1(gt_rows, num_timesteps, CLASS_IDS[cls], IGNORE_CLASS, frames_per_launch, device, b_frame, b_traj, b_ids, b_labels,
                      img_shape, ops)
        out[cls] = _class_metrics(P, metrics, num_timesteps, ops, assignment)
    return out


def evaluate_sequence_files(pred_txt, gt_txt, num_timesteps, classes=("car", "pedestrian"), metrics=METRICS, frames_per_launch=8,
                            device="cuda", assignment="host", _ops=None):
    """``eval_sequence`` of ``trackeval/eval.py`` for one KITTI-MOTS sequence: the MOTS result file ``pred_txt`` against the
    ground truth ``gt_txt`` (paths, or what ``mots_eval.load_mots_txt`` returns) over the frames ``0 .. num_timesteps - 1``.

    Returns ``{cls: {'HOTA': {...}, 'CLEAR': {...}, 'Identity': {...}, 'Count': {...}}}`` with the requested ``metrics`` (Count
    always): HOTA's fields as ``hota_eval.evaluate_hota_files``, every name of ``CLEAR_FIELDS``, ``IDENTITY_FIELDS`` and
    ``COUNT_FIELDS``.  ``frames_per_launch`` and ``assignment`` ('host' or 'device': where HOTA's per-frame problems and
    Identity's one problem are solved) as ``hota_eval.evaluate_hota_files``; the result does not depend on the former."""
    gt, pred = _as_loaded(gt_txt), _as_loaded(pred_txt)
    HE._check_frames(pred["frame"], num_timesteps, "Tracking")
    ops = _ops or sys.modules[__name__]

    def b_side(class_id):
        b = _Side(pred, pred["class_id"] == class_id, (class_id,))

        def b_labels(frames, b_ptr, b_entries, hw):
            _, entries, (re_, rb, ren) = b.launch(frames)
            return ops.paint_label_runs(re_, rb, ren, b_ptr, entries.size, hw, device)
        return b.frame, b.traj, b.ids, b_labels, _image_size(b)
    return _evaluate_classes(gt, num_timesteps, classes, metrics, frames_per_launch, device, b_side, ops, assignment)


def eval_kitti_mots(sequences, classes=("car", "pedestrian"), metrics=METRICS, frames_per_launch=8, device="cuda", assignment="host",
                    _ops=None):
    """``Evaluator.evaluate`` for one tracker (eval.py:84-112): ``sequences`` = {seq: (pred_txt, gt_txt, num_timesteps)}.  Returns
    ``res[seq][cls][metric]`` for every sequence, ``res['COMBINED_SEQ'][cls][metric]`` and
    ``res['COMBINED_SEQ']['cls_comb_cls_av' | 'cls_comb_det_av'][metric]``."""
    if "COMBINED_SEQ" in sequences:
        raise ValueError("'COMBINED_SEQ' is not a sequence name")
    classes, metrics = _check_names(classes, metrics)
    res = {seq: evaluate_sequence_files(pred, gt, T, classes, metrics, frames_per_launch, device, assignment, _ops)
           for seq, (pred, gt, T) in sorted(sequences.items())}
    seqs = list(res)
    combined = {cls: combine_sequences([res[seq][cls] for seq in seqs]) for cls in classes}
    per_class = dict(combined)
    combined["cls_comb_cls_av"] = combine_classes_class_averaged(per_class)
    combined["cls_comb_det_av"] = combine_classes_det_averaged(per_class)
    res["COMBINED_SEQ"] = combined
    return res
