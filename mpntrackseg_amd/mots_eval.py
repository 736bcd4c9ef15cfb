"""MOTS metrics (sMOTSA, MOTSA, MOTSP, IDF1, ...) of a tracked sequence: host mirror of ``compute_mots_metrics`` (reference
``src/mot_neural_solver/utils/evaluation.py:87-102``), i.e. ``MOTSMetrics.compute_metrics_per_sequence`` and ``compute_clearmot`` of
the vendored evaluation kit (``MOTChallengeEvalKit/src/MOTChallengeEvalKit/MOTS/MOTS_metrics.py``), over the C ABI
(``csrc/mots_eval.hip``).

The kit decodes one run-length mask per object with ``pycocotools`` and intersects every pair of a frame.  Masks of one MOTS
frame are disjoint (the kit's ``load_txt`` refuses anything else, ``mots_common/io.py:57-62``), so here a frame is one int32 label
per pixel on either side (the images of ``masks.py``), all intersections of a frame are one joint histogram of two label images
(``label_overlap``), and the kit's decisions are integer comparisons on that small table (``frame_match``).  What reaches the host
is a handful of integers per object; ``metrics_from_matches`` -- numpy and scipy, no device -- does the kit's bookkeeping from
them.  ``pycocotools`` is not needed.

One deliberate difference: a ground-truth and a predicted mask that are BOTH empty have IoU 0 / 0 = NaN in the kit, which its
IDF1 part counts as a match (``NaN < 0.5`` is false, ``MOTS_metrics.py:529``); here such a pair matches nowhere."""
import ctypes as C
import sys

import numpy as np
import torch

from . import capi, masks as M
from .capi import MpnhipError, check, ptr, stream_ptr

CLASS_ID, IGNORE_CLASS = 2, 10   # MOTS_metrics.py:12-13: pedestrians only


# ------------------------------------------------------------------------------------------------ text files (host)
def load_mots_txt(path, device=None):
    """The rows ``frame id class img_height img_width rle`` of a MOTS text file as arrays, refusing what the kit's ``load_txt``
    (``mots_common/io.py:31-69``) refuses: two rows of one id in a frame, a class other than 1 / 2 / 10, overlapping masks in a
    frame.  Returns a dict: ``frame``, ``track_id``, ``class_id``, ``h``, ``w`` (int64 [n], file order) and the masks as runs of
    set pixels -- ``run_row``, ``run_begin``, ``run_end`` (row of the file and positions ``x * h + y`` in COCO's column-major
    order; sorted by row, then position) -- and ``area`` [n].

    ``device``: decode the strings there, all rows in two launches (``masks.rle_decode_batch``), instead of one numpy decode per
    row; the host still splits the lines.  The same dict and the same refusals, with the same text."""
    if device is not None:
        return _load_mots_txt_device(path, device)
    frame, tid, cls, hs, ws, rr, rb, re_ = [], [], [], [], [], [], [], []
    seen = set()
    with open(path, "r") as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            fields = line.split(" ")
            try:
                fr, ti, ci, h, w = (int(v) for v in fields[:5])
                counts = M.rle_counts(fields[5])
            except (ValueError, IndexError):
                raise ValueError("Error in %s in line: %s" % (str(path).split("/")[-1], line))
            if (fr, ti) in seen:
                raise ValueError("Multiple objects with track id %d in frame %d" % (ti, fr))
            seen.add((fr, ti))
            if ci not in (1, 2, 10):
                raise ValueError("Unknown object class %d" % ci)
            if h < 0 or w < 0 or (counts.size and counts.min() < 0) or int(counts.sum()) != h * w:
                raise ValueError("the counts of track id %d in frame %d do not describe a %d x %d mask" % (ti, fr, h, w))
            b, e = counts_to_runs(counts)
            rr.append(np.full(b.size, len(frame), np.int64))
            rb.append(b)
            re_.append(e)
            frame.append(fr); tid.append(ti); cls.append(ci); hs.append(h); ws.append(w)
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    out = {"frame": np.asarray(frame, np.int64), "track_id": np.asarray(tid, np.int64), "class_id": np.asarray(cls, np.int64),
           "h": np.asarray(hs, np.int64), "w": np.asarray(ws, np.int64), "run_row": cat(rr), "run_begin": cat(rb), "run_end": cat(re_)}
    out["area"] = np.bincount(out["run_row"], weights=out["run_end"] - out["run_begin"], minlength=len(frame)).astype(np.int64)
    refuse_overlapping_masks(out["frame"], out["run_row"], out["run_begin"], out["run_end"])
    return out


def first_refused_row(frame, track_id, class_id, h, w, status):
    """Which row of a file ``load_mots_txt`` refuses, and why, from the rows' integers and the decoder's status words
    (``masks.RLE_*``): ``(row, reason)`` of the first bad row in file order, or None.  Inside a row the loader's order: ``'parse'``
    (a string ``rle_counts`` does not read), ``'duplicate'`` (the id occurred in the frame before), ``'class'`` (not 1 / 2 / 10),
    ``'counts'`` (a negative size or count, or counts that do not sum to ``h * w``).  Pure host arithmetic."""
    frame, track_id, class_id, h, w, status = (np.asarray(v, np.int64).reshape(-1) for v in (frame, track_id, class_id, h, w, status))
    n = frame.size
    if n == 0:
        return None
    parse = (status & M.RLE_UNREADABLE) != 0
    order = np.lexsort((np.arange(n), track_id, frame))   # the rows of one (frame, id) side by side, in file order
    same = (frame[order][1:] == frame[order][:-1]) & (track_id[order][1:] == track_id[order][:-1])
    duplicate = np.zeros(n, bool)
    duplicate[order[1:][same]] = True
    unknown = ~np.isin(class_id, (1, 2, 10))
    counts = (h < 0) | (w < 0) | ((status & (M.RLE_NEGATIVE | M.RLE_BAD_SUM)) != 0)
    bad = np.flatnonzero(parse | duplicate | unknown | counts)
    if bad.size == 0:
        return None
    r = int(bad[0])
    return r, ("parse" if parse[r] else "duplicate" if duplicate[r] else "class" if unknown[r] else "counts")


def _split_mots_rows(path):
    """The host's share of the device ``load_mots_txt``: ``(ints [n, 5], strings, lines, unreadable)`` of the rows up to the first
    one the host alone refuses (fewer than six fields, an integer or a string that is none) -- ``unreadable``: that line, or None"""
    ints, strings, lines = [], [], []
    unreadable = None
    with open(path, "r") as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            fields = line.split(" ")
            try:
                row = [int(v) for v in fields[:5]]
                if len(row) < 5 or not fields[5].isascii():
                    raise ValueError
            except (ValueError, IndexError):
                unreadable = line
                break
            ints.append(row)
            strings.append(fields[5])
            lines.append(line)
    return np.asarray(ints, np.int64).reshape(-1, 5), strings, lines, unreadable


def _load_mots_txt_device(path, device):
    """``load_mots_txt`` with the strings decoded on the device.  The rows behind a line the host cannot split are not looked
    at: they cannot be refused before it."""
    cols, strings, lines, unreadable = _split_mots_rows(path)
    frame, tid, cls, hs, ws = (np.ascontiguousarray(cols[:, k]) for k in range(5))
    dec = M.rle_decode_batch(strings, hs, ws, device)
    refused = first_refused_row(frame, tid, cls, hs, ws, dec["status"])
    if refused is not None:
        r, why = refused
        if why == "parse":
            raise ValueError("Error in %s in line: %s" % (str(path).split("/")[-1], lines[r]))
        if why == "duplicate":
            raise ValueError("Multiple objects with track id %d in frame %d" % (tid[r], frame[r]))
        if why == "class":
            raise ValueError("Unknown object class %d" % cls[r])
        raise ValueError("the counts of track id %d in frame %d do not describe a %d x %d mask" % (tid[r], frame[r], hs[r], ws[r]))
    if unreadable is not None:
        raise ValueError("Error in %s in line: %s" % (str(path).split("/")[-1], unreadable))
    runs = torch.stack((dec["run_row"], dec["run_begin"], dec["run_end"])).cpu().numpy().astype(np.int64)
    out = {"frame": frame, "track_id": tid, "class_id": cls, "h": hs, "w": ws, "run_row": runs[0], "run_begin": runs[1], "run_end": runs[2],
           "area": dec["area"].astype(np.int64)}
    refuse_overlapping_masks(out["frame"], out["run_row"], out["run_begin"], out["run_end"])
    return out


def counts_to_runs(counts):
    """``(begin, end)`` of the runs of set pixels of COCO's ``counts`` (positions ``x * h + y``), empty runs left out"""
    edges = np.cumsum(counts)
    b, e = edges[0::2][:edges.size // 2], edges[1::2]
    keep = e > b
    return b[keep], e[keep]


def refuse_overlapping_masks(frame, run_row, run_begin, run_end):
    """``ValueError`` where two masks of one frame share a pixel: sort the frame's runs by their begin; two neighbours overlap iff
    the later begins before the earlier ends"""
    run_frame = frame[run_row]
    order = np.lexsort((run_begin, run_frame))
    f_s, b_s, e_s = run_frame[order], run_begin[order], run_end[order]
    bad = np.flatnonzero((f_s[1:] == f_s[:-1]) & (b_s[1:] < e_s[:-1]))
    if bad.size:
        raise ValueError("Objects with overlapping masks in frame %d" % int(f_s[bad[0]]))


# ------------------------------------------------------------------------------------------------ operators (device)
def _i32(v, dev):
    if isinstance(v, torch.Tensor):
        return v.to(device=dev, dtype=torch.int32).contiguous().view(-1)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.int32)).to(dev)


def _buf(n, dtype, dev):
    return torch.empty(max(int(n), 1), dtype=dtype, device=dev)[:int(n)]


def table_offsets(a_ptr, b_ptr):
    """``table_ptr`` [F + 1] (int64, host) of two lists: frame f owns ``(na_f + 1) * (nb_f + 1)`` cells."""
    a, b = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    if a.size != b.size or a.size < 1:
        raise MpnhipError("a_ptr and b_ptr need one entry per frame plus one")
    return np.concatenate(([0], np.cumsum((np.diff(a) + 1) * (np.diff(b) + 1)))).astype(np.int64)


def paint_label_runs(run_entry, run_begin, run_end, frame_ptr, n_entries, hw, device):
    """``labels`` [F, hw] int32 on ``device``: -1, then ``run_entry[r]`` over ``[run_begin[r], run_end[r])`` of the entry's frame
    (``mpnhip_paint_label_runs``).  The runs are host arrays or device tensors."""
    lib = capi.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise MpnhipError("mpntrackseg_amd runs on a HIP device only (%s); there is no CPU fallback" % dev)
    with torch.cuda.device(dev):
        e, b, en, fp = _i32(run_entry, dev), _i32(run_begin, dev), _i32(run_end, dev), _i32(frame_ptr, dev)
        if not (e.numel() == b.numel() == en.numel()):
            raise MpnhipError("one entry, begin and end per run")
        F, n, hw = int(fp.numel()) - 1, int(e.numel()), int(hw)
        if F < 0:
            raise MpnhipError("frame_ptr needs at least one entry")
        labels = _buf(F * hw, torch.int32, dev).view(F, hw)
        ws = capi.workspace(lib.mpnhip_mots_workspace_bytes(n, int(n_entries), 0, F, hw), dev, "mots_eval")
        check(lib.mpnhip_paint_label_runs(ptr(e), ptr(b), ptr(en), n, ptr(fp), int(n_entries), F, hw, ptr(labels), ptr(ws), ws.numel(),
                                          stream_ptr()), "mpnhip_paint_label_runs")
    return labels


@capi.on_tensor_device
def label_overlap(labels_a, labels_b, a_ptr, b_ptr):
    """The joint histogram of two label images [F, ...] (int32, device) of the same frames: ``(table, table_ptr)`` -- the int32
    cells on the device and the int64 offsets as a host array (``mpnhip_label_overlap``)."""
    lib = capi.load()
    capi.require_device(labels_a, labels_b)
    if labels_a.dtype != torch.int32 or labels_b.dtype != torch.int32 or labels_a.shape != labels_b.shape or labels_a.dim() < 1:
        raise MpnhipError("two int32 label images of one shape [F, ...]")
    la, lb, dev = labels_a.contiguous(), labels_b.contiguous(), labels_a.device
    F = int(la.shape[0])
    hw = int(la.numel() // F) if F else 0
    ap, bp = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    if ap.size != F + 1 or bp.size != F + 1:
        raise MpnhipError("a_ptr and b_ptr need %d entries for %d frames" % (F + 1, F))
    tp = table_offsets(ap, bp)
    cells = int(tp[-1])
    if cells >= 1 << 31:
        raise MpnhipError("a table of %d cells (2^31 or more) is not supported: fewer frames per launch" % cells)
    table = _buf(cells, torch.int32, dev)
    tp_dev, ap_dev, bp_dev = torch.from_numpy(tp).to(dev), _i32(ap, dev), _i32(bp, dev)   # (named: they live until the call returns)
    check(lib.mpnhip_label_overlap(ptr(la), ptr(lb), ptr(ap_dev), int(ap[-1]), ptr(bp_dev), int(bp[-1]), ptr(tp_dev),
                                   tp.ctypes.data_as(C.c_void_p), F, hw, ptr(table), cells, stream_ptr()), "mpnhip_label_overlap")
    return table, tp


@capi.on_tensor_device
def frame_match(table, table_ptr, a_ptr, b_ptr, a_ignore, a_traj, b_traj, n_a_traj, n_b_traj):
    """The kit's per-object decisions from a table (``mpnhip_mots_frame_match``), as host arrays: a dict with ``match_b``,
    ``inter``, ``uni`` [n_a], ``b_matched``, ``b_ignored`` (bool), ``b_area`` [n_b] and ``id_match`` [n_a_traj, n_b_traj]."""
    lib = capi.load()
    capi.require_device(table)
    dev = table.device
    ap, bp = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    tp = np.ascontiguousarray(np.asarray(table_ptr, np.int64).reshape(-1))
    F, n_a, n_b, na_t, nb_t = ap.size - 1, int(ap[-1]), int(bp[-1]), int(n_a_traj), int(n_b_traj)
    if bp.size != F + 1 or tp.size != F + 1:
        raise MpnhipError("a_ptr, b_ptr and table_ptr need one entry per frame plus one")
    if na_t * nb_t >= 1 << 31:
        raise MpnhipError("an id_match of %d x %d (2^31 cells or more) is not supported" % (na_t, nb_t))
    ign = torch.from_numpy(np.ascontiguousarray(np.asarray(a_ignore).reshape(-1), dtype=np.uint8)).to(dev)
    at, bt = _i32(a_traj, dev), _i32(b_traj, dev)
    if ign.numel() != n_a or at.numel() != n_a or bt.numel() != n_b:
        raise MpnhipError("one ignore flag and trajectory per a-entry, one trajectory per b-entry")
    a_out = _buf(3 * n_a, torch.int32, dev).view(3, n_a)
    b_flags = _buf(2 * n_b, torch.uint8, dev).view(2, n_b)
    b_area = _buf(n_b, torch.int32, dev)
    idm = _buf(na_t * nb_t, torch.int32, dev)
    ws = capi.workspace(lib.mpnhip_mots_workspace_bytes(0, n_a, n_b, F, 0), dev, "mots_eval")
    tp_dev, ap_dev, bp_dev = torch.from_numpy(tp).to(dev), _i32(ap, dev), _i32(bp, dev)   # (named: they live until the call returns)
    check(lib.mpnhip_mots_frame_match(ptr(table), int(tp[-1]), ptr(tp_dev), ptr(ap_dev), n_a, ptr(bp_dev), n_b, F, ptr(ign), ptr(at), ptr(bt), na_t, nb_t, ptr(a_out[0]), ptr(a_out[1]),
                                      ptr(a_out[2]), ptr(b_flags[0]), ptr(b_flags[1]), ptr(b_area), ptr(idm), ptr(ws), ws.numel(),
                                      stream_ptr()), "mpnhip_mots_frame_match")
    a_h, f_h = a_out.cpu().numpy(), b_flags.cpu().numpy()
    return {"match_b": a_h[0].copy(), "inter": a_h[1].copy(), "uni": a_h[2].copy(), "b_matched": f_h[0].astype(bool),
            "b_ignored": f_h[1].astype(bool), "b_area": b_area.cpu().numpy(), "id_match": idm.cpu().numpy().reshape(na_t, nb_t)}


# ------------------------------------------------------------------------------------------------ the kit's bookkeeping (host)
METRIC_NAMES = ("sMOTSA", "MOTSA", "MOTSP", "MOTSAL", "MODSA", "MODSP", "IDF1", "IDTP", "MT", "PT", "ML", "MTR", "PTR", "MLR",
                "n_gt_trajectories", "tp", "fp", "fn", "recall", "precision", "F1", "FAR", "total_cost", "fragments", "fragments_rel",
                "id_switches", "id_switches_rel", "n_tr_trajectories", "total_num_frames", "n_gt", "n_tr", "n_itr", "id_n_tr", "nbox_gt")


def metrics_from_matches(a_frame, a_traj, a_ignore, a_match_b, a_inter, a_uni, b_frame, b_traj, b_matched, b_ignored, id_match,
                         seq_length, details=False):
    """The rest of ``compute_metrics_per_sequence`` and ``compute_clearmot`` (``MOTS_metrics.py:182-382``, ``:85-159``) from the
    per-entry results of every launch, concatenated in (frame, file row) order.

    a-side [n_a]: ``a_frame``, ``a_traj`` (index of the entry's ground-truth trajectory, -1 for ignore entries), ``a_ignore``,
    ``a_match_b`` (index into the b-side arrays, or -1), ``a_inter``, ``a_uni``.  b-side [n_b]: ``b_frame``, ``b_traj``,
    ``b_matched``, ``b_ignored``.  ``id_match`` [n_gt_trajectories, n_tr_trajectories] summed over the launches.  Frames lie in
    ``[0, seq_length]``.  Returns the dict of the kit's registered metrics; with ``details`` also ``per_frame`` (int64
    [seq_length + 1, 4]: tp, fp, fn, ignored) and ``trajectories`` (per ground-truth trajectory, the b-trajectory index matched
    in each of its frames, -1 for none)."""
    ai = lambda v: np.asarray(v).reshape(-1).astype(np.int64)
    a_frame, a_traj, a_match_b, a_inter, a_uni = ai(a_frame), ai(a_traj), ai(a_match_b), ai(a_inter), ai(a_uni)
    b_frame, b_traj = ai(b_frame), ai(b_traj)
    a_ignore, b_matched, b_ignored = (np.asarray(v).reshape(-1).astype(bool) for v in (a_ignore, b_matched, b_ignored))
    id_match = np.asarray(id_match, np.int64)
    n_gt_traj, n_tr_traj = int(id_match.shape[0]), int(id_match.shape[1])
    n_frames = int(seq_length) + 1
    for fr in (a_frame, b_frame):
        if fr.size and (fr.min() < 0 or fr.max() > seq_length):
            raise ValueError("a frame outside [0, seq_length = %d]" % seq_length)
    if a_frame.size > 1 and (np.diff(a_frame) < 0).any():
        raise ValueError("the a-side entries must be sorted by frame")
    m = dict.fromkeys(METRIC_NAMES, 0)
    m["total_num_frames"] = n_frames
    gt = ~a_ignore
    g_per_frame = np.bincount(a_frame[gt], minlength=n_frames)
    t_per_frame = np.bincount(b_frame, minlength=n_frames)
    matched = gt & (a_match_b >= 0)
    tp_per_frame = np.bincount(a_frame[matched], minlength=n_frames)
    itr_per_frame = np.bincount(b_frame[b_ignored & ~b_matched], minlength=n_frames)
    fn_per_frame = g_per_frame - tp_per_frame
    fp_per_frame = t_per_frame - tp_per_frame - itr_per_frame
    if (fp_per_frame < 0).any() or (fn_per_frame < 0).any():
        raise ValueError("Something went wrong! a negative count of false positives or negatives")
    m["n_gt"], m["n_tr"] = int(g_per_frame.sum()), int(t_per_frame.sum())
    m["tp"], m["fn"], m["fp"], m["n_itr"] = (int(v.sum()) for v in (tp_per_frame, fn_per_frame, fp_per_frame, itr_per_frame))
    # the overlaps, as doubles, summed in (frame, gt row) order: total_cost over the sequence, tmpc per frame (:256-257)
    total_cost, modsp = 0, 0
    frame_cost = [0] * n_frames
    for k in np.flatnonzero(matched):
        c = float(a_inter[k]) / float(a_uni[k])
        total_cost += c
        frame_cost[a_frame[k]] += c
    for f in range(n_frames):
        modsp += frame_cost[f] / float(tp_per_frame[f]) if tp_per_frame[f] != 0 else 1
    m["total_cost"], m["MODSP"] = total_cost, modsp
    m["n_gt_trajectories"], m["n_tr_trajectories"] = n_gt_traj, n_tr_traj

    # :343-373, literally: MT / PT / ML, fragments and id switches of every ground-truth trajectory
    seqs = [[] for _ in range(n_gt_traj)]
    for k in np.flatnonzero(gt):
        seqs[a_traj[k]].append(int(b_traj[a_match_b[k]]) if a_match_b[k] >= 0 else -1)
    for g in seqs:
        if all([this == -1 for this in g]):
            m["ML"] += 1
            continue
        last_id = g[0]
        tracked = 1 if g[0] >= 0 else 0
        f = 0
        for f in range(1, len(g)):
            if last_id != g[f] and last_id != -1 and g[f] != -1:
                m["id_switches"] += 1
            if f < len(g) - 1 and g[f - 1] != g[f] and last_id != -1 and g[f] != -1 and g[f + 1] != -1:
                m["fragments"] += 1
            if g[f] != -1:
                tracked += 1
                last_id = g[f]
        if len(g) > 1 and g[f - 1] != g[f] and last_id != -1 and g[f] != -1:
            m["fragments"] += 1
        tracking_ratio = tracked / float(len(g))
        if tracking_ratio > 0.8:
            m["MT"] += 1
        elif tracking_ratio < 0.2:
            m["ML"] += 1
        else:
            m["PT"] += 1

    # IDF1 (:388-472): the (n_gt + n_st)-square assignment problem over trajectory pairs
    if n_gt_traj != 0:
        len_gt = np.bincount(a_traj[gt], minlength=n_gt_traj).astype(float)
        len_st = np.bincount(b_traj, minlength=n_tr_traj).astype(float)
        # a prediction that the ignore region covers by more than half cannot reach IoU 0.5 with a ground-truth object (those are
        # disjoint from the region): it is unmatched against every trajectory, so ign[i, j] of :535 is the same for every i
        ign_st = np.bincount(b_traj[b_ignored], minlength=n_tr_traj).astype(float)
        n_gt, n_st = n_gt_traj, n_tr_traj
        cost = np.zeros((n_gt + n_st, n_st + n_gt), dtype=float)
        cost[n_gt:, :n_st] = sys.maxsize
        cost[:n_gt, n_st:] = sys.maxsize
        fp, fn, ign = np.zeros(cost.shape), np.zeros(cost.shape), np.zeros(cost.shape)
        fn[:n_gt, :n_st] = len_gt[:, None] - id_match
        fp[:n_gt, :n_st] = (len_st - ign_st)[None, :] - id_match
        ign[:n_gt, :n_st] = ign_st[None, :]
        cost[:n_gt, :n_st] = fp[:n_gt, :n_st] + fn[:n_gt, :n_st]
        for i in range(n_st):
            cost[i + n_gt, i] = fp[i + n_gt, i] = len_st[i] - ign_st[i]
            ign[i + n_gt, i] = ign_st[i]
        for i in range(n_gt):
            cost[i, i + n_st] = fn[i, i + n_st] = len_gt[i]
        from scipy.optimize import linear_sum_assignment
        rows, cols = linear_sum_assignment(cost)
        nbox_gt, nbox_st = len_gt.sum(), len_st.sum()
        idfn, id_ign = fn[rows, cols].sum(), ign[rows, cols].sum()
        m["IDTP"], m["id_n_tr"], m["nbox_gt"] = nbox_gt - idfn, nbox_st - id_ign, nbox_gt

    # compute_clearmot (:85-159)
    tp, fp_, fn_, n_gt_ = m["tp"], m["fp"], m["fn"], m["n_gt"]
    if (fp_ + tp) == 0 or (tp + fn_) == 0:
        m["recall"] = m["precision"] = 0.
    else:
        m["recall"] = tp / float(tp + fn_) * 100.
        m["precision"] = tp / float(fp_ + tp) * 100.
    m["F1"] = 0. if (m["recall"] + m["precision"]) == 0 else (2. * (m["precision"] * m["recall"]) / (m["precision"] + m["recall"])) * 100.
    m["FAR"] = fp_ / float(n_frames)
    if n_gt_ == 0:
        m["MOTSA"] = m["MODSA"] = m["sMOTSA"] = m["MOTSAL"] = -float("inf")
    else:
        idsw = m["id_switches"]
        m["MOTSA"] = (1 - (fn_ + fp_ + idsw) / float(n_gt_)) * 100.
        m["MODSA"] = (1 - (fn_ + fp_) / float(n_gt_)) * 100.
        m["sMOTSA"] = ((total_cost - fp_ - idsw) / float(n_gt_)) * 100.
        m["MOTSAL"] = (1 - (fn_ + fp_ + (np.log10(idsw) if idsw else 0)) / float(n_gt_)) * 100.
    m["MOTSP"] = float("inf") if tp == 0 else total_cost / float(tp) * 100.
    m["MODSP"] = modsp / float(n_frames) * 100.
    for name in ("MT", "PT", "ML"):
        m[name + "R"] = m[name] * 100. / float(n_gt_traj) if n_gt_traj else 0.
    if m["recall"] != 0:
        m["id_switches_rel"] = m["id_switches"] / m["recall"] * 100
        m["fragments_rel"] = m["fragments"] / m["recall"] * 100
    else:
        m["id_switches_rel"] = m["fragments_rel"] = float("inf")
    m["IDF1"] = (2 * m["IDTP"]) / (m["nbox_gt"] + m["id_n_tr"]) * 100. if n_gt_traj else 0.
    if details:
        m["per_frame"] = np.stack((tp_per_frame, fp_per_frame, fn_per_frame, itr_per_frame), axis=1).astype(np.int64)
        m["trajectories"] = seqs
    return m


# ------------------------------------------------------------------------------------------------ sequences
def _as_loaded(v):
    return v if isinstance(v, dict) else load_mots_txt(v)


class _Side:
    """One side's list for the whole sequence: the rows of a loaded file that take part (sorted by frame, file order inside a
    frame), their trajectory index and their runs regrouped by entry."""

    def __init__(self, rows, keep, traj_classes):
        order = np.flatnonzero(keep)
        order = order[np.argsort(rows["frame"][order], kind="stable")]
        self.frame = rows["frame"][order]
        self.class_id = rows["class_id"][order]
        self.track_id = rows["track_id"][order]
        in_traj = np.isin(self.class_id, traj_classes)
        self.ids = np.unique(self.track_id[in_traj])                       # sorted: the kit's sorted(gt_ids) / sorted(st_ids)
        self.traj = np.where(in_traj, np.searchsorted(self.ids, self.track_id), -1).astype(np.int64)
        entry_of_row = np.full(rows["frame"].size, -1, np.int64)
        entry_of_row[order] = np.arange(order.size)
        e = entry_of_row[rows["run_row"]]
        sel = np.flatnonzero(e >= 0)
        sel = sel[np.argsort(e[sel], kind="stable")]
        self.run_entry, self.run_begin, self.run_end = e[sel], rows["run_begin"][sel], rows["run_end"][sel]
        self.size = rows["h"][order], rows["w"][order]

    def launch(self, frames):
        """(ptr [len(frames) + 1], first entry, runs of those entries with LOCAL entry numbers) for ascending ``frames``"""
        lo, hi = np.searchsorted(self.frame, frames, "left"), np.searchsorted(self.frame, frames, "right")
        counts = hi - lo
        entries = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]) if len(frames) else np.zeros(0, np.int64)
        local = np.full(self.frame.size + 1, -1, np.int64)
        local[entries] = np.arange(entries.size)
        r0, r1 = np.searchsorted(self.run_entry, entries, "left"), np.searchsorted(self.run_entry, entries, "right")
        runs = np.concatenate([np.arange(a, b) for a, b in zip(r0, r1)]).astype(np.int64) if entries.size else np.zeros(0, np.int64)
        return (np.concatenate(([0], np.cumsum(counts))).astype(np.int64), entries,
                (local[self.run_entry[runs]], self.run_begin[runs], self.run_end[runs]))


def _image_size(*sides):
    sizes = {(int(h), int(w)) for s in sides for h, w in zip(*s.size)}
    if len(sizes) > 1:
        raise ValueError("the masks of a sequence need one image size (found %s)" % sorted(sizes))
    return sizes.pop() if sizes else None


def _evaluate(gt_rows, seq_length, class_id, ignore_class, frames_per_launch, device, b_frame, b_traj, b_ids,
              b_labels, img_shape, details, ops=None):
    """The launches of a sequence.  The b-side is given by its frames' entries (``b_frame`` ascending, ``b_traj``; -1: an entry
    that only occupies pixels) and ``b_labels(frames, b_ptr, b_entries, hw)`` -> the label images of ascending ``frames``.
    ``ops``: the three operators (this module's; the tests' numpy restatements have no device to run on)."""
    ops = ops or sys.modules[__name__]
    n_b_traj = int(np.asarray(b_ids).size)
    a = _Side(gt_rows, np.isin(gt_rows["class_id"], (class_id, ignore_class)), (class_id,))
    a_size = _image_size(a)
    if img_shape is not None and a_size is not None and a_size != (int(img_shape[0]), int(img_shape[1])):
        raise ValueError("the ground truth's image size %s is not the prediction's %s" % (a_size, tuple(img_shape)))
    H, W = (int(v) for v in (img_shape if img_shape is not None else (a_size or (0, 0))))
    hw = H * W
    a_ignore = a.class_id == ignore_class
    n_a, n_b = a.frame.size, b_frame.size
    res = {"match_b": np.full(n_a, -1, np.int64), "inter": np.zeros(n_a, np.int64), "uni": np.zeros(n_a, np.int64),
           "b_matched": np.zeros(n_b, bool), "b_ignored": np.zeros(n_b, bool)}
    id_match = np.zeros((a.ids.size, n_b_traj), np.int64)
    frames = np.union1d(a.frame, b_frame)
    step = max(int(frames_per_launch), 1)
    for g0 in range(0, frames.size if hw else 0, step):
        fl = frames[g0:g0 + step]
        a_ptr, a_entries, (re_, rb, ren) = a.launch(fl)
        b_lo, b_hi = np.searchsorted(b_frame, fl, "left"), np.searchsorted(b_frame, fl, "right")
        b_ptr = np.concatenate(([0], np.cumsum(b_hi - b_lo))).astype(np.int64)
        b_entries = np.concatenate([np.arange(x, y) for x, y in zip(b_lo, b_hi)]).astype(np.int64)
        labels_a = ops.paint_label_runs(re_, rb, ren, a_ptr, a_entries.size, hw, device)
        labels_b = b_labels(fl, b_ptr, b_entries, hw).reshape(fl.size, hw)
        table, tp = ops.label_overlap(labels_a, labels_b, a_ptr, b_ptr)
        out = ops.frame_match(table, tp, a_ptr, b_ptr, a_ignore[a_entries], a.traj[a_entries], b_traj[b_entries], a.ids.size, n_b_traj)
        res["match_b"][a_entries] = np.append(b_entries, -1)[out["match_b"]]   # (-1 stays -1)
        res["inter"][a_entries], res["uni"][a_entries] = out["inter"], out["uni"]
        res["b_matched"][b_entries], res["b_ignored"][b_entries] = out["b_matched"], out["b_ignored"]
        id_match += out["id_match"]
    # b-entries without a trajectory (another class) only occupied pixels: the kit never sees them, so a match with one is none
    counted = b_traj >= 0
    renum = np.append(np.where(counted, np.cumsum(counted) - 1, -1), -1)   # (the last one: no match stays no match)
    match_b = renum[res["match_b"]]
    m = metrics_from_matches(a.frame, a.traj, a_ignore, match_b, res["inter"], res["uni"], b_frame[counted], b_traj[counted],
                             res["b_matched"][counted], res["b_ignored"][counted], id_match, seq_length, details=details)
    if details:   # trajectories by their MOTS ids: {ground-truth id: the prediction id matched in each of its frames, or -1}
        m["trajectories"] = {int(g): [int(b_ids[j]) if j >= 0 else -1 for j in seq] for g, seq in zip(a.ids, m["trajectories"])}
    return m


def evaluate_mots_files(pred_txt, gt_txt, seq_length, class_id=CLASS_ID, ignore_class=IGNORE_CLASS, frames_per_launch=8,
                        device="cuda", details=False, _ops=None):
    """``compute_mots_metrics`` for one sequence: the metrics of the MOTS result file ``pred_txt`` against the ground truth
    ``gt_txt`` (paths, or what ``load_mots_txt`` returns) over the frames ``0 .. seq_length`` (``seqlength`` of the sequence's
    ``seqinfo.ini``).  Both sides are painted from their runs, ``frames_per_launch`` frames share a launch (the label workspace
    is 2 x 4 B x H x W x frames_per_launch), and the result does not depend on it.  Objects of other classes are left out of the
    lists (their pixels are -1); ignore-class rows of the ground truth are its ignore region.  ``details``: see
    ``metrics_from_matches`` (the trajectories then by their ids: {ground-truth id: [prediction id or -1 per frame]})."""
    gt, pred = _as_loaded(gt_txt), _as_loaded(pred_txt)
    b = _Side(pred, pred["class_id"] == class_id, (class_id,))

    def b_labels(frames, b_ptr, b_entries, hw):
        _, entries, (re_, rb, ren) = b.launch(frames)
        return (_ops or sys.modules[__name__]).paint_label_runs(re_, rb, ren, b_ptr, entries.size, hw, device)
    return _evaluate(gt, seq_length, class_id, ignore_class, frames_per_launch, device, b.frame, b.traj, b.ids, b_labels,
                     _image_size(b), details, ops=_ops)
