"""The training inputs the reference's ``MOTSeqProcessor`` makes from a detections file and a ground-truth file
(``data/seq_processing/seq_processor.py``), on the device and without ``lapsolver``, ``pycocotools`` or ``torchvision``:

``assign_gt``      ``_assign_gt`` (``:203-237``): a ground-truth identity per detection (``det_df.id``, what
                   ``graph.assign_edge_labels`` needs), frame by frame from box IoU (``utils/iou.py:4-31``) or mask IoU
                   (``iou_mask``, ``:62-76``), a threshold and a bipartite matching;
``gt_roi_masks``   ``_store_gt_masks`` (``:289-393``) up to the files: the matched ground-truth mask of every detection, RoIAligned
                   over the detection's box (torchvision 0.6.0 ``roi_align``, ``spatial_scale=1``, ``sampling_ratio=-1``);
``store_gt_masks`` the two per-frame file families ``graph.assign_mask_labels`` reads.

The operators are ``csrc/gt_assign.hip`` (``include/mpnhip.h`` states them); the matching is ``mpnhip_lsa_batched``.  Masks are
handled as in ``mots_eval``: a side of a frame is ONE int32 label image painted from its run lengths (``paint_label_runs``), all
intersections of a frame are one joint histogram (``label_overlap``), and RoIAlign samples the ground truth's label image -- the
reference decodes one full-frame float image per matched detection.  This needs masks that are DISJOINT within a side of a frame,
as the masks of a MOTS file are; overlapping masks are refused with ``load_mots_txt``'s error.

The assignment contract.  The reference calls ``lapsolver.solve_dense(1 - iou)`` with NaN where ``iou < min_iou``.  That is taken to
mean: among the matchings that use only allowed pairs, one with the most pairs; among those, one of the smallest total ``1 - iou``.
It is implemented as ``cost = allowed ? 1 - iou : min(na_f, nb_f) + 1`` -- more than any total of allowed costs, each at most 1 --
solved as a plain rectangular assignment, with the matched pairs on forbidden cells dropped.  ``lapsolver`` was not available where
this was written, so this reading of its NaN handling has not been checked against it; ``tests/gt_assign_ref.py`` pins the
contract itself against a brute-force search."""
import os.path as osp

import numpy as np
import torch

from . import assignment, capi, masks as M, mots_eval as ME
from .capi import MpnhipError, check, ptr, stream_ptr

BOX_TLBR = ("bb_top", "bb_left", "bb_bot", "bb_right")    # utils/iou.py: (top, left, bottom, right)
BOX_LTRB = ("bb_left", "bb_top", "bb_right", "bb_bot")    # seq_processor.py:322
IGNORE_IDS = (-1, 10000)                                  # seq_processor.py:329
MAX_GRID = 256                                            # MPNHIP_ROI_MAX_GRID


def _col(rows, name, dtype=None):
    v = rows[name]
    v = np.asarray(v.values if hasattr(v, "values") else v).reshape(-1)
    return v if dtype is None else v.astype(dtype)


def _dev(t, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(t), dtype=dtype)).to(dev)


def _device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise MpnhipError("mpntrackseg_amd runs on a HIP device only (%s); there is no CPU fallback" % dev)
    return dev


class _Rows:
    """the rows of one file sorted by frame (file order inside a frame): ``order`` (row of every entry) and ``frame``"""

    def __init__(self, frame):
        self.order = np.argsort(frame, kind="stable")
        self.frame = frame[self.order]

    def launch(self, frames):
        """(ptr [len(frames) + 1], entries) of ascending ``frames``"""
        lo, hi = np.searchsorted(self.frame, frames, "left"), np.searchsorted(self.frame, frames, "right")
        entries = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]).astype(np.int64) if len(frames) else np.zeros(0, np.int64)
        return np.concatenate(([0], np.cumsum(hi - lo))).astype(np.int64), entries


def mask_rows(rows, device=None):
    """The masks of ``rows`` (``frame``, ``img_height``, ``img_width``, ``rle``: COCO's compressed strings) as ``load_mots_txt``
    returns them -- runs of set pixels at positions ``x * h + y`` -- refusing what it refuses: counts that do not describe the
    image, and overlapping masks in a frame.  ``device``: decode the strings there, all rows in two launches
    (``masks.rle_decode_batch``), instead of one numpy decode per row: the same dict, the same refusals."""
    frame, hs, ws = _col(rows, "frame", np.int64), _col(rows, "img_height", np.int64), _col(rows, "img_width", np.int64)
    rle = _col(rows, "rle")
    if device is not None:
        return _mask_rows_device(frame, hs, ws, rle, device)
    rr, rb, re_ = [], [], []
    for k in range(frame.size):
        s = rle[k]
        counts = M.rle_counts(s.decode("ascii") if isinstance(s, bytes) else str(s))
        if hs[k] < 0 or ws[k] < 0 or (counts.size and counts.min() < 0) or int(counts.sum()) != hs[k] * ws[k]:
            raise ValueError("the counts of row %d in frame %d do not describe a %d x %d mask" % (k, frame[k], hs[k], ws[k]))
        b, e = ME.counts_to_runs(counts)
        rr.append(np.full(b.size, k, np.int64))
        rb.append(b)
        re_.append(e)
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    out = {"frame": frame, "h": hs, "w": ws, "run_row": cat(rr), "run_begin": cat(rb), "run_end": cat(re_),
           "class_id": np.zeros(frame.size, np.int64), "track_id": np.arange(frame.size, dtype=np.int64)}
    ME.refuse_overlapping_masks(frame, out["run_row"], out["run_begin"], out["run_end"])
    return out


def _mask_rows_device(frame, hs, ws, rle, device):
    """``mask_rows`` with the strings decoded on the device.  A string that is not ASCII is the host codec's to refuse: the rows
    before it are decoded first, since an earlier bad row decides."""
    strings, foreign = [], None
    for k in range(frame.size):
        s = rle[k]
        if (isinstance(s, bytes) and not s.isascii()) or (not isinstance(s, bytes) and not str(s).isascii()):
            foreign = k
            break
        strings.append(s.decode("ascii") if isinstance(s, bytes) else str(s))
    n = len(strings)
    dec = M.rle_decode_batch(strings, hs[:n], ws[:n], device)
    status = dec["status"]
    bad = np.flatnonzero((status != 0) | (hs[:n] < 0) | (ws[:n] < 0))
    if bad.size:
        k = int(bad[0])
        text = M.rle_status_error(int(status[k]))
        if text is not None:
            raise ValueError(text)
        raise ValueError("the counts of row %d in frame %d do not describe a %d x %d mask" % (k, frame[k], hs[k], ws[k]))
    if foreign is not None:
        s = rle[foreign]
        M.rle_counts(s.decode("ascii") if isinstance(s, bytes) else str(s))   # raises what the host path raises
    runs = torch.stack((dec["run_row"], dec["run_begin"], dec["run_end"])).cpu().numpy().astype(np.int64)
    out = {"frame": frame, "h": hs, "w": ws, "run_row": runs[0], "run_begin": runs[1], "run_end": runs[2],
           "class_id": np.zeros(frame.size, np.int64), "track_id": np.arange(frame.size, dtype=np.int64)}
    ME.refuse_overlapping_masks(frame, out["run_row"], out["run_begin"], out["run_end"])
    return out


def _mask_side(rows, strings_device=None):
    """``mots_eval._Side`` over all rows: the same order as ``_Rows`` (a stable sort by frame), plus the runs by entry"""
    loaded = mask_rows(rows, strings_device)
    return ME._Side(loaded, np.ones(loaded["frame"].size, bool), ())


def _cells(a_ptr, b_ptr):
    cell_ptr = np.concatenate(([0], np.cumsum(np.diff(a_ptr) * np.diff(b_ptr)))).astype(np.int64)
    if int(cell_ptr[-1]) >= 1 << 31:
        raise MpnhipError("%d cells (2^31 or more) in one launch are not supported: fewer frames per launch" % int(cell_ptr[-1]))
    return cell_ptr


def _cost_buffers(cells, dev):
    return ME._buf(cells, torch.float64, dev), ME._buf(cells, torch.uint8, dev), ME._buf(cells, torch.float64, dev)


# ------------------------------------------------------------------------------------------------ operators (device)
def box_iou_costs(a_boxes, b_boxes, a_ptr, b_ptr, min_iou=0.5, device=None):
    """``mpnhip_box_iou_costs``: ``(iou, allowed, cost, cell_ptr)`` of two box lists ([n, 4] float64 host arrays: top, left,
    bottom, right) grouped by frame -- the cells on the device, ``cell_ptr`` (int64) on the host."""
    lib, dev = capi.load(), _device(device)
    a_ptr, b_ptr = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    if a_ptr.size != b_ptr.size or a_ptr.size < 1:
        raise MpnhipError("a_ptr and b_ptr need one entry per frame plus one")
    cell_ptr = _cells(a_ptr, b_ptr)
    with torch.cuda.device(dev):
        a, b = _dev(np.asarray(a_boxes, np.float64).reshape(-1, 4), np.float64, dev), _dev(np.asarray(b_boxes, np.float64).reshape(-1, 4), np.float64, dev)
        if a.shape[0] != int(a_ptr[-1]) or b.shape[0] != int(b_ptr[-1]):
            raise MpnhipError("one box per entry of either list")
        ap, bp, cp = _dev(a_ptr, np.int32, dev), _dev(b_ptr, np.int32, dev), _dev(cell_ptr, np.int64, dev)
        iou, allowed, cost = _cost_buffers(int(cell_ptr[-1]), dev)
        check(lib.mpnhip_box_iou_costs(ptr(a), a.shape[0], ptr(b), b.shape[0], ptr(ap), ptr(bp), ptr(cp), a_ptr.size - 1, iou.numel(),
                                       float(min_iou), ptr(iou), ptr(allowed), ptr(cost), stream_ptr()), "mpnhip_box_iou_costs")
    return iou, allowed, cost, cell_ptr


@capi.on_tensor_device
def overlap_iou_costs(table, table_ptr, a_ptr, b_ptr, min_iou=0.5):
    """``mpnhip_overlap_iou_costs``: the same from ``label_overlap(labels of the detections, labels of the ground truth)``"""
    lib = capi.load()
    capi.require_device(table)
    dev = table.device
    a_ptr, b_ptr = np.asarray(a_ptr, np.int64).reshape(-1), np.asarray(b_ptr, np.int64).reshape(-1)
    tp = np.ascontiguousarray(np.asarray(table_ptr, np.int64).reshape(-1))
    if a_ptr.size != b_ptr.size or a_ptr.size < 1 or tp.size != a_ptr.size:
        raise MpnhipError("a_ptr, b_ptr and table_ptr need one entry per frame plus one")
    if table.dtype != torch.int32 or table.numel() < int(tp[-1]):
        raise MpnhipError("the table must be int32 and hold table_ptr's %d cells" % int(tp[-1]))
    cell_ptr = _cells(a_ptr, b_ptr)
    ap, bp, cp, tpd = _dev(a_ptr, np.int32, dev), _dev(b_ptr, np.int32, dev), _dev(cell_ptr, np.int64, dev), _dev(tp, np.int64, dev)
    iou, allowed, cost = _cost_buffers(int(cell_ptr[-1]), dev)
    check(lib.mpnhip_overlap_iou_costs(ptr(table), int(tp[-1]), ptr(tpd), ptr(ap), int(a_ptr[-1]), ptr(bp), int(b_ptr[-1]), ptr(cp),
                                       a_ptr.size - 1, iou.numel(), float(min_iou), ptr(iou), ptr(allowed), ptr(cost), stream_ptr()),
          "mpnhip_overlap_iou_costs")
    return iou, allowed, cost, cell_ptr


# ------------------------------------------------------------------------------------------------ the reference's two steps
def _strings_device(strings, dev):
    if strings not in ("host", "device"):
        raise MpnhipError("strings must be 'host' or 'device' (%r)" % (strings,))
    return dev if strings == "device" else None


def assign_gt(det, gt, min_iou=0.5, mask_priority=False, frames_per_launch=8, device=None, details=False, strings="host"):
    """``MOTSeqProcessor._assign_gt``.  ``det`` / ``gt``: dict-likes or DataFrames with ``frame`` and the box columns ``bb_top``,
    ``bb_left``, ``bb_bot``, ``bb_right``; ``gt`` also ``id``; with ``mask_priority`` both instead of the boxes ``img_height``,
    ``img_width`` and ``rle`` (masks disjoint within a side of a frame, see the module docstring).  ``min_iou``:
    ``dataset_params['gt_assign_min_iou']``.  Returns ``(det_id, det_gt_entry)`` on the device, one per row of ``det``: the id of
    the ground-truth row the detection was assigned (int64; -1: a false positive) and that row's index in ``gt`` (int32; -1).

    A frame without ground truth leaves its detections false positives; ground truth in a frame without detections takes no
    part.  ``frames_per_launch`` frames share the launches; the result does not depend on it.  A frame whose problem the solver
    does not take (NaN costs, more than ``assignment.MAX_SIDE`` rows on a side) raises ``MpnhipError`` once all frames are
    enqueued.  ``strings`` (with ``mask_priority``): 'host' decodes the run-length strings row by row in numpy, 'device' all at once
    on the device (``mask_rows``); the result is the same.  ``details``: also a list with one dict per launch: ``frames``,
    ``a_ptr``, ``b_ptr``, ``cell_ptr`` (host), ``det_row``, ``gt_row`` (host: the row of every entry) and ``iou``, ``allowed``
    (device cells)."""
    lib, dev = capi.load(), _device(device)
    if mask_priority:
        sdev = _strings_device(strings, dev)
        a_masks, b_masks = _mask_side(det, sdev), _mask_side(gt, sdev)
        size = ME._image_size(a_masks, b_masks)
        hw = size[0] * size[1] if size else 0
    d_frame, g_frame = _col(det, "frame", np.int64), _col(gt, "frame", np.int64)
    a, b = _Rows(d_frame), _Rows(g_frame)
    g_id = _col(gt, "id", np.int64)
    if g_id.size != g_frame.size:
        raise MpnhipError("one id per ground-truth row")
    if not mask_priority:
        d_box, g_box = (np.stack([_col(r, c, np.float64) for c in BOX_TLBR], axis=1) for r in (det, gt))
    n_det = d_frame.size
    frames = np.unique(d_frame)
    step = max(int(frames_per_launch), 1)
    launches, statuses = [], []
    with torch.cuda.device(dev):
        det_id = torch.full((max(n_det, 1),), -1, dtype=torch.int64, device=dev)[:n_det]
        det_gt_entry = torch.full((max(n_det, 1),), -1, dtype=torch.int32, device=dev)[:n_det]
        for g0 in range(0, frames.size, step):
            fl = frames[g0:g0 + step]
            (a_ptr, a_e), (b_ptr, b_e) = a.launch(fl), b.launch(fl)
            det_row, gt_row = a.order[a_e], b.order[b_e]
            if mask_priority:
                _, _, (re_, rb, ren) = a_masks.launch(fl)
                labels_a = ME.paint_label_runs(re_, rb, ren, a_ptr, a_e.size, hw, dev)
                _, _, (re_, rb, ren) = b_masks.launch(fl)
                labels_b = ME.paint_label_runs(re_, rb, ren, b_ptr, b_e.size, hw, dev)
                table, tp = ME.label_overlap(labels_a, labels_b, a_ptr, b_ptr)
                iou, allowed, cost, cell_ptr = overlap_iou_costs(table, tp, a_ptr, b_ptr, min_iou)
            else:
                iou, allowed, cost, cell_ptr = box_iou_costs(d_box[det_row], g_box[gt_row], a_ptr, b_ptr, min_iou, dev)
            match_b, _, status = assignment.linear_sum_assignment_batched(cost, cell_ptr, a_ptr, b_ptr)
            ap, bp, cp = _dev(a_ptr, np.int32, dev), _dev(b_ptr, np.int32, dev), _dev(cell_ptr, np.int64, dev)
            ids, grow, drow = _dev(g_id[gt_row], np.int64, dev), _dev(gt_row, np.int32, dev), _dev(det_row, np.int32, dev)
            check(lib.mpnhip_gt_assign_finish(ptr(match_b), ptr(allowed), iou.numel(), ptr(cp), ptr(ap), a_e.size, ptr(bp), b_e.size, fl.size,
                                              ptr(ids), ptr(grow), ptr(drow), n_det, ptr(det_gt_entry), ptr(det_id), stream_ptr()),
                  "mpnhip_gt_assign_finish")
            statuses.append(status)
            if details:
                launches.append({"frames": fl, "a_ptr": a_ptr, "b_ptr": b_ptr, "cell_ptr": cell_ptr, "det_row": det_row, "gt_row": gt_row,
                                 "iou": iou, "allowed": allowed})
        if statuses:
            assignment.raise_on_status(torch.cat(statuses), "assign_gt (problems are the detections' frames in ascending order)")
    return (det_id, det_gt_entry, launches) if details else (det_id, det_gt_entry)


def gt_roi_masks(det, gt, det_gt_entry, size=(56, 56), ignore_ids=IGNORE_IDS, frames_per_launch=8, strings="host"):
    """``MOTSeqProcessor._store_gt_masks`` up to its files.  ``det``: ``frame`` and the box columns ``bb_left``, ``bb_top``,
    ``bb_right``, ``bb_bot`` (used as float32, like the reference's ``.float()``); ``gt``: ``frame``, ``id``, ``img_height``,
    ``img_width``, ``rle`` (masks disjoint within a frame); ``det_gt_entry``: ``assign_gt``'s, on the device.  ``size``:
    ``dataset_params['gt_mask_spatial_size']``.  Returns ``(masks [n_det, 1, size[0], size[1]] float32, valid [n_det] uint8)`` on
    that device: ``roi_align`` of the assigned ground-truth mask over the detection's box, and whether there is one -- a
    detection without a match, or matched to an id of ``ignore_ids``, has a zero mask and ``valid`` 0.  ``strings``: as in
    ``assign_gt``."""
    lib = capi.load()
    capi.require_device(det_gt_entry)
    dev = det_gt_entry.device
    ph, pw = int(size[0]), int(size[1])
    d_frame = _col(det, "frame", np.int64)
    n_det = d_frame.size
    if det_gt_entry.dtype != torch.int32 or det_gt_entry.numel() != n_det:
        raise MpnhipError("det_gt_entry must be int32 with one entry per detection")
    if ph <= 0 or pw <= 0:
        raise MpnhipError("the output size must be positive")
    d_box = np.stack([_col(det, c, np.float32) for c in BOX_LTRB], axis=1)
    if not np.isfinite(d_box).all():
        raise ValueError("a detection's box is not finite")
    with np.errstate(over="ignore"):
        too_large = ((d_box[:, 2] - d_box[:, 0]) / np.float32(pw) > MAX_GRID) | ((d_box[:, 3] - d_box[:, 1]) / np.float32(ph) > MAX_GRID)
    if too_large.any():
        raise ValueError("the box of detection %d needs more than %d samples per output pixel and axis" % (int(np.flatnonzero(too_large)[0]), MAX_GRID))
    g_id = _col(gt, "id", np.int64)
    b = _mask_side(gt, _strings_device(strings, dev))
    n_gt = b.frame.size
    b_order = np.argsort(_col(gt, "frame", np.int64), kind="stable")   # (the order of b's entries)
    img = ME._image_size(b)
    a = _Rows(d_frame)
    frames = np.unique(d_frame)
    step = max(int(frames_per_launch), 1)
    with torch.cuda.device(dev):
        entry = det_gt_entry.contiguous()
        masks = torch.zeros((n_det, 1, ph, pw), dtype=torch.float32, device=dev)
        valid = torch.zeros(max(n_det, 1), dtype=torch.uint8, device=dev)[:n_det]
        if img is None:   # no ground truth at all
            return masks, valid
        ids, ign = _dev(g_id, np.int64, dev), _dev(np.asarray(ignore_ids, np.int64).reshape(-1), np.int64, dev)
        for g0 in range(0, frames.size, step):
            fl = frames[g0:g0 + step]
            a_ptr, a_e = a.launch(fl)
            b_ptr, b_e, (re_, rb, ren) = b.launch(fl)
            labels = ME.paint_label_runs(re_, rb, ren, b_ptr, b_e.size, img[0] * img[1], dev)
            gt_label = np.full(n_gt, -1, np.int32)
            gt_label[b_order[b_e]] = np.arange(b_e.size)
            det_row = a.order[a_e]
            ap, bp, lab = _dev(a_ptr, np.int32, dev), _dev(b_ptr, np.int32, dev), _dev(gt_label, np.int32, dev)
            boxes, drow = _dev(d_box[det_row], np.float32, dev), _dev(det_row, np.int32, dev)
            check(lib.mpnhip_roi_align_labels(ptr(labels), fl.size, img[0], img[1], ptr(ap), ptr(bp), ptr(boxes), a_e.size, ptr(drow), ptr(entry),
                                              n_det, ptr(lab), ptr(ids), n_gt, ptr(ign), ign.numel(), ph, pw, ptr(masks), ptr(valid),
                                              stream_ptr()), "mpnhip_roi_align_labels")
    return masks, valid


def store_gt_masks(seq_path, det, masks, valid, gt_dir=osp.join("gt", "gt_mask")):
    """The files of ``_store_gt_masks`` (``:372-391``) under ``<seq_path>/processed_data/<gt_dir>/``: ``masks/<frame>.pt``
    ``[n, 2, H, W]`` with the detection id broadcast into channel 0, and ``valid_ixs/<frame>.pt`` ``[n, 2]`` = (detection id, has
    a ground-truth mask).  ``det``: ``frame`` and ``detection_id`` (rows sorted by frame, as the reference's ``det_df``);
    ``graph.assign_mask_labels`` reads them back."""
    from .embeddings import write_frame_embeddings
    frame, det_ids = _col(det, "frame", np.int64), _col(det, "detection_id", np.int64)
    masks, valid = torch.as_tensor(masks).detach().cpu().float(), torch.as_tensor(valid).detach().cpu().float().view(-1, 1)
    if masks.dim() != 4 or masks.shape[1] != 1 or masks.shape[0] != frame.size or valid.shape[0] != frame.size:
        raise MpnhipError("masks [n, 1, H, W] and valid [n] need one row per detection")
    write_frame_embeddings(seq_path, osp.join(gt_dir, "masks"), frame, det_ids, masks)
    write_frame_embeddings(seq_path, osp.join(gt_dir, "valid_ixs"), frame, det_ids, valid)
