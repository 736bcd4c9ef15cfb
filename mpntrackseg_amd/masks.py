"""Full-frame MOTS masks: host mirror of ``MPNTracker._to_full_masks`` (reference ``src/mot_neural_solver/tracker/mpn_tracker.py:267-298``)
over the C ABI (``csrc/full_masks.hip``).

The reference pastes every RoI mask of a frame into an image of its own (torchvision's ``paste_masks_in_image``), takes the arg-max
over the n images (``utils/mots.py:5-25``), thresholds and hands the (H, W, n) array to ``pycocotools``.  Here a frame is one
int32 label per pixel, written by one kernel (``paste_unique_masks``), and a detection's run-length code is the list of
positions where ``label == detection`` flips (``mask_run_events``): what reaches the host is that list, a few hundred integers
per detection, and the only host work is ``np.diff`` and COCO's string form (``rle_string``).

Label images are column-major, as COCO flattens a mask: ``labels[frame, x, y]``, position ``p = x * H + y``.  The codec
(``rle_string`` / ``rle_counts`` / ``rle_to_mask``) is plain numpy and needs neither a device nor ``pycocotools``.  The same codec
for all masks of a call runs on the device (``csrc/rle_codec.hip``): ``mask_run_strings`` / ``rle_strings`` write the strings of a
launch, ``rle_decode_batch`` reads a list of strings into runs of set pixels; both give the host codec's bytes and integers."""
import numpy as np
import torch

from . import capi
from .capi import MpnhipError, check, ptr, stream_ptr


def _as_masks(roi_masks):
    m = capi.f32c(roi_masks)
    if m.dim() == 4 and m.shape[1] == 1:
        m = m.view(m.shape[0], m.shape[2], m.shape[3])
    if m.dim() != 3:
        raise MpnhipError("roi_masks must be [n, 1, mh, mw] or [n, mh, mw]")
    return m


def _as_int32(v, device):
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=torch.int32).contiguous().view(-1)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.int32)).to(device)


@capi.on_tensor_device
def paste_unique_masks(roi_masks, boxes, frame_ptr, img_shape, mask_threshold, return_values=False, det_ids=None):
    """Paste, arg-max and threshold of ``frame_ptr.numel() - 1`` frames of size ``img_shape = (H, W)`` in one launch.

    ``roi_masks`` [n, 1, mh, mw] float32 and ``boxes`` [n, 4] (left, top, right, bottom; evaluated in float64) on the device.  The
    launch's detections are a list grouped by frame: entry j is row ``det_ids[j]`` of masks and boxes (``det_ids`` None: the rows
    themselves), frame f owns the entries ``frame_ptr[f] : frame_ptr[f + 1]``.  Returns ``labels`` [F, W, H] int32 (the list
    entry that owns the pixel, or -1), and with ``return_values`` the winner's value per pixel [F, W, H] float32 as well."""
    lib = capi.load()
    capi.require_device(roi_masks)
    if not float(mask_threshold) > 0.0:
        raise MpnhipError("mask_threshold must be positive: with a threshold <= 0 the reference hands every pixel no mask covers to "
                          "the frame's first detection")
    m = _as_masks(roi_masks)
    dev = m.device
    bx = boxes if isinstance(boxes, torch.Tensor) else torch.from_numpy(np.asarray(boxes, dtype=np.float64))
    bx = bx.to(device=dev, dtype=torch.float64).contiguous()
    if bx.dim() != 2 or bx.shape[1] != 4 or bx.shape[0] != m.shape[0]:
        raise MpnhipError("boxes must be [n, 4] with one row per mask (%s for %d masks)" % (tuple(bx.shape), m.shape[0]))
    fp = _as_int32(frame_ptr, dev)
    ids = None if det_ids is None else _as_int32(det_ids, dev)
    F = int(fp.numel()) - 1
    n = int(m.shape[0]) if ids is None else int(ids.numel())
    H, W = int(img_shape[0]), int(img_shape[1])
    if F < 0 or H < 0 or W < 0:
        raise MpnhipError("frame_ptr needs at least one entry and the image a non-negative size")
    labels = torch.empty((F, W, H), dtype=torch.int32, device=dev)
    values = torch.empty((F, W, H), dtype=torch.float32, device=dev) if return_values else None
    ws = capi.workspace(lib.mpnhip_full_masks_workspace_bytes(n, F, H * W, 0), dev, "full_masks")
    check(lib.mpnhip_paste_unique_masks(ptr(m), m.shape[0], m.shape[1], m.shape[2], ptr(bx), ptr(ids), n, ptr(fp), F, H, W,
                                        float(mask_threshold), ptr(labels), ptr(values), ptr(ws), ws.numel(), stream_ptr()),
          "mpnhip_paste_unique_masks")
    return (labels, values) if return_values else labels


@capi.on_tensor_device
def mask_run_events(labels, num_dets):
    """The run boundaries of the masks ``labels == d`` for d in [0, num_dets): ``(positions, counts)`` as host arrays --
    ``counts`` [num_dets] events per detection, ``positions`` [counts.sum()] sorted by (detection, position).  ``labels`` [F, W, H]
    int32 as ``paste_unique_masks`` returns it.  Two host reads: the number of events (it sizes the buffer), then the events."""
    lib = capi.load()
    capi.require_device(labels)
    if labels.dtype != torch.int32 or labels.dim() != 3:
        raise MpnhipError("labels must be int32 [F, W, H]")
    lab = labels.contiguous()
    F, hw, n, dev = int(lab.shape[0]), int(lab.shape[1]) * int(lab.shape[2]), int(num_dets), lab.device
    counts = torch.zeros(n + 1, dtype=torch.int32, device=dev)   # [n]: the total
    ws = capi.workspace(lib.mpnhip_full_masks_workspace_bytes(n, F, hw, 0), dev, "full_masks")
    check(lib.mpnhip_mask_run_events_count(ptr(lab), F, hw, n, ptr(counts), ptr(counts[n:]), ptr(ws), ws.numel(), stream_ptr()),
          "mpnhip_mask_run_events_count")
    counts_h = counts.cpu().numpy()
    total = int(counts_h[n])
    pos = torch.empty(max(total, 1), dtype=torch.int32, device=dev)[:total]
    ws = capi.workspace(lib.mpnhip_full_masks_workspace_bytes(n, F, hw, total), dev, "full_masks")
    check(lib.mpnhip_mask_run_events(ptr(lab), F, hw, n, total, ptr(pos), ptr(ws), ws.numel(), stream_ptr()), "mpnhip_mask_run_events")
    return pos.cpu().numpy(), counts_h[:n].copy()


# ------------------------------------------------------------------------------------------------ COCO run-length codec (host)
def rle_counts_from_events(positions, hw):
    """COCO's ``counts`` of one mask from its ascending run boundaries: alternating run lengths that begin with a run of zeros
    (of length 0 when pixel 0 is set) and sum to ``hw``."""
    p = np.asarray(positions, dtype=np.int64).reshape(-1)
    return np.diff(np.concatenate((np.zeros(1, np.int64), p, np.array([hw], np.int64))))


def rle_string(counts):
    """``rleToString`` of the COCO API (``maskApi.c``): every count from the fourth on is stored as the difference to the one two
    before it, in 5-bit groups, low bits first, as the characters ``chr(48 + group + 32 * more)``."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if c.size == 0:
        return ""
    x = c.copy()
    x[3:] -= c[1:-2]
    groups = np.zeros((c.size, 13), dtype=np.uint8)   # an int64 needs at most 13 groups
    active = np.ones(c.size, dtype=bool)
    for g in range(groups.shape[1]):
        bits = x & 0x1f
        x = x >> 5   # arithmetic
        more = ~(((x == 0) & ((bits & 0x10) == 0)) | ((x == -1) & ((bits & 0x10) != 0)))
        groups[:, g] = np.where(active, bits + 48 + np.where(more, 0x20, 0), 0)
        active &= more
        if not active.any():
            break
    flat = groups.reshape(-1)
    return flat[flat != 0].tobytes().decode("ascii")


def rle_counts(string):
    """``rleFrString``: the counts of a COCO run-length string (int64)."""
    raw = np.frombuffer(string.encode("ascii"), dtype=np.uint8).astype(np.int64) - 48
    if raw.size == 0:
        return np.zeros(0, np.int64)
    if raw.min() < 0 or raw.max() > 63:
        raise ValueError("not a COCO run-length string")
    more = (raw & 0x20) != 0
    if more[-1]:
        raise ValueError("truncated COCO run-length string")
    ends = np.flatnonzero(~more)
    starts = np.concatenate(([0], ends[:-1] + 1))
    k = np.arange(raw.size) - np.repeat(starts, ends - starts + 1)   # index of the group inside its count
    if k.max() > 11:   # 60 bits: far beyond any pixel count
        raise ValueError("count too long")
    x = np.add.reduceat((raw & 0x1f) << (5 * k), starts)
    last, nk = raw[ends], k[ends] + 1
    x = np.where((last & 0x10) != 0, x | (np.int64(-1) << (5 * nk)), x)   # sign extension
    out = x.copy()   # count i >= 3 is its difference plus count i - 2: running sums over the odd and over the even places
    out[1::2] = np.cumsum(x[1::2])
    out[2::2] = np.cumsum(x[2::2])
    return out


def rle_to_mask(string, h, w):
    """The (h, w) uint8 mask of a COCO run-length string."""
    c = rle_counts(string)
    if c.size and (c.min() < 0 or int(c.sum()) != h * w):
        raise ValueError("the counts do not describe a %d x %d mask" % (h, w))
    if c.size == 0 and h * w:
        raise ValueError("the counts do not describe a %d x %d mask" % (h, w))
    vals = (np.arange(c.size) & 1).astype(np.uint8)
    return np.repeat(vals, c).reshape(w, h).T.copy()


# ------------------------------------------------------------------------------------------------ COCO run-length codec (device)
# mpnhip_rle_decode_scan's status bits: what the host codec refuses, in the order it looks
RLE_BAD_CHAR, RLE_TRUNCATED, RLE_TOO_LONG, RLE_NEGATIVE, RLE_BAD_SUM = 1, 2, 4, 8, 16
RLE_UNREADABLE = RLE_BAD_CHAR | RLE_TRUNCATED | RLE_TOO_LONG   # ``rle_counts`` raises; the other two bits judge its counts


def rle_status_error(status):
    """The ``ValueError`` text ``rle_counts`` raises for a string with this status word, or None when it reads the string."""
    if status & RLE_BAD_CHAR:
        return "not a COCO run-length string"
    if status & RLE_TRUNCATED:
        return "truncated COCO run-length string"
    if status & RLE_TOO_LONG:
        return "count too long"
    return None


def rle_encode_events(event_pos, det_counts, hw):
    """``(bytes, str_ptr)`` on the device from the run boundaries ``mpnhip_mask_run_events`` leaves there (``event_pos`` [n_events],
    ``det_counts`` [n_dets], int32): the COCO strings of the entries one behind the other in a uint8 buffer of the size that always
    suffices, and their offsets [n_dets + 1] int64 (``mpnhip_rle_encode``).  No host read."""
    lib = capi.load()
    capi.require_device(event_pos, det_counts)
    if event_pos.dtype != torch.int32 or det_counts.dtype != torch.int32:
        raise MpnhipError("event_pos and det_counts must be int32")
    pos, cnt = event_pos.contiguous().view(-1), det_counts.contiguous().view(-1)
    n, e, dev = int(cnt.numel()), int(pos.numel()), cnt.device
    with torch.cuda.device(dev):
        cap = 7 * (n + e)
        data = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        str_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ws = capi.workspace(lib.mpnhip_rle_encode_workspace_bytes(n, e), dev, "rle_codec")
        check(lib.mpnhip_rle_encode(ptr(pos) if e else None, ptr(cnt) if n else None, n, e, int(hw), ptr(data), cap, ptr(str_ptr), ptr(ws),
                                    ws.numel(), stream_ptr()), "mpnhip_rle_encode")
    return data, str_ptr


@capi.on_tensor_device
def mask_run_strings(labels, num_dets):
    """The COCO strings of the masks ``labels == d`` for d in [0, num_dets), encoded on the device: ``(bytes, str_ptr)`` as host
    arrays (uint8, int64 [num_dets + 1]); ``rle_strings`` slices them.  ``labels`` [F, W, H] int32 as ``paste_unique_masks`` returns
    it.  Host reads: the number of events (it sizes the buffers, as in ``mask_run_events``), then the offsets and the bytes."""
    lib = capi.load()
    capi.require_device(labels)
    if labels.dtype != torch.int32 or labels.dim() != 3:
        raise MpnhipError("labels must be int32 [F, W, H]")
    lab = labels.contiguous()
    F, hw, n, dev = int(lab.shape[0]), int(lab.shape[1]) * int(lab.shape[2]), int(num_dets), lab.device
    counts = torch.zeros(n + 1, dtype=torch.int32, device=dev)   # [n]: the total
    ws = capi.workspace(lib.mpnhip_full_masks_workspace_bytes(n, F, hw, 0), dev, "full_masks")
    check(lib.mpnhip_mask_run_events_count(ptr(lab), F, hw, n, ptr(counts), ptr(counts[n:]), ptr(ws), ws.numel(), stream_ptr()),
          "mpnhip_mask_run_events_count")
    total = int(counts[n:].cpu()[0])
    pos = torch.empty(max(total, 1), dtype=torch.int32, device=dev)[:total]
    ws = capi.workspace(lib.mpnhip_full_masks_workspace_bytes(n, F, hw, total), dev, "full_masks")
    check(lib.mpnhip_mask_run_events(ptr(lab), F, hw, n, total, ptr(pos), ptr(ws), ws.numel(), stream_ptr()), "mpnhip_mask_run_events")
    data, str_ptr = rle_encode_events(pos, counts[:n], hw)
    sp = str_ptr.cpu().numpy()
    return data[:int(sp[-1])].cpu().numpy(), sp


def rle_strings(data, str_ptr):
    """The strings of a ``(bytes, str_ptr)`` pair as a list of ``str``: one decode, then slices"""
    sp = np.asarray(str_ptr, dtype=np.int64).reshape(-1).tolist()
    text = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).reshape(-1)).tobytes().decode("ascii")
    return [text[a:b] for a, b in zip(sp[:-1], sp[1:])]


def rle_decode_batch(strings, h, w, device):
    """The runs of set pixels of COCO strings, decoded on ``device`` (``mpnhip_rle_decode_scan`` / ``_runs``).  ``strings``: a
    list of ``str`` (ASCII), or an already joined ``(bytes, str_ptr)`` pair; ``h``, ``w``: the image size, one for all or one per
    string.  Returns a dict: ``n_counts``, ``n_runs``, ``area``, ``status`` [n] and ``run_ptr`` [n + 1] as host arrays (int64; the
    ``RLE_*`` bits say what the host codec refuses about a string, and such a string has no runs) and ``run_row``,
    ``run_begin``, ``run_end`` as int32 tensors on the device, ordered by string, then position -- what
    ``mots_eval.paint_label_runs`` takes.  An image of 2^31 pixels or more, or a negative size, is ``RLE_BAD_SUM``.  Host reads:
    the per-string numbers (they size the runs)."""
    lib = capi.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise MpnhipError("mpntrackseg_amd runs on a HIP device only (%s); there is no CPU fallback" % dev)
    if isinstance(strings, tuple):
        data = np.ascontiguousarray(np.asarray(strings[0], dtype=np.uint8).reshape(-1))
        sp = np.ascontiguousarray(np.asarray(strings[1], dtype=np.int64).reshape(-1))
    else:
        data = np.frombuffer("".join(strings).encode("ascii"), dtype=np.uint8)
        sp = np.zeros(len(strings) + 1, np.int64)
        np.cumsum(np.fromiter((len(s) for s in strings), np.int64, len(strings)), out=sp[1:])
    n = sp.size - 1
    if n < 0 or (n and int(sp[-1]) != data.size):
        raise MpnhipError("str_ptr needs one entry per string plus one, the last one the number of bytes")
    hs, ws_ = np.broadcast_to(np.asarray(h, np.int64), (n,)), np.broadcast_to(np.asarray(w, np.int64), (n,))
    hw = np.where((hs < 0) | (ws_ < 0), -1, hs * ws_).astype(np.int64)
    with torch.cuda.device(dev):
        buf = lambda count, dtype: torch.empty(max(int(count), 1), dtype=dtype, device=dev)[:int(count)]
        d_bytes, d_ptr, d_hw = buf(data.size, torch.uint8), torch.from_numpy(sp).to(dev), buf(n, torch.int64)
        d_bytes.copy_(torch.from_numpy(data.copy()))
        d_hw.copy_(torch.from_numpy(hw))
        small = buf(3 * n, torch.int32).view(3, n)   # n_counts, n_runs, status
        area = buf(n, torch.int64)
        check(lib.mpnhip_rle_decode_scan(ptr(d_bytes), data.size, ptr(d_ptr), ptr(d_hw), n, ptr(small[0]), ptr(small[1]), ptr(area),
                                         ptr(small[2]), stream_ptr()), "mpnhip_rle_decode_scan")
        small_h = small.cpu().numpy().astype(np.int64)
        total = int(small_h[1].sum())
        run_ptr = buf(n + 1, torch.int64)
        runs = buf(3 * total, torch.int32).view(3, total)
        ws = capi.workspace(lib.mpnhip_rle_decode_workspace_bytes(n), dev, "rle_codec")
        check(lib.mpnhip_rle_decode_runs(ptr(d_bytes), data.size, ptr(d_ptr), ptr(d_hw), n, ptr(small[1]), ptr(small[2]), total, ptr(run_ptr),
                                         ptr(runs[0]), ptr(runs[1]), ptr(runs[2]), ptr(ws), ws.numel(), stream_ptr()),
              "mpnhip_rle_decode_runs")
        return {"n_counts": small_h[0], "n_runs": small_h[1], "area": area.cpu().numpy(), "status": small_h[2],
                "run_ptr": run_ptr.cpu().numpy(), "run_row": runs[0], "run_begin": runs[1], "run_end": runs[2]}
