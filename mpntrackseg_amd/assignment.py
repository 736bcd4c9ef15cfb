"""Batched rectangular linear sum assignment on the device (``csrc/assignment.hip``, ``mpnhip_lsa_batched``): what
``scipy.optimize.linear_sum_assignment`` solves, for many problems in one launch and without leaving the device.  One wavefront
per problem runs the shortest augmenting path of Crouse 2016 (scipy's algorithm) in float64 with the problem's state in LDS; the
layout, the tie rule and the status codes are in ``include/mpnhip.h``.  Where a problem's optimum is unique the pairs are scipy's;
among ties (equal totals) they need not be."""
import numpy as np
import torch

from . import capi
from .capi import MpnhipError, check, ptr, stream_ptr

MAX_SIDE = 2048   # MPNHIP_LSA_MAX_SIDE: the most kept rows, or kept columns, of one problem
STATUS = {1: "the costs are not finite (a NaN, or no column at a finite distance)",
          2: "more than %d kept rows or kept columns" % MAX_SIDE, 3: "the problem's cells do not lie inside cost"}


def _list(v, dtype, dev):
    """a pointer list as a device tensor and, where the caller gave it as a host array, its last entry"""
    if isinstance(v, torch.Tensor):
        return v.to(device=dev, dtype=dtype).contiguous().view(-1), None
    h = np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.int64)
    return torch.from_numpy(h).to(device=dev, dtype=dtype), (int(h[-1]) if h.size else 0)


def _keep(v, dev):
    """a keep mask as uint8 on the device; a bool tensor (one byte per flag, 0 / 1) is taken as it is"""
    if v is None:
        return None
    v = v.to(device=dev).contiguous().view(-1)
    return v.view(torch.uint8) if v.dtype == torch.bool else (v if v.dtype == torch.uint8 else v.ne(0).view(torch.uint8))


@capi.on_tensor_device
def linear_sum_assignment_batched(cost, cell_ptr, a_ptr, b_ptr, a_keep=None, b_keep=None, maximize=False):
    """One launch of ``mpnhip_lsa_batched``.  ``cost`` (float64, device): problem f owns ``na_f x nb_f`` cells at ``cell_ptr[f]``,
    cell ``[ia * nb_f + ib]``, with ``na_f = a_ptr[f + 1] - a_ptr[f]`` and ``nb_f`` likewise -- the layout of ``hota_eval``'s
    ``sim``, ``sim_ptr``, ``a_ptr`` and ``b_ptr``.  ``a_keep`` / ``b_keep`` (device, one flag per entry of either list): the rows and
    columns that take part; None: all.  Returns ``(match_b, match_a, status)``, int32 device tensors: the b-entry (index into the
    whole list) of every a-entry or -1, the inverse, and 0 per solved problem (the other codes: ``STATUS``).

    Nothing is read back from the device: the number of entries of a list is that of its keep mask, or the last entry of a
    pointer list given as a host array; a device list without a mask is refused."""
    lib = capi.load()
    capi.require_device(cost)
    dev = cost.device
    if cost.dtype != torch.float64:
        raise MpnhipError("cost must be float64 (%s)" % cost.dtype)
    cost = cost.contiguous().view(-1)
    (cp, _), (ap, a_last), (bp, b_last) = _list(cell_ptr, torch.int64, dev), _list(a_ptr, torch.int32, dev), _list(b_ptr, torch.int32, dev)
    ka, kb = _keep(a_keep, dev), _keep(b_keep, dev)
    sizes = []
    for keep, last, name in ((ka, a_last, "a"), (kb, b_last, "b")):
        if keep is None and last is None:
            raise MpnhipError("%s_ptr is on the device: give %s_keep (the list's last entry is not read back)" % (name, name))
        if keep is not None and last is not None and keep.numel() != last:
            raise MpnhipError("one keep flag per %s-entry" % name)
        sizes.append(keep.numel() if keep is not None else last)
    F = ap.numel() - 1
    if F < 0 or bp.numel() != F + 1 or cp.numel() != F + 1:
        raise MpnhipError("cell_ptr, a_ptr and b_ptr need one entry per problem plus one")
    need = lib.mpnhip_lsa_workspace_bytes(sizes[0], sizes[1], F)
    if need == 0:
        raise MpnhipError("%d x %d entries in %d problems are not supported" % (sizes[0], sizes[1], F))
    ws = capi.workspace(need, dev, "lsa")
    match_b, match_a = (torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n] for n in sizes)   # (the call fills them with -1)
    status = torch.zeros(max(F, 1), dtype=torch.int32, device=dev)[:F]
    if F == 0:   # (no problem: the call is a no-op)
        match_b.fill_(-1), match_a.fill_(-1)
    check(lib.mpnhip_lsa_batched(ptr(cost), cost.numel(), ptr(cp), ptr(ap), sizes[0], ptr(bp), sizes[1], F, ptr(ka), ptr(kb),
                                 1 if maximize else 0, ptr(match_b), ptr(match_a), ptr(status), ptr(ws), ws.numel(), stream_ptr()),
          "mpnhip_lsa_batched")
    return match_b, match_a, status


def raise_on_status(status, what="linear_sum_assignment"):
    """``MpnhipError`` naming the first problem of ``status`` (a device tensor; this reads it) that was not solved"""
    st = status.cpu().numpy()
    bad = np.flatnonzero(st)
    if bad.size:
        raise MpnhipError("%s: problem %d of %d: %s" % (what, int(bad[0]), st.size, STATUS.get(int(st[bad[0]]), "status %d" % st[bad[0]])))


def linear_sum_assignment(cost_2d, maximize=False):
    """``scipy.optimize.linear_sum_assignment`` for one matrix on the device: ``(row_ind, col_ind)``, int64 host arrays, rows
    ascending.  Raises ``MpnhipError`` where the operator's status is not 0 (costs that are not finite, a side over ``MAX_SIDE``)."""
    capi.require_device(cost_2d)
    if cost_2d.dim() != 2:
        raise MpnhipError("expected a matrix (%d-D)" % cost_2d.dim())
    na, nb = (int(v) for v in cost_2d.shape)
    match_b, _, status = linear_sum_assignment_batched(cost_2d.to(torch.float64), [0, na * nb], [0, na], [0, nb], maximize=maximize)
    raise_on_status(status)
    mb = match_b.cpu().numpy().astype(np.int64)
    rows = np.flatnonzero(mb >= 0)
    return rows, mb[rows]
