"""The reference of the weight-gradient products (include/mpnhip.h, mpnhip_debug_weight_grad_batch), evaluated from the same flat
description the entry takes.  For every group g, every batch b and every row r in [row_begin, row_end) intersected with [0, rows):

    z[o] = dZ[b * z_bstride + (dz_idx ? dz_idx[r] : r) * ldz + o]                                            o < n_out
    h[c] = c < csplit ? H[b * h_bstride + i * ldh + c] : H2[b * h2_bstride + i * ldh2 + c - csplit]          i = h_idx ? h_idx[r] : r
    grad_w[o][c] += z[o] * h[c]
    grad_b[o]    += z[o]

dz_idx / h_idx are the same for every batch.  ``bf16``: both operands of the product are rounded to nearest-even bf16, the bias sum
is not (as the kernels do).  tests/test_wgrad_reference_cpu.py pins this function against torch.autograd and a plain loop."""
import numpy as np
import torch


class Product:
    """One product as flat buffers: dZ / H / H2 are 1-D float32 CPU tensors whose element 0 is element [0, 0] of batch 0 (the
    values of bf16 source rows are held as float32 here); dz_idx / h_idx int tensors or None; groups: one or two
    (row_begin, row_end) pairs, None for "all rows"."""

    def __init__(self, dZ, ldz, z_bstride, H, ldh, h_bstride, rows, nbatch, n_out, k_in, groups=(None,), dz_idx=None, h_idx=None,
                 H2=None, ldh2=0, h2_bstride=0, csplit=None):
        self.dZ, self.ldz, self.z_bstride, self.dz_idx = dZ, ldz, z_bstride, dz_idx
        self.H, self.ldh, self.h_bstride, self.h_idx = H, ldh, h_bstride, h_idx
        self.H2, self.ldh2, self.h2_bstride = H2, ldh2, h2_bstride
        self.csplit = k_in if H2 is None else csplit
        self.rows, self.nbatch, self.n_out, self.k_in, self.groups = rows, nbatch, n_out, k_in, tuple(groups)
        assert 1 <= len(self.groups) <= 2 and (H2 is None or 0 < self.csplit < k_in)

    def group_rows(self, g):
        """the rows r of group g, ascending (int64)"""
        rb, re = (0, self.rows) if self.groups[g] is None else self.groups[g]
        return torch.arange(max(rb, 0), max(min(re, self.rows), max(rb, 0)), dtype=torch.int64)

    def operands(self, g, b):
        """(z [m, n_out], h [m, k_in]) of group g, batch b, float32, gathered from the flat buffers row by row"""
        r = self.group_rows(g)
        zi = self.dz_idx[r].long() if self.dz_idx is not None else r
        hi = self.h_idx[r].long() if self.h_idx is not None else r
        o, c1, c2 = torch.arange(self.n_out), torch.arange(self.csplit), torch.arange(self.k_in - self.csplit)
        z = self.dZ[(b * self.z_bstride + zi * self.ldz)[:, None] + o[None, :]]
        h = self.H[(b * self.h_bstride + hi * self.ldh)[:, None] + c1[None, :]]
        if self.H2 is not None:
            h = torch.cat([h, self.H2[(b * self.h2_bstride + hi * self.ldh2)[:, None] + c2[None, :]]], 1)
        return z, h


def reference(p, bf16=False, exact=False):
    """float64: per group (grad_w increment [n_out, k_in], grad_b increment [n_out]).  exact: asserts that the inputs are of the
    exact family (multiples of 1/4 in [-4, 4], few enough rows that every partial sum of sixteenths is an fp32 integer)."""
    out = []
    for g in range(len(p.groups)):
        gw = torch.zeros((p.n_out, p.k_in), dtype=torch.float64)
        gb = torch.zeros(p.n_out, dtype=torch.float64)
        for b in range(p.nbatch):
            z, h = p.operands(g, b)
            if exact:
                for t in (z, h):
                    assert bool(((t * 4).round() == t * 4).all()) and (t.numel() == 0 or float(t.abs().max()) <= 4.0)
            zp, hp = (z.to(torch.bfloat16), h.to(torch.bfloat16)) if bf16 else (z, h)
            gw += zp.double().t() @ hp.double()
            gb += z.double().sum(0)
        out.append((gw, gb))
    if exact:
        # every product is a multiple of 1/16 below 16 in size: |any partial sum| * 16 <= rows * nbatch * 256 (+ 64 for old contents of
        # the same family), an integer below 2^24 -- representable in fp32 whatever the order of the additions
        assert p.rows * p.nbatch * 256 + 64 < 2 ** 24
    return out


def reference_float32(p, bf16=False):
    """The same sums in float32, sequential over the rows (batch after batch): the error of a plain fp32 evaluation of the same
    case, the yardstick of the tolerances."""
    out = []
    for g in range(len(p.groups)):
        gw = np.zeros((p.n_out, p.k_in), dtype=np.float32)
        gb = np.zeros(p.n_out, dtype=np.float32)
        for b in range(p.nbatch):
            z, h = p.operands(g, b)
            zp, hp = (z.to(torch.bfloat16).float(), h.to(torch.bfloat16).float()) if bf16 else (z, h)
            zp, hp, zn = zp.numpy(), hp.numpy(), z.numpy()
            for r in range(zp.shape[0]):
                gw += zp[r][:, None] * hp[r][None, :]
                gb += zn[r]
        out.append((torch.from_numpy(gw), torch.from_numpy(gb)))
    return out
