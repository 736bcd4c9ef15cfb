"""Operator-level parity of the weight-gradient products as mpnhip_backward issues them: mpnhip_debug_weight_grad_batch runs the
backward's own routing (csrc/wgrad.hip: weight_grad_route) over the row-panel kernels (csrc/wgrad_panel.hip), the LDS-DMA kernel
over bf16 rows (csrc/wgrad_rows16.hip) and the four fp32 kernels behind launch_gemm_tn, against ONE float64 CPU reference of the
documented formula (tests/wgrad_ref.py, pinned by tests/test_wgrad_reference_cpu.py).

Every grad_w lives inside a larger finite random matrix (3 guard rows above and below, at least 8 guard columns: ldw >= k_in + 8),
every grad_b between 8 guard elements; everything the reference does not write is compared bit for bit with the prefill.  Operand
paddings (ldz - n_out, ldh - k_in) and the rows of an ungathered operand that belong to no row range hold NaN, and the workspace
(the slabs) is prefilled with NaN: an empty chunk's slab is never written and the slab sum must skip it.

Input families.  EXACT: every operand (and the old contents of grad_w / grad_b) is a multiple of 1/4 in [-4, 4], so every product is
a multiple of 1/16 and -- the reference asserts rows * nbatch * 256 < 2^24 -- every partial sum is an fp32 integer of sixteenths;
the values are exact in bf16 and their second and third split pieces are zero, so the result must equal float64 BIT FOR BIT in all
three operand forms whatever the chunking, the sign alternation or the tile shape, and a missing, duplicated or misattributed row
moves it by at least 1/16.  NORMAL: synth.normal inputs, max |got - ref| / max |ref| < 3e-6 (the bound tests/test_gpu_wgrad.py holds
these kernels to) against float64 -- for the bf16 forms against the float64 product of the bf16-rounded operands --, separately for
grad_w and grad_b.  One exception: the bias of a [1 x k] product is a single element, a sum of few cancelling terms that is its own
max |ref| (31 rows x 2 batches: 5.0e-05 on an MI355X); it alone is held to max(3e-6, 4 x the error of the float32 CPU evaluation of the
same sum, sequential over the rows), as tests/test_gpu_gemm.py does for its split cases.  Labelled normal cases print the kernel's
error and the float32 evaluation's (DESIGN.md section 2 keeps the table of an MI355X run).

Every call asserts what ran from literals: the ``chosen`` report of the entry (path, variant after any narrow re-tiling, tiles,
chunk, nsplit, narrow, rolled, xcd_map, red_ny) and the nine weight-gradient path counters."""

import numpy as np
import pytest
import torch

from mpntrackseg_amd import capi, synth
from wgrad_ref import Product, reference, reference_float32

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
GR, GC, GB = 3, 8, 8          # guard rows above and below grad_w / minimum guard columns / guard elements around grad_b
TOL = 3e-6
COUNTERS = ("gemm_tn_mfma", "gemm_tn_small", "gemm_tn_generic", "gemm_tn_panel", "wgrad_panel_launches", "wgrad_panel_narrow_launches",
            "wgrad_panel_fallback", "wgrad_rows16", "wgrad_rows16_launches")
NAN = float("nan")


def counts(**kw):
    d = dict.fromkeys(COUNTERS, 0)
    d.update(kw)
    return d


def bits(t):
    return t.contiguous().view(torch.int32)


def values(family, seed, shape, stream):
    n = int(np.prod(shape))
    if family == "exact":
        v = np.round(synth.uniform01(seed, n, stream=stream) * 32.0 - 16.0) / 4.0
        return torch.from_numpy(v.astype(np.float32)).reshape(shape)
    return torch.from_numpy(synth.normal(seed, shape, stream=stream))


def upload(t, ld, off, b16):
    """t [nb, r, c] (CPU, float32) -> (CPU flat buffer from element [0, 0, 0] on, leading dimension ld, NaN in the padding; the
    device tensor that owns the memory; the device address of element [0, 0, 0], `off` elements behind an aligned address; the
    batch stride).  b16: the device image holds bf16 rows (the CPU buffer their values as float32)."""
    nb, r, c = t.shape
    buf = torch.full((off + nb * r * ld,), NAN, dtype=torch.float32)
    buf[off:].view(nb, r, ld)[:, :, :c] = t
    if b16:
        d = buf.to(torch.bfloat16)
        buf = d.float()
        d = d.to(dev())
    else:
        d = buf.to(dev())
    return buf[off:], d, d.data_ptr() + d.element_size() * off, r * ld


class Case:
    """One product: operands on the CPU (flat, as the reference reads them) and on the device, prefilled outputs, references."""

    def __init__(self, n_out, k_in, rows, nbatch=1, family="exact", src16=False, groups=(None,), csplit=None, dz_idx=None, h_idx=None,
                 z_b0=False, h_b0=False, ldz_pad=0, ldh_pad=0, ldw_pad=GC, bias=True, off=0, seed=1):
        self.n_out, self.k_in, self.rows, self.nbatch, self.family, self.src16 = n_out, k_in, rows, nbatch, family, src16
        self.groups, self.bias = tuple(groups), bias
        assert ldw_pad >= GC and all(g is None or 0 <= g[0] <= g[1] <= rows for g in groups)
        self.keep = keep = []

        def idx(kind, stream):
            if kind is None:
                return None, rows
            if kind == "perm":
                return torch.from_numpy(np.argsort(synth.uniform01(seed, rows, stream=stream)).astype(np.int32)), rows
            T = max(2, rows // 3 + 1)       # a shorter table: source rows repeat
            return torch.from_numpy((synth.uniform01(seed, rows, stream=stream) * T).astype(np.int32)), T
        self.dz_idx, RZ = idx(dz_idx, 11)
        self.h_idx, RH = idx(h_idx, 12)
        Z = values(family, seed, (1 if z_b0 else nbatch, RZ, n_out), 1)
        H = values(family, seed, (1 if h_b0 else nbatch, RH, k_in), 2)
        if src16:       # (the [1 x k] form keeps an fp32 dZ, values that bf16 does not hold: the product rounds them, the bias sum does not)
            Z, H = (Z if n_out == 1 else Z.to(torch.bfloat16).float()), H.to(torch.bfloat16).float()
        # rows of an ungathered operand that belong to no range must never be read: NaN
        inside = torch.zeros(rows, dtype=torch.bool)
        for g in self.groups:
            b, e = (0, rows) if g is None else g
            inside[b:e] = True
        if self.dz_idx is None:
            Z[:, ~inside] = NAN
        if self.h_idx is None:
            H[:, ~inside] = NAN
        z16 = src16 and n_out != 1          # (the [1 x k] form keeps an fp32 dZ)
        cs = k_in if csplit is None else csplit
        zc, zd, zp, zs = upload(Z, n_out + ldz_pad, off, z16)
        hc, hd, hp, hs = upload(H[:, :, :cs].contiguous(), cs + ldh_pad, off, src16)
        h2c = h2p = None
        h2s = ld2 = 0
        if csplit is not None:
            ld2 = k_in - cs + 4
            h2c, h2d, h2p, h2s = upload(H[:, :, cs:].contiguous(), ld2, 0, False)
            keep.append(h2d)
        zs, hs, h2s = (0 if z_b0 else zs), (0 if h_b0 else hs), (0 if h_b0 else h2s)
        keep += [zd, hd]
        self.ref_product = Product(zc, n_out + ldz_pad, zs, hc, cs + ldh_pad, hs, rows, nbatch, n_out, k_in, groups=self.groups,
                                   dz_idx=self.dz_idx, h_idx=self.h_idx, H2=h2c, ldh2=ld2, h2_bstride=h2s, csplit=csplit)
        p = self.c = capi.WgradProduct()
        p.dZ, p.ldz, p.z_bstride, p.H, p.ldh, p.h_bstride = zp, n_out + ldz_pad, zs, hp, cs + ldh_pad, hs
        p.H2, p.ldh2, p.h2_bstride, p.csplit = h2p, ld2, h2s, (cs if csplit is not None else 0)
        self.ldw = k_in + ldw_pad
        p.ldw, p.rows, p.n_out, p.k_in, p.nbatch, p.src16 = self.ldw, rows, n_out, k_in, nbatch, int(src16)
        for name, t in (("dz_idx", self.dz_idx), ("h_idx", self.h_idx)):
            if t is not None:
                d = t.to(dev())
                keep.append(d)
                setattr(p, name, d.data_ptr())
        ranges = torch.tensor([x for g in self.groups for x in (g if g is not None else (0, rows))], dtype=torch.int32, device=dev())
        keep.append(ranges)
        self.old_w, self.old_b, self.w, self.b = [], [], [], []
        for q, g in enumerate(self.groups):
            ow = values(family, seed, (n_out + 2 * GR, self.ldw), 20 + q).to(dev())
            ob = values(family, seed, (n_out + 2 * GB,), 30 + q).to(dev())
            self.old_w.append(ow); self.old_b.append(ob); self.w.append(ow.clone()); self.b.append(ob.clone())
            p.g[q].grad_w = self.w[q].data_ptr() + 4 * GR * self.ldw
            p.g[q].grad_b = self.b[q].data_ptr() + 4 * GB if bias else None
            if g is not None:
                p.g[q].row_begin, p.g[q].row_end = ranges.data_ptr() + 8 * q, ranges.data_ptr() + 8 * q + 4
        self.ref = {}

    def reset(self):
        for q in range(len(self.groups)):
            self.w[q].copy_(self.old_w[q]); self.b[q].copy_(self.old_b[q])

    def reference(self, bf16):
        if bf16 not in self.ref:
            self.ref[bf16] = reference(self.ref_product, bf16=bf16, exact=self.family == "exact")
        return self.ref[bf16]

    def untouched(self):
        return all(torch.equal(bits(self.w[q]), bits(self.old_w[q])) and torch.equal(bits(self.b[q]), bits(self.old_b[q]))
                   for q in range(len(self.groups)))

    def snapshot(self):
        return [(self.w[q].cpu().clone(), self.b[q].cpu().clone()) for q in range(len(self.groups))]

    def verify(self, name, prec, label=None):
        """guards bit for bit; the written part against float64: exactly (exact family) or within TOL (normal family)"""
        bf16 = prec == "bf16"
        ref = self.reference(bf16)
        worst, worst32, r32 = 0.0, 0.0, None
        for q in range(len(self.groups)):
            got_w, old_w, got_b, old_b = self.w[q].cpu(), self.old_w[q].cpu(), self.b[q].cpu(), self.old_b[q].cpu()
            mw = torch.zeros_like(got_w, dtype=torch.bool)
            mw[GR:GR + self.n_out, :self.k_in] = True
            mb = torch.zeros_like(got_b, dtype=torch.bool)
            if self.bias:
                mb[GB:GB + self.n_out] = True
            assert torch.equal(bits(got_w)[~mw], bits(old_w)[~mw]), (name, q, "grad_w: wrote outside [n_out, k_in]")
            assert torch.equal(bits(got_b)[~mb], bits(old_b)[~mb]), (name, q, "grad_b: wrote outside [n_out] (or a null grad_b)")
            want_w = old_w[GR:GR + self.n_out, :self.k_in].double() + ref[q][0]
            want_b = old_b[GB:GB + self.n_out].double() + ref[q][1]
            g_w, g_b = got_w[GR:GR + self.n_out, :self.k_in].double(), got_b[GB:GB + self.n_out].double()
            assert torch.isfinite(g_w).all() and torch.isfinite(g_b).all(), (name, q, "non-finite output")
            if self.family == "exact":
                bad = (g_w != want_w)
                assert not bad.any(), (name, q, "grad_w differs from float64", int(bad.sum()), float((g_w - want_w).abs().max()))
                if self.bias:
                    assert torch.equal(g_b, want_b), (name, q, "grad_b differs from float64", float((g_b - want_b).abs().max()))
            else:
                if r32 is None:
                    r32 = reference_float32(self.ref_product, bf16=bf16)
                sw, sb = max(float(ref[q][0].abs().max()), 1e-30), max(float(ref[q][1].abs().max()), 1e-30)
                e_w = float((g_w - want_w).abs().max()) / sw
                e_b = float((g_b - want_b).abs().max()) / sb if self.bias else 0.0
                f_w = float((r32[q][0].double() - ref[q][0]).abs().max()) / sw
                f_b = float((r32[q][1].double() - ref[q][1]).abs().max()) / sb if self.bias else 0.0
                worst, worst32 = max(worst, e_w, e_b), max(worst32, f_w, f_b)
                # 3e-6 everywhere.  One exception: grad_b of a [1 x k] product is ONE element, a sum of few terms that cancel, and max |ref|
                # is that sum itself -- there 4 x the error of the float32 CPU evaluation of the same sum where that is more (never from
                # the kernel's own output)
                tol_b = max(TOL, 4.0 * f_b) if self.n_out == 1 else TOL
                assert e_w < TOL and e_b < tol_b, (name, q, e_w, f_w, e_b, f_b)
        if self.family != "exact" and label:
            print("WGRAD_ERR [%s] %s: kernel %.2e  float32-cpu %.2e" % (label, name, worst, worst32))
        return worst


def run(cases, prec, batched=False, one_launch=False, slab=0, rc=0):
    """-> (chosen per case: list of two dicts, the nine counters)"""
    for c in cases:
        c.reset()
    capi.path_counters(reset=True)
    got, chosen = capi.debug_weight_grad_batch([c.c for c in cases], prec, batched=batched, one_launch=one_launch, batch_slab_floats=slab,
                                               fill=0xFF)
    assert got == rc, (got, rc, capi.load().mpnhip_last_error())
    cnt = capi.path_counters(reset=True)
    return chosen, {k: cnt[k] for k in COUNTERS}


def ch(path, variant=0, to=1, tc=1, chunk=256, nsplit=1, narrow=0, rolled=0, xcd_map=0, red_ny=0):
    return dict(path=path, variant=variant, tiles_o=to, tiles_c=tc, chunk=chunk, nsplit=nsplit, narrow=narrow, rolled=rolled,
                xcd_map=xcd_map, red_ny=red_ny)


NONE = ch(None, 0, 0, 0, 0, 0)


def single(case, prec, expect, cnt, name, label=None, **kw):
    """one product, one call: chosen of group 0 (and 1, if the case has two) == expect, counters == cnt, result verified"""
    chosen, got = run([case], prec, **kw)
    want = [expect, expect if len(case.groups) == 2 else NONE]
    assert chosen[0] == want, (name, chosen[0], want)
    assert got == cnt, (name, got, cnt)
    case.verify(name, prec, label)


def panel_counts(narrow, jobs=1):
    return counts(gemm_tn_panel=jobs, wgrad_panel_launches=1, wgrad_panel_narrow_launches=narrow)


# ------------------------------------------------------------------------------------ row counts at the pipeline boundaries
# the partial chunk holds nfull = 0 .. 9 full 16-row stages with tails of 0, 1 and 15 rows
ROWS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 95, 96, 112, 113, 128, 129, 144, 145]
# (n_out, k_in) -> variant, tiles_o, tiles_c, narrow launch, by hand from wp_choose: cost = tiles x (BO + BC) (+ tiles on a tie) over
# <5,1> <1,5> <4,1> <1,1> <2,2>; [80 x 32] is ONE partial <2,2> tile (256 + 1 against 2 x 128 + 2), [8 x 16] is a small shape
# (k_in <= 32, n_out <= 32: variant 7), not a partial MFMA tile; a launch whose jobs are all <1,1> / [1 x k] / small runs narrow
PANEL_SHAPES = [(320, 64, 0, 1, 1, 0), (64, 320, 1, 1, 1, 0), (224, 64, 2, 1, 1, 0), (128, 224, 5, 1, 2, 0), (64, 64, 3, 1, 1, 1),
                (80, 32, 5, 1, 1, 0), (56, 16, 3, 1, 1, 1), (8, 16, 7, 1, 1, 1)]


@pytest.mark.parametrize("prec", ["fp32_split", "bf16"])
@pytest.mark.parametrize("n_out,k_in,variant,to,tc,narrow", PANEL_SHAPES)
def test_row_boundaries_row_panel(n_out, k_in, variant, to, tc, narrow, prec):
    """every row count alone in its chunk, as the odd (negated) chunk behind one full 256-row chunk and as the even chunk behind
    two; D = 1 (<5,1>, <1,5>: the split form's pair-unrolled loop), D = 2 (<4,1>, <2,2>) and D = 4 (<1,1>) stages in flight"""
    for head in (0, 256, 512):
        for r in ROWS:
            rows = head + r
            c = Case(n_out, k_in, rows, family="exact", seed=rows)
            single(c, prec, ch("panel", variant, to, tc, 256, head // 256 + 1, narrow), panel_counts(narrow), (n_out, k_in, rows, prec))
    for rows in (17, 256 + 49, 512 + 145):
        c = Case(n_out, k_in, rows, family="normal", seed=rows)
        single(c, prec, ch("panel", variant, to, tc, 256, -(-rows // 256), narrow), panel_counts(narrow), (n_out, k_in, rows, prec),
               label="panel " + prec)


# bf16 source rows: variants 8 .. 15 = <5,2> <2,5> <4,2> <2,4> <1,2> <2,1> <1,1> <2,2> (by hand from wp_choose's cost: staged columns
# per row first).  ldz = n_out + 4 is no multiple of 8, which keeps [320 x 128] off the LDS-DMA kernel (it would take variant 18)
ROWS16_SHAPES = [(320, 128, 8), (64, 320, 9), (224, 64, 10), (128, 224, 11), (64, 128, 12), (80, 16, 13), (32, 64, 14), (128, 128, 15)]


@pytest.mark.parametrize("n_out,k_in,variant", ROWS16_SHAPES)
def test_row_boundaries_bf16_rows(n_out, k_in, variant):
    for head in (0, 256, 512):
        for r in ROWS:
            rows = head + r
            c = Case(n_out, k_in, rows, family="exact", src16=True, ldz_pad=4, seed=rows)
            single(c, "bf16", ch("panel", variant, 1, 1, 256, head // 256 + 1), panel_counts(0), (n_out, k_in, rows))
    for rows in (17, 512 + 145):
        c = Case(n_out, k_in, rows, family="normal", src16=True, ldz_pad=4, seed=rows)
        single(c, "bf16", ch("panel", variant, 1, 1, 256, -(-rows // 256)), panel_counts(0), (n_out, k_in, rows), label="panel bf16 rows")


@pytest.mark.parametrize("n_out,k_in,variant,tc", [(640, 128, 16, 1), (128, 640, 17, 1), (448, 128, 18, 1), (256, 448, 19, 2)])
def test_row_boundaries_rows16(n_out, k_in, variant, tc):
    """the LDS-DMA kernel's 4-stage ring: nfull = 0 .. 6 with tails 0, 1, 15; alone, odd and even chunk"""
    cnt = counts(gemm_tn_panel=1, wgrad_panel_launches=1, wgrad_rows16=1, wgrad_rows16_launches=1)
    for head in (0, 256, 512):
        for r in [x for x in ROWS if x <= 97] + [111, 112]:
            rows = head + r
            c = Case(n_out, k_in, rows, family="exact", src16=True, seed=rows)
            single(c, "bf16", ch("rows16", variant, 1, tc, 256, head // 256 + 1), cnt, (n_out, k_in, rows))
    for rows in (17, 512 + 97):
        c = Case(n_out, k_in, rows, family="normal", src16=True, seed=rows)
        single(c, "bf16", ch("rows16", variant, 1, tc, 256, -(-rows // 256)), cnt, (n_out, k_in, rows), label="rows16")


# ------------------------------------------------------------------------------------ device-side row ranges, two groups
def range_sets(rows):
    mid = rows // 2 | 1
    return [((0, 0), (0, rows)), ((0, rows), (rows, rows)), ((0, 1), (1, rows)), ((0, rows - 1), (rows - 1, rows)), ((0, 17), (17, rows)),
            ((0, mid), (mid, rows)), ((0, mid - 40), (mid + 23, rows - 5))]


# ranged jobs plan their chunks for rows / 2 expected rows (256 here) and cut nsplit = ceil(rows / 256) slabs: a group shorter than
# (nsplit - 1) chunks leaves slabs unwritten (nvalid < nsplit) -- every set above has such a group
@pytest.mark.parametrize("kind,n_out,k_in,prec,expect", [
    ("panel", 320, 64, "fp32_split", ch("panel", 0, 1, 1, 256, 3)),
    ("panel", 64, 64, "bf16", ch("panel", 3, 1, 1, 256, 3, narrow=1)),
    ("panel16", 224, 64, "bf16", ch("panel", 10, 1, 1, 256, 3)),
    ("rows16", 448, 128, "bf16", ch("rows16", 18, 1, 1, 256, 3)),
    ("fp32", 320, 64, "fp32", ch("tn_mfma", 64, 5, 1, 128, 5, xcd_map=1, red_ny=1)),
    ("fp32", 18, 18, "fp32", ch("tn_small", 0, 1, 1, 64, 10, red_ny=1)),
    ("fp32", 320, 128, "fp32", ch("tn_mfma", 128, 5, 1, 128, 5, xcd_map=1, red_ny=1)),
    ("fp32", 64, 128, "fp32", ch("tn_mfma", 128, 1, 1, 128, 5, red_ny=1)),
    ("fp32", 72, 6, "fp32", ch("tn_narrowk", 0, 1, 1, 128, 5, red_ny=1)),
    ("fp32", 40, 18, "fp32", ch("tn_generic", 0, 1, 1, 128, 5, red_ny=1)),
])
def test_row_ranges(kind, n_out, k_in, prec, expect):
    rows = 601
    src16 = kind in ("panel16", "rows16")
    for fam in ("exact", "normal"):
        for gi, groups in enumerate(range_sets(rows)):
            c = Case(n_out, k_in, rows, nbatch=2, family=fam, src16=src16, groups=groups, ldz_pad=4 if kind == "panel16" else 0, seed=gi + 1)
            if kind == "fp32":
                cnt = counts(**{{"tn_mfma": "gemm_tn_mfma", "tn_small": "gemm_tn_small"}.get(expect["path"], "gemm_tn_generic"): 1})
            elif kind == "rows16":
                cnt = counts(gemm_tn_panel=2, wgrad_panel_launches=1, wgrad_rows16=2, wgrad_rows16_launches=1)
            else:
                cnt = panel_counts(expect["narrow"], jobs=2)
            single(c, prec, expect, cnt, (kind, n_out, k_in, groups, fam), label="ranges " + kind if gi == 5 else None)


# ------------------------------------------------------------------------------------ strides, wider grad_w, null bias
@pytest.mark.parametrize("n_out,k_in,prec,src16,expect", [
    (320, 64, "fp32_split", False, ch("panel", 0, 1, 1, 256, 2)),
    (64, 64, "bf16", False, ch("panel", 3, 1, 1, 256, 2, narrow=1)),
    (128, 128, "bf16", True, ch("panel", 15, 1, 1, 256, 2)),
    (320, 64, "fp32", False, ch("tn_mfma", 64, 5, 1, 128, 3, xcd_map=1, red_ny=1)),
    (72, 6, "fp32", False, ch("tn_narrowk", 0, 1, 1, 128, 3, red_ny=1)),
])
def test_strides(n_out, k_in, prec, src16, expect):
    rows, nb = 300, 3
    fp32 = prec == "fp32"
    cnt = counts(**{("gemm_tn_mfma" if expect["path"] == "tn_mfma" else "gemm_tn_generic"): 1}) if fp32 else panel_counts(expect["narrow"])
    variants = [dict(z_b0=True, h_b0=True), dict(z_b0=True), dict(h_b0=True), dict(ldz_pad=4, ldh_pad=8), dict(ldw_pad=12),
                dict(bias=False), dict(z_b0=True, h_b0=True, ldz_pad=4, ldh_pad=8, ldw_pad=12, bias=False)]
    for fam in ("exact", "normal"):
        for i, kw in enumerate(variants):
            c = Case(n_out, k_in, rows, nbatch=nb, family=fam, src16=src16, seed=i + 1, **kw)
            single(c, prec, expect, cnt, (n_out, k_in, prec, fam, kw), label="strides " + prec if i == 6 else None)
            if i == 0 and fam == "exact":
                # the same block every batch: 3 x one batch, exactly
                one = Case(n_out, k_in, rows, nbatch=1, family=fam, src16=src16, seed=i + 1)
                r1, r3 = one.reference(False), c.reference(False)
                assert torch.equal(r3[0][0], 3 * r1[0][0]) and torch.equal(r3[0][1], 3 * r1[0][1])


# ------------------------------------------------------------------------------------ H2 / csplit
@pytest.mark.parametrize("csplit", [4, 32, 60, 64, 68, 124])
@pytest.mark.parametrize("n_out,prec,expect", [
    (320, "fp32_split", ch("panel", 0, 1, 2, 256, 2)),
    (320, "bf16", ch("panel", 0, 1, 2, 256, 2)),
    (64, "fp32_split", ch("panel", 5, 1, 1, 256, 2)),
    (64, "bf16", ch("panel", 5, 1, 1, 256, 2)),
    (64, "fp32", ch("tn_mfma", 128, 1, 1, 128, 3, red_ny=1)),
    (320, "fp32", ch("tn_mfma", 128, 5, 1, 128, 3, xcd_map=1, red_ny=1)),
])
def test_csplit(n_out, prec, expect, csplit):
    """k_in = 128: the split inside a 64-column tile, on its edge and beside it; per-thread segment choice in wp_block"""
    cnt = counts(gemm_tn_mfma=1) if prec == "fp32" else panel_counts(0)
    for fam in ("exact", "normal"):
        for kw in (dict(), dict(h_b0=True, nbatch=2)):
            c = Case(n_out, 128, 300, family=fam, csplit=csplit, seed=csplit, **kw)
            single(c, prec, expect, cnt, (n_out, prec, csplit, fam, kw), label="csplit " + prec if csplit == 60 and not kw else None)


@pytest.mark.parametrize("prec,expect", [("fp32_split", ch("panel", 3, 1, 1, 256, 2, narrow=1)),
                                         ("fp32", ch("tn_mfma", 64, 1, 1, 128, 3, red_ny=1))])
def test_csplit_k64(prec, expect):
    cnt = counts(gemm_tn_mfma=1) if prec == "fp32" else panel_counts(1)
    for fam in ("exact", "normal"):
        c = Case(64, 64, 300, family=fam, csplit=32, seed=3)
        single(c, prec, expect, cnt, (prec, fam), label="csplit " + prec)


# ------------------------------------------------------------------------------------ gathers and the narrow kernels
@pytest.mark.parametrize("k_in", [4, 32, 64])
@pytest.mark.parametrize("prec,src16", [("fp32_split", False), ("bf16", False), ("bf16", True)])
def test_one_by_k(k_in, prec, src16):
    """wp_block_vec: [1 x k], k / 4 threads per row, rl = 1024 / k row lanes, eight rows in flight per thread; dZ (fp32 also over bf16
    H rows) optionally through a permutation"""
    rl = 1024 // k_in
    for rows in sorted({1, rl - 1, rl, rl + 1, 8 * rl - 1, 8 * rl, 8 * rl + 1, 8 * rl + 300}):
        for gather in (None, "perm"):
            for fam in ("exact", "normal"):
                c = Case(1, k_in, rows, nbatch=2, family=fam, src16=src16, dz_idx=gather, seed=rows)
                narrow = 0 if src16 else 1      # (a launch with a job over bf16 rows is never the narrow one: wp_batch_flush)
                single(c, prec, ch("panel", 6, 1, 1, 256, -(-rows // 256), narrow=narrow), panel_counts(narrow), (k_in, rows, gather, prec, src16, fam),
                       label="[1 x k]" if rows == 8 * rl + 300 and gather else None)


SMALL = [(18, 18), (18, 6), (72, 6), (32, 32), (16, 5)]


@pytest.mark.parametrize("n_out,k_in", SMALL)
@pytest.mark.parametrize("prec", ["fp32_split", "bf16"])
def test_small_shapes_panel(n_out, k_in, prec):
    """wp_block_small: any alignment (operands 4 bytes off a 16-byte boundary), either operand gathered"""
    for rows in (1, 63, 64, 65, 129):
        for dz, hi in (("perm", None), (None, "gather"), ("gather", "perm")):
            for fam in ("exact", "normal"):
                c = Case(n_out, k_in, rows, nbatch=2, family=fam, dz_idx=dz, h_idx=hi, off=1, seed=rows)
                single(c, prec, ch("panel", 7, 1, 1, 256, 1, narrow=1), panel_counts(1), (n_out, k_in, rows, dz, hi, prec, fam),
                       label="small " + prec if rows == 129 and dz == "gather" else None)


# the same shapes in the fp32 precision: gemm_tn_small_kernel (n_out, k_in <= 32; 64-row chunks), gemm_tn_narrowk_kernel (k_in <= 8,
# 32 < n_out <= 256: no counter of its own -- it counts as generic; 128-row chunks), and gemm_tn_generic_kernel for [40 x 18]
@pytest.mark.parametrize("n_out,k_in,path,chunk,counter", [
    (18, 18, "tn_small", 64, "gemm_tn_small"), (18, 6, "tn_small", 64, "gemm_tn_small"), (72, 6, "tn_narrowk", 128, "gemm_tn_generic"),
    (32, 32, "tn_small", 64, "gemm_tn_small"), (16, 5, "tn_small", 64, "gemm_tn_small"), (40, 18, "tn_generic", 128, "gemm_tn_generic")])
def test_small_shapes_fp32(n_out, k_in, path, chunk, counter):
    for rows in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129):
        for dz, hi in (("perm", None), (None, "gather"), ("gather", "perm")):
            for fam in ("exact", "normal"):
                c = Case(n_out, k_in, rows, nbatch=2, family=fam, dz_idx=dz, h_idx=hi, off=1, seed=rows)
                single(c, "fp32", ch(path, 0, 1, 1, chunk, -(-rows // chunk), red_ny=1), counts(**{counter: 1}), (n_out, k_in, rows, dz, hi, fam),
                       label="fp32 " + path if rows == 129 and dz == "gather" else None)


@pytest.mark.parametrize("prec", ["fp32_split", "bf16"])
def test_gathered_mfma_shape_falls_back(prec):
    """a gathered product at an MFMA shape is no job of the row-panel kernel: counted, and correct on the fp32 any-shape kernel"""
    for dz, hi in (("perm", None), (None, "gather")):
        for fam in ("exact", "normal"):
            c = Case(64, 64, 300, family=fam, dz_idx=dz, h_idx=hi, seed=5)
            chosen, got = run([c], prec)
            assert chosen[0] == [ch("tn_generic", 0, 1, 1, 128, 3, red_ny=1), NONE] and got == counts(wgrad_panel_fallback=1, gemm_tn_generic=1)
            c.verify(("fallback", dz, hi, fam), "fp32", label="fallback")     # (the fp32 kernel rounds nothing)


def test_gathered_bf16_rows_are_refused():
    c = Case(64, 64, 300, family="exact", src16=True, dz_idx="perm")
    chosen, got = run([c], "bf16", rc=-4)
    assert chosen[0] == [NONE, NONE] and got == counts(wgrad_panel_fallback=1)
    assert b"not covered by the row-panel kernel" in capi.load().mpnhip_last_error()
    assert c.untouched()


# ------------------------------------------------------------------------------------ the fp32 path's extras
@pytest.mark.parametrize("n_out,k_in,tbn,to,tc,xcd", [(320, 64, 64, 5, 1, 1), (192, 64, 64, 3, 1, 0), (576, 64, 64, 9, 1, 0),
                                                      (128, 224, 128, 2, 2, 1), (68, 132, 128, 2, 2, 1)])
def test_fp32_mfma_kernel(n_out, k_in, tbn, to, tc, xcd):
    """gemm_tn_kernel<64> / <128>: the XCD-aware block mapping on (4 .. 8 tiles) and off; rows around TBK = 32 (two groups with ranges on every fp32 kernel: test_row_ranges)"""
    for rows in (1, 31, 32, 33, 127, 128, 129, 300):
        for fam in ("exact", "normal"):
            c = Case(n_out, k_in, rows, nbatch=2, family=fam, seed=rows)
            single(c, "fp32", ch("tn_mfma", tbn, to, tc, 128, -(-rows // 128), xcd_map=xcd, red_ny=1), counts(gemm_tn_mfma=1),
                   (n_out, k_in, rows, fam), label="fp32 mfma" if rows == 300 else None)


def test_fp32_two_stage_slab_sum():
    """2,816 rows x 3 batches in 128-row chunks: 66 slabs >= 64 and 34 column blocks < 512 -> eight partial sums first"""
    for fam in ("exact", "normal"):
        c = Case(64, 64, 2816, nbatch=3, family=fam)
        single(c, "fp32", ch("tn_mfma", 64, 1, 1, 128, 22, red_ny=8), counts(gemm_tn_mfma=1), ("two-stage", fam), label="fp32 two-stage")
        groups = ((0, 1409), (1409, 2816))
        c = Case(64, 64, 2816, nbatch=3, family=fam, groups=groups)
        single(c, "fp32", ch("tn_mfma", 64, 1, 1, 128, 22, red_ny=8), counts(gemm_tn_mfma=1), ("two-stage, two groups", fam))


# ------------------------------------------------------------------------------------ many jobs in one launch
def step_group(d, N, E, nb, family):
    """the products BackwardRun::mp_weight_grads (csrc/backward.hip) records for one group of nb steps of the d-wide model in the split form, widths
    from synth.model_params: node update, flow layers 1 and 0 (two direction groups), classifier output layer and layer 0, edge
    layers 1 and 0 (the e0 share hoisted), per-node projections (the x0 share hoisted; no bias)"""
    p = synth.model_params(d, 2)
    enc = p["encoder_feats_dict"]
    dn, de = enc["node_out_dim"], enc["edge_out_dim"]
    he, hn, hcw = p["edge_model_feats_dict"]["dims"][0], p["node_model_feats_dict"]["dims"][0], p["classifier_feats_dict"]["edge_dims"][0]
    assert p["edge_model_feats_dict"]["dims"][1] == de and p["node_model_feats_dict"]["dims"][1] == dn
    pw, kx = 2 * he + 2 * hn, 2 * dn
    dirs = ((0, E * 3 // 7), (E * 3 // 7, E))
    k = dict(nbatch=nb, family=family)
    return [Case(dn, 2 * dn, N, seed=1, **k),
            Case(dn, hn, E, groups=dirs, seed=2, **k),
            Case(hn, de, E, groups=dirs, ldw_pad=kx + GC, seed=3, **k),
            Case(1, hcw, E, dz_idx="perm", seed=4, **k),
            Case(hcw, de, E, seed=5, **k),
            Case(de, he, E, seed=6, **k),
            Case(he, de, E, ldw_pad=2 * kx + de + GC, seed=7, **k),
            Case(pw, dn, N, ldw_pad=dn + GC, bias=False, seed=8, **k)]


def check_batch(cases, prec, expect, cnt, name, alone=True, label=None, **kw):
    """all cases in one launch; then (alone) each job against the same product run as a batch of its own with the same batched flag"""
    chosen, got = run(cases, prec, one_launch=True, **kw)
    want = [[e, e if len(c.groups) == 2 else NONE] for c, e in zip(cases, expect)]
    assert chosen == want, (name, [(i, a, b) for i, (a, b) in enumerate(zip(chosen, want)) if a != b])
    assert got == cnt, (name, got, cnt)
    snaps = []
    for i, c in enumerate(cases):
        c.verify((name, i), prec, label if i == len(cases) - 2 else None)
        snaps.append(c.snapshot())
    return chosen, snaps


@pytest.mark.parametrize("prec", ["fp32_split", "bf16"])
def test_batch_of_the_32d_model(prec):
    """(a) ten jobs, every MFMA job re-tiled to <1,1>: [16 x 80] / [80 x 16] from one <2,2> tile to two, [272 x 32] from one <5,1> tile
    to five (12 % more operand columns over the launch: under the 15 % bound); batched plan: 192 / (nb x tiles) chunks wanted,
    never below 256 rows"""
    N, E, nb = 200, 1000, 2
    expect = [ch("panel", 3, 1, 1, 256, 1, 1), ch("panel", 3, 1, 1, 256, 4, 1), ch("panel", 3, 1, 1, 256, 4, 1), ch("panel", 6, 1, 1, 256, 4, 1),
              ch("panel", 7, 1, 1, 256, 4, 1), ch("panel", 3, 1, 2, 256, 4, 1), ch("panel", 3, 2, 1, 256, 4, 1), ch("panel", 3, 5, 1, 256, 1, 1)]
    for fam in ("exact", "normal"):
        cases = step_group(32, N, E, nb, fam)
        _, snaps = check_batch(cases, prec, expect, panel_counts(1, jobs=10), ("32-d", prec, fam), batched=True, label="batch 32-d " + prec)
        # alone, with the same chunk plan: bitwise the same wherever the launch did not re-tile the job (jobs 5 .. 7 were)
        for i, c in enumerate(cases):
            run([c], prec, batched=True)
            same = all(torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])) for a, b in zip(snaps[i], c.snapshot()))
            if i < 5:
                assert same, ("32-d", prec, fam, i, "differs from the product run alone")


@pytest.mark.parametrize("prec", ["fp32_split", "bf16"])
def test_batch_of_the_128d_model(prec):
    """(b) [128 x 256] and [128 x 224]: two <2,2> tiles; [1088 x 128]: nine <2,2> tiles; not narrow.  Chunks: 192 / (2 x tiles) wanted"""
    N, E, nb = 200, 1000, 2
    expect = [ch("panel", 5, 1, 2), ch("panel", 5, 1, 2, 256, 4), ch("panel", 2, 1, 1, 256, 4), ch("panel", 6, 1, 1, 256, 4),
              ch("panel", 3, 1, 1, 256, 4), ch("panel", 1, 1, 1, 256, 4), ch("panel", 0, 1, 1, 256, 4), ch("panel", 5, 9, 1)]
    for fam in ("exact", "normal"):
        cases = step_group(128, N, E, nb, fam)
        _, snaps = check_batch(cases, prec, expect, panel_counts(0, jobs=10), ("128-d", prec, fam), batched=True, label="batch 128-d " + prec)
        for i, c in enumerate(cases):
            run([c], prec, batched=True)
            # (no job was re-tiled.  [1 x 32] and [32 x 64] alone are narrow launches: the same block code in the four-blocks-per-CU
            # instantiation -- bitwise equal as well)
            for a, b in zip(snaps[i], c.snapshot()):
                assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), ("128-d", prec, fam, i)


def test_batch_longest_first():
    """(c) recorded in ascending block length (chunk rows x staged columns per row): the flush reverses them; two jobs of equal
    weight keep their order.  [64 x 64] rides in a launch that is not narrow: wp_block<1,1> of the wide kernel"""
    shapes = [(64, 64, 3), (64, 64, 3), (224, 64, 2), (320, 64, 0), (64, 320, 1)]
    for prec in ("fp32_split", "bf16"):
        for fam in ("exact", "normal"):
            cases = [Case(n, k, 700, nbatch=2, family=fam, seed=i + 1) for i, (n, k, _) in enumerate(shapes)]
            expect = [ch("panel", v, 1, 1, 256, 3) for _, _, v in shapes]
            _, snaps = check_batch(cases, prec, expect, panel_counts(0, jobs=5), ("longest first", prec, fam), batched=True,
                                   label="batch order " + prec)
            for i, c in enumerate(cases):
                run([c], prec, batched=True)
                # ([64 x 64] alone is a narrow launch: the same <1,1> block in the other instantiation -- bitwise equal as well)
                for a, b in zip(snaps[i], c.snapshot()):
                    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), ("order", prec, fam, i)


def test_batch_of_rows16_and_row_panel_jobs():
    """(d) bf16 rows: two jobs of the LDS-DMA kernel and three of the row-panel kernel in one batch -- one launch of each"""
    shapes = [(640, 128, "rows16", 16, 1), (64, 128, "panel", 12, 1), (256, 448, "rows16", 19, 2), (224, 64, "panel", 10, 1),
              (1, 32, "panel", 6, 1)]
    for fam in ("exact", "normal"):
        cases = [Case(n, k, 700, nbatch=2, family=fam, src16=True, seed=i + 1) for i, (n, k, _, _, _) in enumerate(shapes)]
        expect = [ch(path, v, 1, tc, 256, 3) for _, _, path, v, tc in shapes]
        check_batch(cases, "bf16", expect, counts(gemm_tn_panel=5, wgrad_panel_launches=1, wgrad_rows16=2, wgrad_rows16_launches=1),
                    ("rows16 + panel", fam), batched=True, label="batch rows16")


def test_batch_rolls_when_the_job_table_is_full():
    """(e) nine two-group products: the ninth does not fit the 16-job table -- the batch is flushed and goes on empty"""
    rows = 601
    for prec in ("fp32_split", "bf16"):
        for fam in ("exact", "normal"):
            cases = [Case(64, 64, rows, family=fam, groups=((0, 100 + 37 * i), (100 + 37 * i, rows)), seed=i + 1) for i in range(9)]
            expect = [ch("panel", 3, 1, 1, 256, 3, narrow=1, rolled=int(i == 8)) for i in range(9)]
            check_batch(cases, prec, expect, counts(gemm_tn_panel=18, wgrad_panel_launches=2, wgrad_panel_narrow_launches=2),
                        ("rolled: table", prec, fam), batched=True, label="batch rolled")


def test_batch_rolls_when_the_slab_is_full():
    """(f) a slab region one job too small: the same outcome through the slab-space branch"""
    rows = 601
    cases = [Case(64, 64, rows, family="exact", seed=i + 1) for i in range(4)]
    arr = (capi.WgradProduct * 1)(cases[0].c)
    # one job's share of the batch region: the workspace of one product less the part that does not depend on the batch
    lib = capi.load()
    one = (lib.mpnhip_debug_weight_grad_batch_workspace_bytes(arr, 1, capi.PRECISIONS["fp32_split"], 1, 0) -
           lib.mpnhip_debug_weight_grad_batch_workspace_bytes(arr, 1, capi.PRECISIONS["fp32"], 1, 0)) // 4
    assert one == 3 * 64 * 68 == 13056      # nsplit x n_out x (k_in + 4) floats
    for fam in ("exact", "normal"):
        cases = [Case(64, 64, rows, family=fam, seed=i + 1) for i in range(4)]
        expect = [ch("panel", 3, 1, 1, 256, 3, narrow=1, rolled=int(i == 3)) for i in range(4)]
        check_batch(cases, "fp32_split", expect, counts(gemm_tn_panel=4, wgrad_panel_launches=2, wgrad_panel_narrow_launches=2),
                    ("rolled: slab", fam), batched=True, slab=3 * one)


@pytest.mark.parametrize("n_out,k_in,variant", [(320, 128, 0), (128, 224, 5)])
def test_batched_chunk_plan(n_out, k_in, variant):
    """a job that shares its launch wants 192 blocks instead of 512: at 10,000 rows x 3 batches x 2 tiles that is 192 / 6 = 32 chunks of
    ceil(10000 / 32) = 313 -> 320 rows against 512 / 6 = 85 chunks wanted, i.e. the 256-row minimum and 40 chunks"""
    for prec in ("fp32_split", "bf16"):
        for fam in ("exact", "normal"):
            c = Case(n_out, k_in, 10000, nbatch=3, family=fam)
            single(c, prec, ch("panel", variant, 1, 2, 320, 32), panel_counts(0), (n_out, k_in, prec, fam, "batched"), batched=True,
                   label="batched plan " + prec)
            single(c, prec, ch("panel", variant, 1, 2, 256, 40), panel_counts(0), (n_out, k_in, prec, fam, "alone"))


# ------------------------------------------------------------------------------------ run to run
@pytest.mark.parametrize("name", ["panel", "panel bf16", "rows16", "fp32", "fp32 two-stage", "small", "batch"])
def test_bitwise_reproducible(name):
    if name == "batch":
        cases, kw, prec = step_group(32, 200, 1000, 2, "normal"), dict(one_launch=True, batched=True), "fp32_split"
    else:
        kw = {}
        prec = {"panel": "fp32_split", "panel bf16": "bf16", "rows16": "bf16", "small": "fp32_split"}.get(name, "fp32")
        shape = {"rows16": (448, 128), "small": (18, 18), "fp32 two-stage": (64, 64)}.get(name, (320, 64))
        rows = 2816 if name == "fp32 two-stage" else 1500
        groups = ((0, 700), (700, rows)) if name != "fp32 two-stage" else (None,)
        cases = [Case(shape[0], shape[1], rows, nbatch=3, family="normal", src16=name == "rows16", groups=groups)]
    outs = []
    for _ in range(3):
        run(cases, prec, **kw)
        outs.append([c.snapshot() for c in cases])
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            for (aw, ab), (bw, bb) in zip(a, b):
                assert torch.equal(bits(aw), bits(bw)) and torch.equal(bits(ab), bits(bb)), name
