"""Operator-level parity of the fused dense GEMM (csrc/gemm.hip: gemm_kernel in its fp32 / bf16 / three-piece split forms and both B
layouts, gemm_generic_kernel, gemm_smallk_kernel, and the split-K path k_gemm_splitk + k_splitk_sum / k_splitk_sum_l2) against ONE
float64 CPU reference of the documented formula (``reference`` below), called through the C ABI (mpnhip_debug_gemm,
mpnhip_debug_linear_splitk).

Every output buffer has guard rows and guard columns (ldc > N) and is prefilled with NaN -- with finite random values where
``accumulate`` reads the old contents.  Everything the reference does not write (guards, rows of [0, m_upper) that belong to no
group, rows of a taller C that c_idx does not name) is asserted bit-for-bit untouched; elements whose mask is <= 0 are asserted to be
exactly 0.  Input paddings hold NaN as well, so a load from the wrong K segment or past a row's end shows.

Error measure (as in the other operator tests): max |got - ref64| / max(max |ref64|, 1e-30) over all written elements.  Tolerances:
fp32 2e-6 (what test_gpu_parity.py::test_linear_matches_torch holds up to K = 2048); bf16 operands 2e-5 of max(1, max |ref|) against
the float64 product of the SAME bf16-rounded operands (tests/test_gpu_gemm_bf16.py); fp32_split max(2e-6, 4 x the error of the
float32 CPU evaluation of the same reference on the same case) -- the 4 x covers the summation order, as in
tests/test_gpu_attention.py.  Every case prints the kernel's error and the float32 CPU evaluation's error (DESIGN.md section 2 keeps
the table of an MI355X run).

Every case asserts, from the literals in its parametrisation, which kernel ran (the ``chosen`` report of mpnhip_debug_gemm: kernel,
WM, WN, TN, operand form) and the gemm_fp32 / gemm_split / gemm_bf16 / gemm_splitk counters."""
import ctypes as C

import numpy as np
import pytest
import torch

from mpntrackseg_amd import capi, synth

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
FP32, BF16, SPLIT = 0, 1, 2          # MPNHIP_PREC_*
KCONTIG, NCONTIG = 0, 1              # MPNHIP_GEMM_B_*
MFMA, GENERIC, SMALLK = 0, 1, 2      # chosen: kernel
GR, GC = 3, 8                        # guard rows above and below / guard columns right of every output
TOL_FP32, TOL_BF16 = 2e-6, 2e-5
# what a launch of each kernel adds to the (gemm_fp32, gemm_split, gemm_bf16) counters: the MFMA kernel counts its operand form, the
# generic and the small-K kernel have no counter
COUNTS = {(MFMA, FP32): (1, 0, 0), (MFMA, SPLIT): (0, 1, 0), (MFMA, BF16): (0, 0, 1), (GENERIC, FP32): (0, 0, 0),
          (GENERIC, BF16): (0, 0, 0), (SMALLK, FP32): (0, 0, 0), (SMALLK, BF16): (0, 0, 0)}


def reference(Cm, rows, A, A2, ksplit, a_idx, B, bias, G1, g1_idx, G2, g2_idx, relu, accumulate, mask, c_idx, dtype=torch.float64,
              bf16=False):
    """The documented formula of one row group, evaluated in ``dtype`` on the CPU.  Cm [rows of C, N] (dtype) is updated in place for
    the rows m of ``rows`` (int64); A [*, >= ksplit], A2 [*, K - ksplit] or None, B [K, N] (the mathematical matrix, whatever its
    layout in memory); every index is an int tensor or None (identity); bf16: the operands are rounded to bfloat16 first."""
    m = rows
    ai = a_idx[m].long() if a_idx is not None else m
    a = A[ai][:, :ksplit]                                                  # 1. sum_k A[a_idx[m]] B, columns >= ksplit from A2
    if A2 is not None:
        a = torch.cat([a, A2[ai]], 1)
    b = B
    if bf16:
        a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    v = a.to(dtype) @ b.to(dtype)
    if bias is not None:                                                   # 2. + bias + G1[g1_idx[m]] + G2[g2_idx[m]]
        v = v + bias.to(dtype)
    if G1 is not None:
        v = v + G1[g1_idx[m].long() if g1_idx is not None else m].to(dtype)
    if G2 is not None:
        v = v + G2[g2_idx[m].long() if g2_idx is not None else m].to(dtype)
    if relu:                                                               # 3. ReLU
        v = v.relu()
    ci = c_idx[m].long() if c_idx is not None else m
    if accumulate:                                                         # 4. + old C
        v = v + Cm[ci]
    if mask is not None:                                                   # 5. mask[m] > 0 ? value : 0
        v = torch.where(mask[m] > 0, v, torch.zeros_like(v))
    Cm[ci] = v                                                             # 6. store to row c_idx[m]
    return Cm


def err(got, ref, floor=1e-30):
    if ref.numel() == 0:
        return 0.0
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), floor)


def bits(t):
    return t.contiguous().view(torch.int32)


def normal(seed, shape, stream, std=1.0):
    return torch.from_numpy(synth.normal(seed, shape, stream=stream, std=std))


def index(seed, n, hi, stream):
    """n int32 indices in [0, hi): duplicates occur on their own when n > hi"""
    return torch.from_numpy((synth.uniform01(seed, n, stream=stream) * hi).astype(np.int32))


def padded(t, ld, off=0):
    """Device copy of the CPU matrix t [r, c] with leading dimension ld >= c, NaN in the padding, its first element `off` floats
    behind a 16-byte aligned address.  Returns (tensor that owns the memory, address of element [0, 0])."""
    r, c = t.shape
    assert ld >= c
    buf = torch.full((off + max(r, 1) * ld,), float("nan"), dtype=torch.float32)
    buf[off:off + r * ld].view(r, ld)[:, :c] = t
    buf = buf.to(dev())
    return buf, buf.data_ptr() + 4 * off


def iptr(t):
    return None if t is None else t.data_ptr()


class Problem:
    """One product: the logical operands on the CPU, their padded images on the device, and the float64 / float32 references."""

    def __init__(self, groups, m_upper, N, K, prec=FP32, bl=KCONTIG, ksplit=None, a_idx=False, g1=None, g2=None, mask=False,
                 accumulate=False, c_idx=False, relu=1, bias=True, small_tiles=0, device_rows=True, a_off=0, lda_pad=4, seed=1):
        self.groups, self.R, self.N, self.K, self.prec = groups, m_upper, N, K, prec
        assert all(0 <= b <= e <= m_upper for b, e in groups) and 1 <= len(groups) <= 2
        ksplit = K if ksplit is None else ksplit
        R = m_upper
        self.keep = keep = []
        a = self.args = capi.DebugGemmArgs()
        a.ngroups, a.N, a.K, a.ksplit, a.relu, a.accumulate, a.m_upper = len(groups), N, K, ksplit, relu, int(accumulate), m_upper
        a.small_tiles, a.b_layout, a.precision = small_tiles, bl, prec
        # A (and A2) are shared by the groups; a_idx gathers from a shorter table, so source rows repeat
        RA = max(2, R // 3 + 1) if a_idx else max(R, 1)
        self.a_idx = index(seed, R, RA, 11) if a_idx else None
        Afull = normal(seed, (RA, K), 1)
        self.A, self.A2 = Afull[:, :ksplit].contiguous(), (Afull[:, ksplit:].contiguous() if ksplit < K else None)
        hA, pA = padded(self.A, ksplit + lda_pad, a_off)
        hA2, pA2 = padded(self.A2, K - ksplit + 8) if self.A2 is not None else (None, None)
        # mask: negative, zero and positive values
        self.mask = None
        if mask:
            self.mask = normal(seed, (R, N), 6)
            self.mask.view(-1)[::5] = 0.0
            self.mask.view(-1)[3::7] *= -0.0
        hM, pM = padded(self.mask, N + 4) if mask else (None, None)
        # G2 by identity (one row per output row), shared
        self.G2 = normal(seed, (R, N), 7) if g2 else None
        self.g2_idx = index(seed, R, R, 12) if g2 == "idx" else None
        hG2, pG2 = padded(self.G2, N + 4) if g2 else (None, None)
        # C: shared; c_idx is a permutation into a taller C
        self.RC = R + (11 if c_idx else 0)
        self.c_idx = None
        if c_idx:
            self.c_idx = torch.from_numpy(np.argsort(synth.uniform01(seed, self.RC, stream=13))[:R].astype(np.int32))
        self.ldc = N + GC
        old = normal(seed, (self.RC + 2 * GR, self.ldc), 8) if accumulate else torch.full((self.RC + 2 * GR, self.ldc), float("nan"))
        self.old = old.to(dev())
        self.Cd = self.old.clone()
        pC = self.Cd.data_ptr() + 4 * GR * self.ldc
        dev_idx = {k: (v.to(dev()) if v is not None else None) for k, v in (("a", self.a_idx), ("g2", self.g2_idx), ("c", self.c_idx))}
        # row ranges: a device int32[4] (b0, e0, b1, e1), or m_static for one group that starts at row 0
        rows_d = torch.tensor([x for g in groups for x in g], dtype=torch.int32, device=dev())
        keep += [hA, hA2, hM, hG2, dev_idx, rows_d]
        self.B, self.bias, self.G1, self.g1_idx = [], [], [], []
        for i, (b, e) in enumerate(groups):
            W = normal(seed, (K, N), 20 + i, std=(2.0 / max(K, 1)) ** 0.5)      # B as the mathematical [K, N] matrix
            bv = normal(seed, (N,), 30 + i, std=0.1) if bias else None
            T = 37 if g1 == "idx" else R
            G1 = normal(seed, (T, N), 40 + i) if g1 else None
            g1i = index(seed, R, T, 50 + i) if g1 == "idx" else None
            self.B.append(W); self.bias.append(bv); self.G1.append(G1); self.g1_idx.append(g1i)
            hB, pB = padded(W.t().contiguous(), K + 4) if bl == KCONTIG else padded(W, N + 4)
            hb = bv.to(dev()) if bias else None
            hG1, pG1 = padded(G1, N + 4) if g1 else (None, None)
            hg1i = g1i.to(dev()) if g1i is not None else None
            keep += [hB, hb, hG1, hg1i]
            g = a.g[i]
            g.A, g.A2, g.a_idx, g.B, g.bias = pA, pA2, iptr(dev_idx["a"]), pB, iptr(hb)
            g.G1, g.g1_idx, g.G2, g.g2_idx, g.mask = pG1, iptr(hg1i), pG2, iptr(dev_idx["g2"]), pM
            g.C, g.c_idx = pC, iptr(dev_idx["c"])
            g.lda, g.lda2, g.ldb = ksplit + lda_pad, K - ksplit + 8, (K + 4 if bl == KCONTIG else N + 4)
            g.ldg1, g.ldg2, g.ldmask, g.ldc = N + 4, N + 4, N + 4, self.ldc
            if device_rows:
                g.row_begin, g.row_end = rows_d.data_ptr() + 8 * i, rows_d.data_ptr() + 8 * i + 4
            else:
                assert b == 0 and len(groups) == 1
                g.m_static = e
        # the references: float64, and the same function in float32
        self.written = torch.zeros((self.RC + 2 * GR, self.ldc), dtype=torch.bool)
        self.ref, self.ref32 = (self.evaluate(dt) for dt in (torch.float64, torch.float32))

    def evaluate(self, dtype):
        Cm = self.old.cpu()[GR:GR + self.RC, :self.N].to(dtype)
        for i, (b, e) in enumerate(self.groups):
            rows = torch.arange(b, e)
            reference(Cm, rows, self.A, self.A2, self.args.ksplit, self.a_idx, self.B[i], self.bias[i], self.G1[i], self.g1_idx[i], self.G2,
                      self.g2_idx, self.args.relu, self.args.accumulate, self.mask, self.c_idx, dtype=dtype, bf16=self.prec == BF16)
            ci = self.c_idx[rows].long() if self.c_idx is not None else rows
            self.written[GR + ci, :self.N] = True
        return Cm

    def run(self):
        """-> (C as the kernel left it, guards included, on the CPU; chosen = (kernel, WM, WN, TN, form); the three counters)"""
        self.Cd.copy_(self.old)
        chosen = (C.c_int32 * 4)(9, 9, 9, 9)
        capi.path_counters(reset=True)
        capi.check(capi.load().mpnhip_debug_gemm(C.byref(self.args), chosen, capi.stream_ptr()), "mpnhip_debug_gemm")
        torch.cuda.synchronize()
        cnt = capi.path_counters(reset=True)
        assert cnt["gemm_splitk"] == 0 and cnt["gemm_bf16_tiled"] == 0, cnt
        ch = (chosen[0] & 255, chosen[1], chosen[2], chosen[3], chosen[0] >> 8) if chosen[0] >= 0 else tuple(chosen)
        return self.Cd.cpu(), ch, (cnt["gemm_fp32"], cnt["gemm_split"], cnt["gemm_bf16"])

    def check(self, name, expect, family):
        """expect: the literal (kernel, WM, WN, TN, operand form) of the case.  Returns the kernel's output buffer."""
        got, chosen, counts = self.run()
        assert chosen == tuple(expect), (name, chosen, expect)
        assert counts == COUNTS[(expect[0], expect[4])], (name, counts)
        w = self.written
        # bit-for-bit untouched outside what the reference writes: guard rows and columns, rows of no group, unnamed rows of C
        assert torch.equal(bits(got)[~w], bits(self.old.cpu())[~w]), (name, "wrote outside its rows / columns")
        inner, wi = got[GR:GR + self.RC, :self.N], w[GR:GR + self.RC, :self.N]
        g, r64, r32 = inner[wi], self.ref[wi], self.ref32[wi]
        assert torch.isfinite(g).all(), (name, "non-finite output")
        if self.mask is not None:
            for b, e in self.groups:
                rows = torch.arange(b, e)
                ci = self.c_idx[rows].long() if self.c_idx is not None else rows
                off = self.mask[rows] <= 0
                assert e == b or off.any(), name
                assert (bits(inner[ci][off]) == 0).all(), (name, "masked elements must be exactly 0")
        floor = 1.0 if self.prec == BF16 else 1e-30
        e_k, e_32 = err(g, r64, floor), err(r32, r64, floor)
        print("GEMM_ERR %-10s %-58s kernel %.2e  float32-cpu %.2e" % (family, name, e_k, e_32))
        tol = {FP32: TOL_FP32, BF16: TOL_BF16, SPLIT: max(TOL_FP32, 4.0 * e_32)}[expect[4]]
        assert e_k <= tol, (name, e_k, e_32, tol)
        return got


def one_group(M, N, K, expect, family, **kw):
    name = "%d x %d x %d %s" % (M, N, K, " ".join("%s=%s" % kv for kv in sorted(kw.items())))
    p = Problem([(0, M)], M, N, K, **kw)
    p.check(name, expect, family)
    return p


# ------------------------------------------------------------------------------------ strip width (128-row strips, M = 32768)
# K = 136: four full K steps and an 8-wide tail; N = 32 nt - 4.  TN by hand from launch_gemm: the cost ceil(nt / tn) tn, widest
# first, is minimal at tn = nt up to 8, at 3 for nt = 9 (9 against 16, 14, 12, 10, 12) and at 1 for nt = 11 (11 against 16, 14, 12,
# 15, 12, 12, 12); 256 row blocks: nothing is halved.
@pytest.mark.parametrize("nt,tn", [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (8, 8), (9, 3), (11, 1)])
def test_strip_width_fp32(nt, tn):
    one_group(32768, 32 * nt - 4, 136, (MFMA, 4, 1, tn, FP32), "strip")


@pytest.mark.parametrize("nt,tn", [(1, 1), (4, 4), (8, 8)])
def test_strip_width_bf16(nt, tn):
    """K < 192: the bf16 form stays on the strip kernel"""
    one_group(32768, 32 * nt - 4, 136, (MFMA, 4, 1, tn, BF16), "strip", prec=BF16)


@pytest.mark.parametrize("n,tn,form", [(256, 8, SPLIT), (284, 3, SPLIT), (348, 1, SPLIT), (252, 8, FP32), (124, 4, FP32)])
def test_strip_width_split(n, tn, form):
    """the split form from N = 256 (nt = 8 is N = 256 here: 32 * 8 - 4 = 252 is demoted to fp32, like nt = 4)"""
    one_group(32768, n, 136, (MFMA, 4, 1, tn, form), "strip", prec=SPLIT)


def test_strip_halving_rule():
    """8192 x 256: 64 row blocks x 1 strip of 8 < 256 blocks -> 4 -> 2 (64 x 4 = 256 blocks)"""
    one_group(8192, 256, 136, (MFMA, 4, 1, 2, FP32), "strip")


def test_small_tiles_flag():
    one_group(8192, 256, 136, (MFMA, 2, 2, 1, FP32), "tile", small_tiles=1)


# ------------------------------------------------------------------------------------ few rows: 2 x 2 x 1 and 4 x 1 x 1 tiles
T411, T221 = (4, 1, 1), (2, 2, 1)


@pytest.mark.parametrize("K", [4, 32, 36, 160])
@pytest.mark.parametrize("N,tile", [(4, T411), (28, T411), (36, T221), (100, T221), (320, T221)])
@pytest.mark.parametrize("M", [1, 31, 64, 65, 200])
def test_few_rows(M, N, tile, K):
    one_group(M, N, K, (MFMA,) + tile + (FP32,), "tile", device_rows=(M % 2 == 1))


@pytest.mark.parametrize("K", [4, 36, 160])
@pytest.mark.parametrize("N,tile", [(1, T411), (18, T411), (33, T221)])
@pytest.mark.parametrize("M", [1, 65, 200])
def test_scalar_epilogue_under_mfma(M, N, tile, K):
    """N % 4 != 0 with K % 4 == 0: the MFMA kernel with its scalar epilogue"""
    one_group(M, N, K, (MFMA,) + tile + (FP32,), "tile", g1="idx", mask=True, accumulate=True)


@pytest.mark.parametrize("M,N,K", [(200, 320, 160), (65, 260, 132)])
def test_few_rows_split(M, N, K):
    one_group(M, N, K, (MFMA, 2, 2, 1, SPLIT), "tile", prec=SPLIT)


# ------------------------------------------------------------------------------------ full epilogue, one group
ALL = dict(a_idx=True, g1="idx", g2="id", mask=True, accumulate=True, c_idx=True)
TERMS = [dict(a_idx=True), dict(g1="idx"), dict(g2="id"), dict(mask=True), dict(accumulate=True), dict(c_idx=True), ALL]


@pytest.mark.parametrize("prec", [FP32, BF16])
@pytest.mark.parametrize("ksplit", [0, 36, 72])
@pytest.mark.parametrize("terms", TERMS + [dict()], ids=lambda t: "+".join(t) or "plain")
def test_full_epilogue(terms, ksplit, prec):
    one_group(200, 100, 72, (MFMA, 2, 2, 1, prec), "epilogue", prec=prec, ksplit=ksplit, **terms)


@pytest.mark.parametrize("terms", TERMS, ids=lambda t: "+".join(t))
def test_full_epilogue_split(terms):
    one_group(200, 260, 132, (MFMA, 2, 2, 1, SPLIT), "epilogue", prec=SPLIT, ksplit=68, **terms)


# 8200 rows are 65 row blocks: N = 100 (nt = 4): 4 -> 2 -> 1 (65, 130 < 256 blocks); N = 260 (nt = 9): 3 -> 2 (65 x 5 = 325 blocks)
@pytest.mark.parametrize("N,K,ksplit,prec,tn", [(100, 72, 36, FP32, 1), (100, 72, 36, BF16, 1), (260, 132, 68, SPLIT, 2)])
def test_full_epilogue_on_the_strip(N, K, ksplit, prec, tn):
    one_group(8200, N, K, (MFMA, 4, 1, tn, prec), "epilogue", prec=prec, ksplit=ksplit, **ALL)


# ------------------------------------------------------------------------------------ two groups
def two_groups(r0, r1, r2, expect, family, gap=0, extra=0, N=100, K=72, **kw):
    """rows [0, r0) group 0, [r0 + gap, r0 + gap + r1) group 1, then r2 rows of neither; m_upper = all of them + extra.  Each group
    has its own B, bias and G1 table; A and C are shared; the ranges come from a device int32[4]."""
    groups = [(0, r0), (r0 + gap, r0 + gap + r1)]
    m_upper = r0 + gap + r1 + r2 + extra
    p = Problem(groups, m_upper, N, K, **{**dict(g1="idx"), **kw})
    p.check("groups %d + %d (+ %d, gap %d, extra %d) N %d K %d %s" % (r0, r1, r2, gap, extra, N, K, sorted(kw.items())), expect, family)
    return p


@pytest.mark.parametrize("r0,r1,r2", [(0, 0, 5), (0, 70, 0), (70, 0, 3), (1, 1, 0), (33, 95, 2), (128, 128, 0), (130, 61, 9)])
@pytest.mark.parametrize("prec", [FP32, BF16])
def test_two_groups_on_the_tile(r0, r1, r2, prec):
    two_groups(r0, r1, r2, (MFMA, 2, 2, 1, prec), "groups", prec=prec)
    two_groups(r0, r1, r2, (MFMA, 2, 2, 1, prec), "groups", prec=prec, **ALL)


def test_two_groups_on_the_strip():
    two_groups(4100, 4099, 7, (MFMA, 4, 1, 1, FP32), "groups", ksplit=36, **ALL)


def test_two_groups_split():
    two_groups(130, 61, 9, (MFMA, 2, 2, 1, SPLIT), "groups", N=260, K=132, ksplit=68, prec=SPLIT, **ALL)


def test_two_groups_with_a_gap():
    two_groups(40, 70, 0, (MFMA, 2, 2, 1, FP32), "groups", gap=10, mask=True, accumulate=True)
    two_groups(64, 64, 0, (MFMA, 2, 2, 1, FP32), "groups", gap=1)


def test_two_groups_m_upper_beyond_the_last_row():
    two_groups(33, 95, 0, (MFMA, 2, 2, 1, FP32), "groups", extra=372, mask=True, accumulate=True)


# ------------------------------------------------------------------------------------ B stored [K][N] (dH = dZ W)
# 8200 x 132: nt = 5, 65 row blocks: 5 -> 3 -> 2 -> 1
@pytest.mark.parametrize("M,N,K,tile", [(200, 4, 36, T411), (200, 100, 72, T221), (8200, 132, 40, T411)])
def test_b_ncontig(M, N, K, tile):
    """mask and accumulate as the backward's activation-gradient product issues it: one group, two groups, a_idx and c_idx"""
    expect = (MFMA,) + tile + (FP32,)
    one_group(M, N, K, expect, "b_ncontig", bl=NCONTIG, relu=0, bias=False)
    one_group(M, N, K, expect, "b_ncontig", bl=NCONTIG, relu=0, bias=False, mask=True, accumulate=True)
    one_group(M, N, K, expect, "b_ncontig", bl=NCONTIG, relu=0, bias=False, mask=True, accumulate=True, a_idx=True, c_idx=True)
    r0 = M // 3 + 1
    two_groups(r0, M - r0 - 3, 3, expect, "b_ncontig", N=N, K=K, bl=NCONTIG, relu=0, bias=False, mask=True, accumulate=True)


@pytest.mark.parametrize("N,tn", [(92, 3), (252, 8)])
def test_b_ncontig_on_wide_strips(N, tn):
    """32768 rows (256 row blocks: nothing halved), nt = 3 and 8; K = 40: one full K step and an 8-wide tail"""
    one_group(32768, N, 40, (MFMA, 4, 1, tn, FP32), "b_ncontig", bl=NCONTIG, relu=0, bias=False, mask=True, accumulate=True)


def test_b_ncontig_ragged_n_takes_the_generic_kernel():
    one_group(200, 18, 36, (GENERIC, 0, 0, 0, FP32), "generic", bl=NCONTIG, relu=0, bias=False, mask=True, accumulate=True)


# ------------------------------------------------------------------------------------ the generic kernel
@pytest.mark.parametrize("K", [1, 6, 37])
@pytest.mark.parametrize("prec,form", [(FP32, FP32), (BF16, BF16), (SPLIT, FP32)])
def test_generic_kernel(K, prec, form):
    expect = (GENERIC, 0, 0, 0, form)
    one_group(77, 19, K, expect, "generic", prec=prec)
    one_group(77, 20, K, expect, "generic", prec=prec, ksplit=K // 2, **ALL)
    two_groups(33, 40, 4, expect, "generic", N=20, K=K, prec=prec, ksplit=K // 2, **ALL)


@pytest.mark.parametrize("kw", [dict(a_off=1), dict(lda_pad=5), dict(lda_pad=5, bl=NCONTIG, relu=0)], ids=str)
def test_generic_kernel_misaligned_operands(kw):
    """K % 4 == 0 and N % 4 == 0, but A starts 4 bytes behind a 16-byte boundary / lda % 4 != 0: not the MFMA kernel's operands"""
    one_group(130, 36, 40, (GENERIC, 0, 0, 0, FP32), "generic", **kw)
    one_group(130, 36, 40, (GENERIC, 0, 0, 0, FP32), "generic", g1="idx", g2="idx", mask=True, accumulate=True, c_idx=True, a_idx=True, **kw)


# ------------------------------------------------------------------------------------ the small-K kernel
@pytest.mark.parametrize("N", [4, 72, 1024])
@pytest.mark.parametrize("K", [1, 6, 7])
@pytest.mark.parametrize("M", [4096, 5000])
def test_smallk_kernel(M, K, N):
    """K <= 8, N % 4 == 0, from 4096 rows; at N = 72 the 18 threads of a row do not divide the block"""
    one_group(M, N, K, (SMALLK, 0, 0, 0, FP32), "smallk")
    one_group(M, N, K, (SMALLK, 0, 0, 0, FP32), "smallk", relu=0, bias=False, device_rows=False)
    p = Problem([(37, M)], M, N, K, a_idx=True)     # a device row_begin: rows [0, 37) stay untouched
    p.check("%d x %d x %d rows from 37, a_idx" % (M, N, K), (SMALLK, 0, 0, 0, FP32), "smallk")
    one_group(M, N, K, (SMALLK, 0, 0, 0, BF16), "smallk", prec=BF16, a_idx=True)


def test_smallk_kernel_needs_4096_rows():
    one_group(4095, 72, 6, (GENERIC, 0, 0, 0, FP32), "generic")
    one_group(4096, 72, 6, (GENERIC, 0, 0, 0, FP32), "generic", mask=True)     # ... and the plain epilogue


# ------------------------------------------------------------------------------------ split-K
def splitk_case(M, N, K, name, taken=1, fused=None, n2=None, relu2=1, prec=FP32, ldx_pad=0, ldy_pad=GC, scratch_floats=None, relu=1,
                bias=True, seed=2):
    """y1 = act(x W^T + b) through mpnhip_debug_linear_splitk, optionally with the next layer y2 = act2(y1 W2^T + b2); asserts
    taken / fused / the gemm_splitk counter, both outputs against float64, guards and untaken outputs untouched."""
    lib = capi.load()
    x, W = normal(seed, (M, K), 1), normal(seed, (K, N), 2, std=(2.0 / K) ** 0.5)
    b = normal(seed, (N,), 3, std=0.1) if bias else None
    hx, px = padded(x, K + ldx_pad)
    hw, pw = padded(W.t().contiguous(), K)
    hb = b.to(dev()) if bias else None
    ldy = N + ldy_pad
    y_old = torch.full((M + 2 * GR, ldy), float("nan"), device=dev())
    y = y_old.clone()
    need = lib.mpnhip_debug_linear_splitk_scratch_floats(M, N, K)
    floats = need if scratch_floats is None else scratch_floats
    scratch = torch.full((max(need, floats, 1) + 64,), float("nan"), device=dev())
    pw2 = pb2 = py2 = None
    ldy2 = 0
    if n2:
        W2, b2 = normal(seed, (N, n2), 4, std=(2.0 / N) ** 0.5), normal(seed, (n2,), 5, std=0.1)
        hw2, pw2 = padded(W2.t().contiguous(), N)
        hb2 = b2.to(dev())
        pb2, ldy2 = hb2.data_ptr(), n2 + GC
        y2_old = torch.full((M + 2 * GR, ldy2), float("nan"), device=dev())
        y2 = y2_old.clone()
        py2 = y2.data_ptr() + 4 * GR * ldy2
    tf = (C.c_int32 * 2)(9, 9)
    capi.path_counters(reset=True)
    capi.check(lib.mpnhip_debug_linear_splitk(px, K + ldx_pad, pw, iptr(hb), y.data_ptr() + 4 * GR * ldy, ldy, M, N, K, relu, prec, pw2, pb2,
                                              n2 or 0, relu2, py2, ldy2, scratch.data_ptr(), floats, tf, capi.stream_ptr()), "splitk")
    torch.cuda.synchronize()
    cnt = capi.path_counters(reset=True)
    fused = int(bool(n2)) if fused is None else fused
    assert list(tf) == [taken, fused if taken else 0], (name, list(tf))
    assert cnt["gemm_splitk"] == taken and cnt["gemm_fp32"] + cnt["gemm_split"] + cnt["gemm_bf16"] == 0, (name, cnt)
    got = y.cpu()
    if not taken:
        assert torch.equal(bits(got), bits(y_old.cpu())) and torch.isnan(scratch).all(), (name, "launched something")
        assert not n2 or torch.equal(bits(y2.cpu()), bits(y2_old.cpu())), name
        return None
    outs = []
    z = torch.zeros((M, N), dtype=torch.float64)
    rows = torch.arange(M)
    for dt in (torch.float64, torch.float32):
        r1 = reference(z.to(dt), rows, x, None, K, None, W, b, None, None, None, None, relu, 0, None, None, dtype=dt)
        r2 = None
        if n2:
            # the kernel feeds the next layer its own fp32 y1: so does the float32 evaluation; the float64 one keeps float64
            r2 = reference(torch.zeros((M, n2), dtype=dt), rows, r1, None, N, None, W2, b2, None, None, None, None, relu2, 0, None, None, dtype=dt)
        outs.append((r1, r2))
    (r1, r2), (s1, s2) = outs
    inside = torch.zeros_like(got, dtype=torch.bool)
    inside[GR:GR + M, :N] = True
    assert torch.equal(bits(got)[~inside], bits(y_old.cpu())[~inside]), (name, "y1: wrote outside its rows / columns")
    g1 = got[GR:GR + M, :N]
    assert torch.isfinite(g1).all(), name
    e1, f1 = err(g1, r1), err(s1, r1)
    print("GEMM_ERR %-10s %-58s kernel %.2e  float32-cpu %.2e" % ("splitk", name + " y1", e1, f1))
    assert e1 <= TOL_FP32, (name, e1, f1)
    if n2:
        got2 = y2.cpu()
        if fused:
            inside2 = torch.zeros_like(got2, dtype=torch.bool)
            inside2[GR:GR + M, :n2] = True
            assert torch.equal(bits(got2)[~inside2], bits(y2_old.cpu())[~inside2]), (name, "y2: wrote outside its rows / columns")
            g2 = got2[GR:GR + M, :n2]
            assert torch.isfinite(g2).all(), name
            e2, f2 = err(g2, r2), err(s2, r2)
            print("GEMM_ERR %-10s %-58s kernel %.2e  float32-cpu %.2e" % ("splitk_l2", name + " y2", e2, f2))
            assert e2 <= TOL_FP32, (name, e2, f2)
        else:
            assert torch.equal(bits(got2), bits(y2_old.cpu())), (name, "y2 must stay untouched when the next layer is not fused")
        return torch.cat([got.view(-1), got2.view(-1)])
    return got


@pytest.mark.parametrize("K", [512, 576, 640, 704, 516, 2048])
@pytest.mark.parametrize("N", [36, 100, 128])
@pytest.mark.parametrize("M", [1, 65, 140])
def test_splitk(M, N, K):
    """K = 512 ... 704: 8, 9, 10 and 11 slices of 64 -- every tail of splitk_total; 516: a slice that ends off a 32 boundary"""
    splitk_case(M, N, K, "%d x %d x %d" % (M, N, K), ldx_pad=(8 if M == 65 else 0), relu=int(N != 100), bias=(M != 140))


@pytest.mark.parametrize("K", [512, 576, 640, 704, 2048])
@pytest.mark.parametrize("n1,n2,relu2,fused", [(128, 1, 0, 1), (128, 32, 1, 1), (128, 64, 1, 1), (128, 65, 1, 0), (260, 32, 1, 0),
                                               (100, 32, 1, 1), (36, 64, 0, 1), (256, 64, 1, 1)])
def test_splitk_next_layer(n1, n2, relu2, fused, K):
    """the summing launch evaluates the next layer when it is narrow (n2 <= 64) and n1 <= 256; n1 = 100, 36: n1 % 16 != 0"""
    for M in (1, 140):
        splitk_case(M, n1, K, "%d x %d x %d -> %d" % (M, n1, K, n2), fused=fused, n2=n2, relu2=relu2, ldy_pad=0)
    # guard columns behind y1 (ldy > n): the next layer is left to the caller
    splitk_case(65, n1, K, "%d x %d x %d -> %d ldy > n" % (65, n1, K, n2), fused=0, n2=n2, relu2=relu2)


def test_splitk_with_the_split_precision():
    splitk_case(140, 128, 2048, "140 x 128 x 2048 split", prec=SPLIT, n2=32, ldy_pad=0)


def test_splitk_refusals():
    """not a shape of this path: nothing is launched, the outputs and the scratch keep their prefill"""
    splitk_case(65, 36, 508, "k = 508", taken=0)
    splitk_case(65, 36, 512, "bf16", taken=0, prec=BF16, n2=32)
    # 65 x 36 x 512 is cut into 8 slices of 64: 8 * 65 * 36 floats of scratch are enough, one less is not
    splitk_case(65, 36, 512, "scratch one float short", taken=0, scratch_floats=8 * 65 * 36 - 1, n2=32)
    splitk_case(65, 36, 512, "scratch just enough", taken=1, scratch_floats=8 * 65 * 36)
    splitk_case(65, 36, 512, "ldx % 4 != 0", taken=0, ldx_pad=2)


# ------------------------------------------------------------------------------------ reproducibility
def test_bitwise_reproducible():
    """one case of each kernel family three times: no atomics anywhere, so the results are bitwise equal"""
    cases = [(Problem([(0, 8200)], 8200, 100, 72, ksplit=36, **ALL), (MFMA, 4, 1, 1, FP32)),
             (Problem([(0, 130), (130, 191)], 200, 100, 72, **ALL), (MFMA, 2, 2, 1, FP32)),
             (Problem([(0, 200)], 200, 100, 72, prec=BF16, **ALL), (MFMA, 2, 2, 1, BF16)),
             (Problem([(0, 200)], 200, 260, 132, prec=SPLIT, ksplit=68, **ALL), (MFMA, 2, 2, 1, SPLIT)),
             (Problem([(0, 200)], 200, 100, 72, bl=NCONTIG, mask=True, accumulate=True), (MFMA, 2, 2, 1, FP32)),
             (Problem([(0, 77)], 77, 20, 37, ksplit=18, **ALL), (GENERIC, 0, 0, 0, FP32)),
             (Problem([(0, 5000)], 5000, 72, 6, a_idx=True), (SMALLK, 0, 0, 0, FP32))]
    for i, (p, expect) in enumerate(cases):
        first = p.check("reproducibility %d" % i, expect, "repeat")
        for _ in range(2):
            again, chosen, _ = p.run()
            assert chosen == expect and torch.equal(bits(first), bits(again)), i
    for n2 in (None, 32):
        first = splitk_case(140, 128, 704, "reproducibility split-K", n2=n2, ldy_pad=0)
        for _ in range(2):
            assert torch.equal(bits(first), bits(splitk_case(140, 128, 704, "reproducibility split-K", n2=n2, ldy_pad=0)))
