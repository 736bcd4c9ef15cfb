"""Operator-level tests of the segmented reductions (csrc/segment.hip: k_segment_reduce<4> / <1>, k_aggregate,
k_segment_reduce_block, k_segment_reduce_block3, k_segment_reduce3, k_segment_reduce3_b16) and of their gather-form gradient
(csrc/bn_dropout.hip: k_segment_reduce_bwd), every call through the C ABI, against tests/segment_ref.py (pinned to the
reference's torch_scatter outputs by tests/test_segment_ref_cpu.py).

Every output is prefilled with NaN (bf16 rows and arg-max: an integer sentinel) and carries 8 guard columns that must keep the
prefill: entries that take a leading dimension are told a row of ``width`` columns inside a buffer of ``width + 8``; entries
whose output is dense by signature (mpnhip_segment_reduce, its backward, mpnhip_debug_aggregate) write between 8 guard elements
in front and 8 behind.  The path counters are reset before every call and the kernel variant that ran is asserted after it.

Two input families (segment_ref.FAMILIES).  ``exact``: multiples of 1/4 in [-8, 8] -- every partial sum is exact in float32 in
any order, so sums must equal float64 bit for bit in EVERY kernel, mean must equal float32(sum) / float32(count), the bf16 rows
the exact sum rounded to nearest even; no tolerance.  ``normal``: the short-segment kernels document the sequential order of the
reference's CPU scatter and must equal the float32 sequential reference bit for bit; the block-per-segment kernels sum in a
fixed tree and are held to 4 x the largest error the float32 sequential reference shows against float64 on the same inputs
(computed here; a tree sum has the smaller error bound, so the factor leaves room for the order only: a lost or doubled row is
an error of the size of an input).  Max and arg-max are exact everywhere; every entry is called twice, bitwise equal."""
import ctypes as C

import numpy as np
import pytest
import torch

import segment_ref as R
from mpntrackseg_amd import capi, modular, synth

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
PAD = 8
ARG_SENTINEL = -77
B16_SENTINEL = 0x7FC1   # a bf16 NaN no rounding produces
SEG_COUNTERS = ("aggregate", "aggregate_block", "segment_reduce", "segment_reduce_block", "segment_reduce_block3", "segment_reduce3")
AGG = capi.AGG_CODE
# one empty segment in front, one behind, the lengths around the 8-rows-in-flight unroll, one long segment
SEG_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000, 0]


def to_dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev())


def expect_counters(counts, **want):
    got = {k: counts[k] for k in SEG_COUNTERS}
    assert got == {k: want.get(k, 0) for k in SEG_COUNTERS}, got


class Dense:
    """A dense [rows, cols] output between two guards of PAD elements (16-byte alignment is kept: PAD * 4 = 32 bytes)."""

    def __init__(self, rows, cols, dtype=torch.float32):
        self.n = rows * cols
        fill = float("nan") if dtype == torch.float32 else ARG_SENTINEL
        self.flat = torch.full((self.n + 2 * PAD,), fill, dtype=dtype, device=dev())
        self.shape, self.fill = (rows, cols), fill

    def ptr(self):
        return C.c_void_p(self.flat.data_ptr() + PAD * self.flat.element_size())

    def get(self):
        h = self.flat.cpu().numpy()
        g = np.concatenate([h[:PAD], h[PAD + self.n:]])
        assert (np.isnan(g).all() if self.fill != ARG_SENTINEL else (g == ARG_SENTINEL).all()), "guard elements overwritten"
        return h[PAD:PAD + self.n].reshape(self.shape).copy()


def max_abs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) if np.size(a) else 0.0


def check_values(name, family, agg, tree, got, seq32, ref64):
    """The comparison rules of the module docstring for one output tensor; returns (kernel error, float32 reference error)."""
    assert np.isfinite(got).all(), (name, "non-finite output")
    e_k, e_r = max_abs(got, ref64), max_abs(seq32, ref64)
    if agg == "max":
        assert np.array_equal(got, ref64.astype(np.float32)), name
    elif family == "exact":
        if agg == "sum":
            assert np.array_equal(got.astype(np.float64), ref64), name
        else:
            assert np.array_equal(got, seq32), name   # seq32 = float32(exact sum) / float32(count) here
    elif not tree:
        assert np.array_equal(got, seq32), (name, e_k, e_r)
    else:
        print("SEG_ERR %-44s %-4s kernel %.3e  float32-sequential %.3e" % (name, agg, e_k, e_r))
        assert e_r > 0 and e_k <= 4.0 * e_r, (name, e_k, e_r)
    return e_k, e_r


# ------------------------------------------------------------------------------------ mpnhip_segment_reduce
def segment_rows():
    """row [m] int64 in a scrambled order: segment s has SEG_LENGTHS[s] rows; five rows each of -1, x_size and x_size + 5 are
    mixed in.  Returns (row, x_size, the out-of-range mask)."""
    x_size = len(SEG_LENGTHS)
    row = np.concatenate([np.full(n, s, np.int64) for s, n in enumerate(SEG_LENGTHS)] + [np.full(5, v, np.int64) for v in (-1, x_size, x_size + 5)])
    row = row[np.argsort(synth.uniform01(31, row.size, stream=7), kind="stable")]
    return row, x_size, (row < 0) | (row >= x_size)


def call_segment_reduce(src_ptr, row_d, m, dim, x_size, agg, want_arg):
    lib = capi.load()
    out = Dense(x_size, dim)
    arg = Dense(x_size, dim, torch.int32) if want_arg else None
    nb = lib.mpnhip_segment_reduce_workspace_bytes(m, x_size)
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=dev())
    capi.path_counters(reset=True)
    capi.check(lib.mpnhip_segment_reduce(src_ptr, capi.ptr(row_d), m, dim, x_size, AGG[agg], out.ptr(), arg.ptr() if arg else None,
                                         capi.ptr(ws), ws.numel(), capi.stream_ptr()), "mpnhip_segment_reduce")
    torch.cuda.synchronize()
    return out.get(), (arg.get() if arg else None), capi.path_counters(reset=True)


SEGMENT_DIMS = [(1, 0), (3, 0), (7, 0), (4, 0), (8, 0), (32, 0), (80, 0), (128, 0), (224, 0), (256, 0), (260, 0), (320, 0), (640, 0),
                (1024, 0), (256, 1)]


@pytest.mark.parametrize("dim,shift", SEGMENT_DIMS)
def test_segment_reduce(dim, shift):
    """k_segment_reduce<4> (dim % 4 == 0: sub / nblk geometries 1 ... 64 lanes, 20 of 32 and 56 of 64 lanes live, two passes of
    the column loop at 260, column blocks at 320 / 640 / 1024) and <1> (dim 1, 3, 7; dim 256 on a source shifted by one float:
    the scalar path with nblk = 4) over segments of every length around the unroll, rows outside [0, x_size) mixed in."""
    row, x_size, parked = segment_rows()
    m = row.size
    lst, ptr, _ = R.rows_to_csr(row, x_size)
    row_d = to_dev(row)
    for family in R.FAMILIES:
        src = R.FAMILIES[family](40 + dim, (m, dim), stream=1, relu=True)
        src[parked] = 8.0    # would win every max and move every sum
        flat = torch.zeros(m * dim + 4, dtype=torch.float32, device=dev())
        flat[shift:shift + m * dim] = to_dev(src).reshape(-1)
        src_ptr = C.c_void_p(flat.data_ptr() + 4 * shift)
        for agg in R.AGGS:
            name = "segment_reduce dim %d shift %d %s" % (dim, shift, family)
            seq, arg_ref = R.seg_reduce_seq(src, ptr, x_size, agg, list=lst)
            r64, _ = R.seg_reduce_f64(src, ptr, x_size, agg, list=lst)
            if family == "exact" and agg == "mean":
                s64, _ = R.seg_reduce_f64(src, ptr, x_size, "sum", list=lst)
                seq = s64.astype(np.float32) / np.maximum(np.diff(ptr), 1).astype(np.float32)[:, None]
            out, arg, counts = call_segment_reduce(src_ptr, row_d, m, dim, x_size, agg, agg == "max")
            expect_counters(counts, segment_reduce=1)
            check_values(name, family, agg, False, out, seq, r64)
            assert not out[0].any() and not out[-1].any(), name          # the empty segments
            if agg == "max":
                assert np.array_equal(arg, arg_ref), name
                assert (arg[0] == -1).all() and (arg[-1] == -1).all() and not np.isin(arg, np.flatnonzero(parked)).any(), name
            out2, arg2, _ = call_segment_reduce(src_ptr, row_d, m, dim, x_size, agg, agg == "max")
            assert np.array_equal(out, out2) and (arg is None or np.array_equal(arg, arg2)), name


@pytest.mark.parametrize("agg", R.AGGS)
def test_segment_reduce_without_rows(agg):
    """m = 0: zeros, arg-max -1, no kernel."""
    out, arg, counts = call_segment_reduce(None, None, 0, 12, 5, agg, agg == "max")
    expect_counters(counts)
    assert out.shape == (5, 12) and not out.any() and not np.signbit(out).any()
    assert arg is None or (arg == -1).all()


# ------------------------------------------------------------------------------------ graphs
def sparse_graph(N=64):
    """E ~ 700: node 5 isolated (no edge names it), node 30 only past edges (row > col), node 20 only future edges, three self
    loops, node 40 a hub of 200 edges; the rest uniformly random with duplicates."""
    u = lambda n, s: synth.uniform01(77 + N, n, stream=s)
    row, col = (u(520, 0) * N).astype(np.int64), (u(520, 1) * N).astype(np.int64)
    keep = (row != 5) & (col != 5) & (row != col) & ~((row == 30) & (col > 30)) & ~((row == 20) & (col < 20)) & (row != 40)
    row, col = row[keep], col[keep]
    hub = (u(200, 2) * N).astype(np.int64)
    hub[(hub == 5) | (hub == 40)] = 41
    extra = np.array([[7, 7, 22, 30, 20], [7, 7, 22, 3, 50]], np.int64)
    ei = np.concatenate([np.stack([row, col]), np.stack([np.full(200, 40, np.int64), hub]), extra], axis=1)
    ei = ei[:, np.argsort(u(ei.shape[1], 3), kind="stable")]
    d = R.directions(ei)
    assert not (ei == 5).any() and (d[ei[0] == 30] == 1).all() and (d[ei[0] == 20] == 0).all() and int((d == 2).sum()) == 3
    assert int((ei[0] == 40).sum()) == 200 and 600 <= ei.shape[1] < 48 * N
    return ei


def dense_graph(N=24, E=None):
    """E edges (default 100 N) over N nodes: node 3 is nobody's row, node 10 has one edge per direction, everything else random."""
    E = 100 * N if E is None else E
    u = lambda n, s: synth.uniform01(91, n, stream=s)
    allowed = np.array([n for n in range(N) if n not in (3, 10)], np.int64)
    row = allowed[(u(E - 2, 0) * allowed.size).astype(np.int64)]
    col = (u(E - 2, 1) * N).astype(np.int64)
    ei = np.concatenate([np.stack([row, col]), np.array([[10, 10], [2, 15]], np.int64)], axis=1)
    ei = ei[:, np.argsort(u(E, 2), kind="stable")]
    assert ei.shape[1] == E and not (ei[0] == 3).any() and int((ei[0] == 10).sum()) == 2 and (R.directions(ei) == 2).any()
    return ei


_graphs = {}


def graph(kind, N, E=None):
    """(edge_index, segment_ref.graph_csr, {name: int32 device array}, PreparedGraph): built once per shape, never modified."""
    key = (kind, N, E)
    if key not in _graphs:
        ei = sparse_graph(N) if kind == "sparse" else dense_graph(N, E)
        csr = R.graph_csr(ei, N)
        pg = capi.PreparedGraph(to_dev(ei), N, validate=True, full=True)
        # the primary order of the device's own graph preparation is the helper's (tests/test_gpu_parity.py::test_graph_prep_order)
        perm = pg.buf.cpu().numpy()[256:256 + 4 * ei.shape[1]].view(np.int32)
        assert np.array_equal(perm, csr["perm"])
        _graphs[key] = (ei, csr, {k: to_dev(v, np.int32) for k, v in csr.items()}, pg)
    return _graphs[key]


# ------------------------------------------------------------------------------------ mpnhip_debug_aggregate
def run_aggregate(pg, src_d, dim, agg):
    lib = capi.load()
    out = Dense(pg.N, 2 * dim)
    arg = Dense(pg.N, 2 * dim, torch.int32) if agg == "max" else None
    capi.path_counters(reset=True)
    capi.check(lib.mpnhip_debug_aggregate(capi.ptr(pg.buf), pg.N, pg.E, capi.ptr(src_d), dim, AGG[agg], out.ptr(),
                                          arg.ptr() if arg else None, capi.stream_ptr()), "mpnhip_debug_aggregate")
    torch.cuda.synchronize()
    return out.get(), (arg.get() if arg else None), capi.path_counters(reset=True)


AGGREGATE_CASES = [("sparse", 64, None, d, "aggregate") for d in (4, 32, 128, 256, 260)] + [("sparse", 64, None, 6, "segment_reduce")] + \
                  [("dense", 24, 2400, d, "aggregate_block") for d in (4, 32, 80, 256)] + [("dense", 24, 96 * 24 - 1, 32, "aggregate")]


@pytest.mark.parametrize("kind,N,E,dim,path", AGGREGATE_CASES)
def test_aggregate(kind, N, E, dim, path):
    """mpnhip_debug_aggregate: k_aggregate (1 ... 64 lanes, two passes of its column loop at 260), the scalar short-segment
    fallback (dim 6), k_segment_reduce_block with 1, 8, 32 and 64 column lanes (E >= 96 N), and the last E below that threshold."""
    ei, csr, _, pg = graph(kind, N, E)
    E = ei.shape[1]
    tree = path == "aggregate_block"
    want = {path: 1, "segment_reduce_block": 1} if tree else {path: 1}
    kw = dict(nmod=N, off0=dim, off1=0)          # keys [0, N): row < col = flow_out, the right half
    d = R.directions(ei)[csr["perm"]]
    for family in R.FAMILIES:
        src = R.FAMILIES[family](60 + dim, (E, dim), stream=2, relu=True)      # rows in sorted edge order
        src_d = to_dev(src)
        for agg in R.AGGS:
            name = "aggregate %s E %d dim %d %s" % (kind, E, dim, family)
            seq, arg_ref = R.seg_reduce_seq(src, csr["seg_ptr"], 2 * N, agg, **kw)
            r64, _ = R.seg_reduce_f64(src, csr["seg_ptr"], 2 * N, agg, **kw)
            if family == "exact" and agg == "mean":
                s64, _ = R.seg_reduce_f64(src, csr["seg_ptr"], 2 * N, "sum", **kw)
                cnt = np.maximum(np.diff(csr["seg_ptr"][:2 * N + 1]), 1).astype(np.float32)
                seq = s64.astype(np.float32) / np.concatenate([np.repeat(cnt[N:, None], dim, 1), np.repeat(cnt[:N, None], dim, 1)], axis=1)
            out, arg, counts = run_aggregate(pg, src_d, dim, agg)
            expect_counters(counts, **want)
            check_values(name, family, agg, tree, out, seq, r64)
            if agg == "sum" and family == "exact":   # the layout, without the CSR helper: [flow_in | flow_out] by masks
                for half, k in ((0, 1), (1, 0)):
                    ref = np.zeros((N, dim))
                    np.add.at(ref, csr["srow"][d == k], src[d == k].astype(np.float64))
                    assert np.array_equal(out[:, half * dim:(half + 1) * dim], ref), name
            if agg == "max":
                assert np.array_equal(arg, arg_ref), name
                assert arg.max() < int(csr["seg_ptr"][2 * N]), name      # never a self loop's row
            out2, arg2, _ = run_aggregate(pg, src_d, dim, agg)
            assert np.array_equal(out, out2) and (arg is None or np.array_equal(arg, arg2)), name


# ------------------------------------------------------------------------------------ mpnhip_debug_segment_reduce3
def short_threads(nseg, dim):
    """Threads seg_short_geometry gives the float4 path of the short-segment kernel for ``nseg`` segments of ``dim`` columns."""
    per = dim // 4
    sub = 1
    while sub < per and sub < 64:
        sub <<= 1
    nblk = 1
    if per > sub or per & (per - 1):
        p2 = min(per & -per, 64)
        if p2 * 16 >= 256:
            sub, nblk = p2, per // p2
    return nseg * sub * nblk


def three_jobs(csr_d, N, he, hn, zf, z1, dP, ld, by_row_list, out16=None):
    """The three reductions of a backward step as csrc/backward.hip lays them out over dP [N, 2 he + 2 hn]: by column per direction
    (2N segments of the flow gradients, to columns 2 he and 2 he + hn), by row (the edge gradients, columns 0 .. he: the three runs
    of a node in the (dir, row) CSR, or the by-row list), by column over all directions (columns he .. 2 he)."""
    jobs = (capi.SegJob * 3)()
    esz = zf.element_size()
    specs = [(zf, hn, csr_d["cperm"], csr_d["cseg_ptr"], 2 * N, 2 * he, 2 * he + hn, 0, 0),
             (z1, he, csr_d["rperm"], csr_d["rseg_ptr"], N, 0, 0, 0, 0) if by_row_list else (z1, he, None, csr_d["seg_ptr"], N, 0, 0, 3, N),
             (z1, he, csr_d["cperm_all"], csr_d["cseg_all"], N, he, he, 0, 0)]
    for j, (src, dim, lst, ptr, nseg, off0, off1, runs, stride) in zip(jobs, specs):
        assert src.shape[1] == dim and esz in (2, 4)
        j.src, j.lds, j.list, j.ptr, j.nseg, j.dim = src.data_ptr(), dim, (lst.data_ptr() if lst is not None else None), ptr.data_ptr(), nseg, dim
        j.out, j.ldo, j.nmod, j.off0, j.off1, j.runs, j.run_stride = dP.data_ptr(), ld, N, off0, off1, runs, stride
        j.out16, j.ldo16 = (out16.data_ptr() if out16 is not None else None), ld
    return jobs


def three_refs(csr, N, he, hn, zf, z1, by_row_list, fn):
    pw = 2 * he + 2 * hn
    out = np.full((N, pw), np.nan, np.float32 if fn is R.seg_reduce_seq else np.float64)
    fn(zf, csr["cseg_ptr"], 2 * N, list=csr["cperm"], out=out, nmod=N, off0=2 * he, off1=2 * he + hn)
    if by_row_list:
        fn(z1, csr["rseg_ptr"], N, list=csr["rperm"], out=out, nmod=N)
    else:
        fn(z1, csr["seg_ptr"], N, runs=3, run_stride=N, out=out, nmod=N)
    fn(z1, csr["cseg_all"], N, list=csr["cperm_all"], out=out, nmod=N, off0=he, off1=he)
    assert not np.isnan(out).any()   # the three jobs cover every column once
    return out


def expected_dispatch(N, E, he, hn, by_row_list):
    """What segment_reduce_csr2_x3 launches: a job can take the block-per-segment kernel when its width is a multiple of 4 up to
    256 columns, it is no runs-form job, and the graph has at least 48 rows per segment of it."""
    vec = he % 4 == 0 and hn % 4 == 0
    blk = [vec and dim <= 256 and E >= 48 * nseg and ok for dim, nseg, ok in ((hn, 2 * N, True), (he, N, by_row_list), (he, N, True))]
    if all(blk):
        return dict(segment_reduce_block3=1), [True] * 3
    if not any(blk) and vec:
        return dict(segment_reduce3=1), [False] * 3
    want = {}
    if sum(blk):
        want["segment_reduce_block"] = sum(blk)
    if sum(blk) < 3:
        want["segment_reduce"] = 3 - sum(blk)
    return want, blk


WIDTHS = [(80, 56), (160, 112), (320, 224), (640, 448)]     # (he, hn) of the 32 / 64 / 128 / 256-d models
REDUCE3_CASES = [("sparse", 61, None, he, hn) for he, hn in WIDTHS] + [("dense", 24, 2400, he, hn) for he, hn in WIDTHS] + \
                [("dense", 24, 1500, he, hn) for he, hn in WIDTHS] + [("sparse", 61, None, 81, 57)]


def column_tree(he, hn, blk):
    """Per column of dP: was it written by the block-per-segment kernel?"""
    return np.concatenate([np.full(he, blk[1]), np.full(he, blk[2]), np.full(2 * hn, blk[0])])


@pytest.mark.parametrize("kind,N,E,he,hn", REDUCE3_CASES)
def test_segment_reduce3(kind, N, E, he, hn):
    """fp32 rows.  Sparse graph (N = 61: no job's thread count is a multiple of 256, so both block boundaries b0 / b1 of
    k_segment_reduce3 fall inside a job's last block; the by-row job in its runs = 3 form): one launch of k_segment_reduce3.  Dense
    graph, E >= 96 N, by-row list form: one launch of k_segment_reduce_block3 where every width fits the block kernel (<= 256
    columns: the 32-d and 64-d models); at he = 320 only the flow job does, at 640 / 448 none does and k_segment_reduce3 runs.
    48 N <= E < 96 N: three launches, short-segment for the 2N direction segments, block for the two by-node jobs.
    (he, hn) = (81, 57): three launches of the scalar short-segment kernel, the runs form among them."""
    ei, csr, csr_d, _ = graph(kind, N, E)
    E = ei.shape[1]
    by_row_list = E >= 48 * N
    pw, ld = 2 * he + 2 * hn, 2 * he + 2 * hn + PAD
    want, blk = expected_dispatch(N, E, he, hn, by_row_list)
    if kind == "sparse":
        assert want == (dict(segment_reduce3=1) if he % 4 == 0 else dict(segment_reduce=3))
        if he % 4 == 0:
            assert all(short_threads(n, d) % 256 for n, d in ((2 * N, hn), (N, he)))
    elif E >= 96 * N and he <= 256:
        assert want == dict(segment_reduce_block3=1)
    elif E < 96 * N and he <= 256:
        assert want == dict(segment_reduce=1, segment_reduce_block=2)
    tree = column_tree(he, hn, blk)
    lib = capi.load()
    for family in R.FAMILIES:
        name = "reduce3 %s E %d (%d, %d) %s" % (kind, E, he, hn, family)
        zf, z1 = R.FAMILIES[family](he, (E, hn), stream=3), R.FAMILIES[family](he, (E, he), stream=4)
        zf_d, z1_d = to_dev(zf), to_dev(z1)
        seq = three_refs(csr, N, he, hn, zf, z1, by_row_list, R.seg_reduce_seq)
        r64 = three_refs(csr, N, he, hn, zf, z1, by_row_list, R.seg_reduce_f64)
        outs = []
        for _ in range(2):
            dP = torch.full((N, ld), float("nan"), dtype=torch.float32, device=dev())
            jobs = three_jobs(csr_d, N, he, hn, zf_d, z1_d, dP, ld, by_row_list)
            capi.path_counters(reset=True)
            capi.check(lib.mpnhip_debug_segment_reduce3(jobs, E, 0, capi.stream_ptr()), "mpnhip_debug_segment_reduce3")
            torch.cuda.synchronize()
            expect_counters(capi.path_counters(reset=True), **want)
            outs.append(dP.cpu().numpy())
        got = outs[0]
        assert np.isnan(got[:, pw:]).all() and np.array_equal(got[:, :pw], outs[1][:, :pw]), name
        got = got[:, :pw]
        if tree.any():
            check_values(name + " tree", family, "sum", True, got[:, tree], seq[:, tree], r64[:, tree])
        if not tree.all():
            check_values(name, family, "sum", False, got[:, ~tree], seq[:, ~tree], r64[:, ~tree])


@pytest.mark.parametrize("he,hn", WIDTHS)
def test_segment_reduce3_bf16_rows(he, hn):
    """k_segment_reduce3_b16: bf16 source rows, fp32 sums in sequential order, and the same sums as bf16 rows (nearest even) when
    out16 is given; with out16 = NULL the fp32 sums are the same and nothing else is written."""
    N = 61
    ei, csr, csr_d, _ = graph("sparse", N)
    E = ei.shape[1]
    pw, ld = 2 * he + 2 * hn, 2 * he + 2 * hn + PAD
    lib = capi.load()
    for family in R.FAMILIES:
        name = "reduce3 bf16 (%d, %d) %s" % (he, hn, family)
        zf16, z116 = R.bf16_bits(R.FAMILIES[family](he, (E, hn), stream=5)), R.bf16_bits(R.FAMILIES[family](he, (E, he), stream=6))
        zf, z1 = R.bf16_value(zf16), R.bf16_value(z116)
        zf_d, z1_d = to_dev(zf16.view(np.int16)), to_dev(z116.view(np.int16))
        seq = three_refs(csr, N, he, hn, zf, z1, False, R.seg_reduce_seq)
        r64 = three_refs(csr, N, he, hn, zf, z1, False, R.seg_reduce_f64)
        outs = []
        for with16 in (True, False, True):
            dP = torch.full((N, ld), float("nan"), dtype=torch.float32, device=dev())
            dP16 = torch.full((N, ld), B16_SENTINEL, dtype=torch.int16, device=dev())
            jobs = three_jobs(csr_d, N, he, hn, zf_d, z1_d, dP, ld, False, dP16 if with16 else None)
            capi.path_counters(reset=True)
            capi.check(lib.mpnhip_debug_segment_reduce3(jobs, E, 1, capi.stream_ptr()), "mpnhip_debug_segment_reduce3 (bf16 rows)")
            torch.cuda.synchronize()
            expect_counters(capi.path_counters(reset=True), segment_reduce3=1)
            got, got16 = dP.cpu().numpy(), dP16.cpu().numpy().view(np.uint16)
            assert np.isnan(got[:, pw:]).all() and (got16[:, pw:] == B16_SENTINEL).all(), name
            check_values(name, family, "sum", False, got[:, :pw], seq, r64)
            if with16:
                exact = r64.astype(np.float32) if family == "exact" else seq
                assert np.array_equal(got16[:, :pw], R.bf16_bits(exact)), name
            else:
                assert (got16 == B16_SENTINEL).all(), name
            outs.append((got[:, :pw], got16))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][0], outs[2][0]) and np.array_equal(outs[0][1], outs[2][1])


def test_segment_reduce3_bf16_rows_refuses_misaligned_width():
    """he = 82: rows of 82 bf16 values cannot be read four at a time; the alignment check refuses, nothing is launched."""
    N, he, hn = 61, 82, 56
    ei, csr, csr_d, _ = graph("sparse", N)
    E = ei.shape[1]
    ld = 2 * he + 2 * hn + PAD
    zf_d, z1_d = torch.zeros((E, hn), dtype=torch.int16, device=dev()), torch.zeros((E, he), dtype=torch.int16, device=dev())
    dP = torch.full((N, ld), float("nan"), dtype=torch.float32, device=dev())
    dP16 = torch.full((N, ld), B16_SENTINEL, dtype=torch.int16, device=dev())
    jobs = three_jobs(csr_d, N, he, hn, zf_d, z1_d, dP, ld, False, dP16)
    capi.path_counters(reset=True)
    assert capi.load().mpnhip_debug_segment_reduce3(jobs, E, 1, capi.stream_ptr()) == -1
    assert b"alignment" in capi.load().mpnhip_last_error()
    torch.cuda.synchronize()
    expect_counters(capi.path_counters(reset=True))
    assert torch.isnan(dP).all() and (dP16 == B16_SENTINEL).all()


# ------------------------------------------------------------------------------------ mpnhip_segment_reduce_backward
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("dim", [1, 7, 32, 260])
def test_segment_reduce_backward(dim):
    """k_segment_reduce_bwd after the forward that made its arg-max: post-ReLU sources (ties at 0 in every long segment), signed
    gradients, rows outside [0, x_size) (zero gradient, nothing read for them).  Sum and max exact, mean within 1 ulp."""
    lib = capi.load()
    row, x_size, parked = segment_rows()
    m = row.size
    row_d = to_dev(row)
    count = np.bincount(row[~parked], minlength=x_size)
    count_d = to_dev(count, np.int32)
    for family in R.FAMILIES:
        src = R.FAMILIES[family](70 + dim, (m, dim), stream=1, relu=True)
        src[parked] = 8.0
        g = R.FAMILIES[family](70 + dim, (x_size, dim), stream=2)
        src_d, g_d = to_dev(src), to_dev(g)
        for agg in R.AGGS:
            name = "backward dim %d %s %s" % (dim, family, agg)
            arg_d = None
            if agg == "max":
                out, arg, counts = call_segment_reduce(capi.ptr(src_d), row_d, m, dim, x_size, "max", True)
                expect_counters(counts, segment_reduce=1)
                lst, ptr, _ = R.rows_to_csr(row, x_size)
                assert np.array_equal(arg, R.seg_reduce_seq(src, ptr, x_size, "max", list=lst)[1]), name
                arg_d = to_dev(arg, np.int32)
            ref = R.seg_reduce_grad(g, row, agg, src=src)
            outs = []
            for _ in range(2):
                ds = Dense(m, dim)
                capi.path_counters(reset=True)
                capi.check(lib.mpnhip_segment_reduce_backward(capi.ptr(g_d), capi.ptr(row_d), capi.ptr(arg_d),
                                                              capi.ptr(count_d) if agg == "mean" else None, m, dim, x_size, AGG[agg],
                                                              ds.ptr(), capi.stream_ptr()), "mpnhip_segment_reduce_backward")
                torch.cuda.synchronize()
                expect_counters(capi.path_counters(reset=True))        # the gather kernel is none of the reductions
                outs.append(ds.get())
            got = outs[0]
            assert np.array_equal(got, outs[1]) and np.isfinite(got).all(), name
            assert not got[parked].any(), name
            if agg == "mean":
                assert (np.abs(got - ref) <= ulp32(ref)).all(), (name, max_abs(got, ref))
            else:
                assert np.array_equal(got.astype(np.float64), ref), name
    # m = 0: nothing to write, no pointer needed
    assert lib.mpnhip_segment_reduce_backward(None, None, None, None, 0, dim, x_size, AGG["sum"], None, capi.stream_ptr()) == 0


# ------------------------------------------------------------------------------------ autograd glue
@pytest.mark.parametrize("agg", R.AGGS)
def test_autograd_segment_reduce(agg):
    """modular.segment_reduce on one 64-node case: value and every element of the gradient against the float64 reference."""
    N, m, dim = 64, 700, 24
    row = (synth.uniform01(12, m, stream=0) * N).astype(np.int64)
    row[row == 9] = 10
    lst, ptr, _ = R.rows_to_csr(row, N)
    for family in R.FAMILIES:
        src = R.FAMILIES[family](13, (m, dim), stream=1, relu=True)
        w = R.FAMILIES[family](13, (N, dim), stream=2)
        x = to_dev(src).requires_grad_(True)
        capi.path_counters(reset=True)
        out = modular.segment_reduce(x, to_dev(row), N, AGG[agg])
        (out * to_dev(w)).sum().backward()
        torch.cuda.synchronize()
        expect_counters(capi.path_counters(reset=True), segment_reduce=1)
        seq, _ = R.seg_reduce_seq(src, ptr, N, agg, list=lst)
        if family == "exact" and agg == "mean":
            seq = R.seg_reduce_f64(src, ptr, N, "sum", list=lst)[0].astype(np.float32) / np.maximum(np.diff(ptr), 1).astype(np.float32)[:, None]
        check_values("autograd " + family, family, agg, False, out.detach().cpu().numpy(), seq, R.seg_reduce_f64(src, ptr, N, agg, list=lst)[0])
        ref, got = R.seg_reduce_grad(w, row, agg, src=src), x.grad.cpu().numpy()
        assert got.shape == ref.shape
        if agg == "mean":
            assert (np.abs(got - ref) <= ulp32(ref)).all()
        else:
            assert np.array_equal(got.astype(np.float64), ref)


def test_autograd_gather_rows():
    """modular.gather_rows (_GatherRows): x[idx], and its gradient -- the segment sum of the upstream rows over idx in ascending
    row order (k_segment_reduce behind mpnhip_segment_reduce), node 9 gathered by nobody."""
    N, m, dim = 64, 700, 24
    idx = (synth.uniform01(14, m, stream=0) * N).astype(np.int64)
    idx[idx == 9] = 10
    lst, ptr, _ = R.rows_to_csr(idx, N)
    for family in R.FAMILIES:
        xv = R.FAMILIES[family](15, (N, dim), stream=1)
        w = R.FAMILIES[family](15, (m, dim), stream=2)
        x = to_dev(xv).requires_grad_(True)
        capi.path_counters(reset=True)
        y = modular.gather_rows(x, to_dev(idx))
        (y * to_dev(w)).sum().backward()
        torch.cuda.synchronize()
        expect_counters(capi.path_counters(reset=True), segment_reduce=1)
        assert np.array_equal(y.detach().cpu().numpy(), xv[idx])
        got = x.grad.cpu().numpy()
        check_values("gather_rows " + family, family, "sum", False, got, R.seg_reduce_seq(w, ptr, N, list=lst)[0], R.seg_reduce_f64(w, ptr, N, list=lst)[0])
        assert not got[9].any()
