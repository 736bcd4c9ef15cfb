"""Numpy restatement of the segmented reductions of csrc/segment.hip and of their gradient (test infrastructure only): a strictly
sequential reduction over CSR segments in float32 (the order of torch_scatter's CPU kernels, which the short-segment kernels
document) and the same in float64, the torch_scatter backward, and the index structures mpnhip_graph_prep builds.
tests/test_segment_ref_cpu.py pins it to the reference's own scatter outputs (tests/golden/g5_modules.npz) and to torch autograd;
tests/test_gpu_segment.py uses it as the expectation for every kernel variant.  Also the two input families of those tests."""
import numpy as np

from mpntrackseg_amd import synth

AGGS = ("sum", "mean", "max")


def seg_reduce(src, ptr, nseg, agg="sum", list=None, runs=1, run_stride=0, out=None, ldo=None, nmod=None, off0=0, off1=0,
               accumulate=False, argmax=None, dtype=np.float32):
    """Segment s < nseg reduces the rows src[list[j] if list is given else j], j in [ptr[s], ptr[s + 1]) -- with runs > 1 (sum
    only, no list) the union of the runs [ptr[s + r * run_stride], ptr[s + r * run_stride + 1]), r < runs, in that order -- one
    row after the other in ``dtype``, and writes out[s % nmod, (off0 if s // nmod == 0 else off1) + 0 .. dim) (added to what is
    there with ``accumulate``).  mean divides the sum by max(count, 1) in ``dtype``; max starts from -inf, takes a row only when
    it is strictly larger (the FIRST maximum wins), gives 0 and arg-max -1 for an empty segment; arg-max names the source row.
    ``out`` / ``argmax``: [rows, ldo] arrays to write into, created ([nmod, max(off0, off1) + dim], zeros / -1) when None.
    Returns (out, argmax)."""
    src = np.asarray(src)
    dim = int(src.shape[1])
    ptr = np.asarray(ptr, np.int64)
    nmod = int(nmod) if nmod is not None else max(int(nseg), 1)
    assert agg in AGGS and (runs <= 1 or (agg == "sum" and list is None))
    if out is None:
        width = int(ldo) if ldo is not None else max(off0, off1) + dim
        out = np.zeros((nmod, width), dtype)
    if argmax is None:
        argmax = np.full(out.shape, -1, np.int64)
    s_t = src.astype(dtype)
    for s in range(int(nseg)):
        acc = np.full(dim, -np.inf if agg == "max" else 0.0, dtype)
        arg = np.full(dim, -1, np.int64)
        count = 0
        for r in range(max(int(runs), 1)):
            b, e = int(ptr[s + r * run_stride]), int(ptr[s + r * run_stride + 1])
            if r == 0:
                count = e - b
            for j in range(b, e):
                i = int(list[j]) if list is not None else j
                v = s_t[i]
                if agg == "max":
                    take = v > acc
                    acc = np.where(take, v, acc)
                    arg = np.where(take, i, arg)
                else:
                    acc = acc + v
        if agg == "mean":
            acc = acc / dtype(max(count, 1))
        elif agg == "max" and count == 0:
            acc = np.zeros(dim, dtype)
        c0 = off0 if s // nmod == 0 else off1
        o = out[s % nmod, c0:c0 + dim]
        out[s % nmod, c0:c0 + dim] = (o + acc) if accumulate else acc
        argmax[s % nmod, c0:c0 + dim] = arg
    return out, argmax


def seg_reduce_seq(src, ptr, nseg, agg="sum", **kw):
    """float32, strictly sequential: every partial sum is rounded to float32."""
    return seg_reduce(src, ptr, nseg, agg, dtype=np.float32, **kw)


def seg_reduce_f64(src, ptr, nseg, agg="sum", **kw):
    return seg_reduce(src, ptr, nseg, agg, dtype=np.float64, **kw)


def rows_to_csr(row, x_size):
    """(list, ptr [x_size + 1], keys) of mpnhip_segment_reduce: a stable sort of the row indices, rows outside [0, x_size) parked
    behind the last segment (key x_size), where no segment reads them."""
    row = np.asarray(row, np.int64)
    keys = np.where((row < 0) | (row >= x_size), x_size, row)
    lst = np.argsort(keys, kind="stable")
    ptr = np.searchsorted(keys[lst], np.arange(x_size + 1), side="left")
    return lst.astype(np.int64), ptr.astype(np.int64), keys


def seg_reduce_grad(grad_out, row, agg, src=None, argmax=None):
    """The torch_scatter backward of out = scatter_<agg>(src, row, dim_size = x_size) in float64: sum broadcasts grad_out[row[j]]
    to row j, mean divides it by the segment's count, max gives it only to the row the forward picked (``argmax`` [x_size, dim]
    as the forward returned it, or worked out from ``src`` by the first-maximum rule) -- ties are NOT split.  Rows outside
    [0, x_size) took no part in the forward: zero gradient."""
    g = np.asarray(grad_out, np.float64)
    x_size, dim = g.shape
    row = np.asarray(row, np.int64)
    ok = (row >= 0) & (row < x_size)
    safe = np.where(ok, row, 0)
    out = g[safe] if x_size else np.zeros((row.size, dim))
    if agg == "mean":
        count = np.bincount(row[ok], minlength=x_size)
        out = out / np.maximum(count, 1)[safe][:, None]
    elif agg == "max":
        if argmax is None:
            lst, ptr, _ = rows_to_csr(row, x_size)
            _, argmax = seg_reduce_f64(src, ptr, x_size, "max", list=lst)
        out = np.where(np.asarray(argmax)[safe] == np.arange(row.size)[:, None], out, 0.0)
    else:
        assert agg == "sum"
    return np.where(ok[:, None], out, 0.0)


def directions(ei):
    """0: row < col (flow_out), 1: row > col (flow_in), 2: self loop (in neither aggregate)."""
    return np.where(ei[0] < ei[1], 0, np.where(ei[0] > ei[1], 1, 2))


def _order(keys, nkeys):
    perm = np.argsort(keys, kind="stable")
    return perm.astype(np.int64), np.searchsorted(keys[perm], np.arange(nkeys + 1), side="left").astype(np.int64)


def graph_csr(edge_index, N):
    """The structures mpnhip_graph_prep leaves in the graph buffer (csrc/graph_prep.hip), as int64 arrays:
    perm [E] sorted position -> edge id, the stable sort by dir * N + row; srow / scol [E] the end points in sorted order;
    seg_ptr [3N + 1] CSR over the keys dir * N + row; cperm [E] sorted positions re-sorted stably by dir * N + col, with
    cseg_ptr [3N + 1]; rperm / rseg_ptr [N + 1] sorted positions by row alone (all directions); cperm_all / cseg_all by col."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    d = directions(ei)
    perm, seg_ptr = _order(d * N + ei[0], 3 * N)
    srow, scol, sd = ei[0][perm], ei[1][perm], d[perm]
    cperm, cseg_ptr = _order(sd * N + scol, 3 * N)
    rperm, rseg_ptr = _order(srow, N)
    cperm_all, cseg_all = _order(scol, N)
    return dict(perm=perm, srow=srow, scol=scol, seg_ptr=seg_ptr, cperm=cperm, cseg_ptr=cseg_ptr, rperm=rperm, rseg_ptr=rseg_ptr,
                cperm_all=cperm_all, cseg_all=cseg_all)


# ------------------------------------------------------------------------------------ bf16
def bf16_bits(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


# ------------------------------------------------------------------------------------ input families
def exact_values(seed, shape, stream=0, relu=False):
    """k / 4 with integer |k| <= 32 (float32): any sum of up to 2^12 of them is a multiple of 1/4 below 2^15, so every partial
    sum in any order is exact in float32, and each value is exact in bf16.  ``relu``: max(., 0) -- half the entries tie at 0."""
    n = int(np.prod(shape)) if len(shape) else 1
    k = np.floor(synth.uniform01(seed, n, stream) * 65.0) - 32.0
    v = (k / 4.0).astype(np.float32).reshape(shape)
    return np.maximum(v, np.float32(0)) if relu else v


def normal_values(seed, shape, stream=0, relu=False):
    v = synth.normal(seed, shape, stream=stream)
    return np.maximum(v, np.float32(0)) if relu else v


FAMILIES = {"exact": exact_values, "normal": normal_values}
