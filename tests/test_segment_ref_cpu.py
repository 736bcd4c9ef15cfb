"""tests/segment_ref.py (the expectation of tests/test_gpu_segment.py) pinned without a GPU: to the reference's own torch_scatter
outputs (tests/golden/g5_modules.npz), to torch autograd, to brute-force masks, and to itself across precisions."""
import numpy as np
import pytest
import torch

import segment_ref as R


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


@pytest.mark.parametrize("agg", R.AGGS)
def test_sequential_reference_reproduces_the_reference_scatter(golden, agg):
    z = golden("g5_modules.npz")
    lst, ptr, _ = R.rows_to_csr(z["edge_index"][0], 40)
    out, _ = R.seg_reduce_seq(z["msg"], ptr, 40, agg, list=lst)
    assert out.dtype == np.float32 and out.shape == z[f"agg_{agg}"].shape
    if agg == "max":
        assert np.array_equal(out, z["agg_max"])
    else:
        assert rel_err(out, z[f"agg_{agg}"]) < 1e-6


@pytest.mark.parametrize("agg", R.AGGS)
def test_float64_and_float32_agree_on_exact_inputs(agg):
    m, dim, x_size = 3000, 5, 7
    src = R.exact_values(3, (m, dim), stream=1, relu=(agg == "max"))
    row = (R.synth.uniform01(3, m, stream=2) * (x_size + 2)).astype(np.int64) - 1      # -1 and x_size: parked
    row[row == 3] = 4                                                                  # an empty segment
    lst, ptr, keys = R.rows_to_csr(row, x_size)
    assert ptr[-1] == int((keys < x_size).sum()) < m and ptr[3] == ptr[4]
    o32, a32 = R.seg_reduce_seq(src, ptr, x_size, agg, list=lst)
    o64, a64 = R.seg_reduce_f64(src, ptr, x_size, agg, list=lst)
    assert np.array_equal(a32, a64)
    if agg == "mean":   # the sums are exact; the quotient is rounded once
        s64, _ = R.seg_reduce_f64(src, ptr, x_size, "sum", list=lst)
        assert np.array_equal(o32, s64.astype(np.float32) / np.maximum(np.diff(ptr), 1).astype(np.float32)[:, None])
        assert rel_err(o32, o64) < 1e-7
    else:
        assert np.array_equal(o32.astype(np.float64), o64)
    assert not o32[3].any() and (a32[3] == -1).all()
    # the bf16 rows of such sums: every input is its own bf16 value
    assert np.array_equal(R.bf16_value(R.bf16_bits(src)), src)
    assert np.array_equal(R.bf16_bits(np.array([1.0, 1.00390625, 1.01171875, -2.5], np.float32)),
                          np.array([0x3F80, 0x3F80, 0x3F82, 0xC020], np.uint16))   # ties to even, both ways


def test_placement_runs_and_accumulate():
    N, dim = 5, 3
    ei = np.array([[0, 1, 1, 3, 3, 3, 4, 2, 4], [1, 0, 2, 1, 4, 3, 0, 2, 3]])
    g = R.graph_csr(ei, N)
    z = R.exact_values(5, (ei.shape[1], dim))
    # by row: the three runs of a node in the (dir, row) CSR cover the same rows as the by-row list
    a, _ = R.seg_reduce_f64(z, g["seg_ptr"], N, runs=3, run_stride=N)
    b, _ = R.seg_reduce_f64(z, g["rseg_ptr"], N, list=g["rperm"])
    ref = np.zeros((N, dim))
    np.add.at(ref, g["srow"], z.astype(np.float64))
    assert np.array_equal(a, ref) and np.array_equal(b, ref)
    # 2N segments placed side by side, then accumulated once more
    out = np.full((N, 2 * dim + 2), 100.0)
    R.seg_reduce_f64(z, g["cseg_ptr"], 2 * N, list=g["cperm"], out=out, nmod=N, off0=1, off1=1 + dim, accumulate=True)
    d = R.directions(ei)[g["perm"]]
    for k in (0, 1):
        ref = np.zeros((N, dim))
        np.add.at(ref, g["scol"][d == k], z[d == k].astype(np.float64))
        assert np.array_equal(out[:, 1 + k * dim:1 + (k + 1) * dim], 100.0 + ref)
    assert (out[:, 0] == 100.0).all() and (out[:, -1] == 100.0).all()


def test_graph_csr_against_masks():
    N, E = 23, 400
    ei = np.stack([(R.synth.uniform01(8, E, stream=0) * N).astype(np.int64), (R.synth.uniform01(8, E, stream=1) * N).astype(np.int64)])
    g = R.graph_csr(ei, N)
    d = R.directions(ei)
    assert (d == 2).any()
    assert np.array_equal(g["perm"], np.argsort(d * N + ei[0], kind="stable"))
    sd = d[g["perm"]]
    for n in range(N):
        for k in range(3):
            seg = np.arange(g["seg_ptr"][k * N + n], g["seg_ptr"][k * N + n + 1])
            assert np.array_equal(g["perm"][seg], np.flatnonzero((ei[0] == n) & (d == k)))
            cs = g["cperm"][g["cseg_ptr"][k * N + n]:g["cseg_ptr"][k * N + n + 1]]
            assert np.array_equal(cs, np.flatnonzero((g["scol"] == n) & (sd == k)))
        assert np.array_equal(g["rperm"][g["rseg_ptr"][n]:g["rseg_ptr"][n + 1]], np.flatnonzero(g["srow"] == n))
        assert np.array_equal(g["cperm_all"][g["cseg_all"][n]:g["cseg_all"][n + 1]], np.flatnonzero(g["scol"] == n))
    assert g["seg_ptr"][-1] == E and g["cseg_ptr"][-1] == E and g["rseg_ptr"][-1] == E and g["cseg_all"][-1] == E


@pytest.mark.parametrize("agg", ["sum", "mean"])
def test_grad_matches_autograd_through_index_add(agg):
    m, dim, x_size = 500, 6, 11
    row = (R.synth.uniform01(9, m, stream=2) * x_size).astype(np.int64)
    row[row == 5] = 6
    src = torch.from_numpy(R.normal_values(9, (m, dim), stream=1).astype(np.float64)).requires_grad_(True)
    out = torch.zeros((x_size, dim), dtype=torch.float64).index_add_(0, torch.from_numpy(row), src)
    if agg == "mean":
        out = out / torch.bincount(torch.from_numpy(row), minlength=x_size).clamp(min=1).double()[:, None]
    g = R.normal_values(9, (x_size, dim), stream=3).astype(np.float64)
    (out * torch.from_numpy(g)).sum().backward()
    got = R.seg_reduce_grad(g, row, agg)
    assert np.abs(got - src.grad.numpy()).max() <= 1e-15


def test_max_grad_goes_to_the_first_maximum_only():
    #            row:   0    0    0    1    1    2   (parked)
    src = np.array([[0.0, 2.0], [0.0, 2.0], [0.0, 1.0], [3.0, 0.0], [3.0, 0.5], [-1.0, -1.0], [9.0, 9.0]], np.float32)
    row = np.array([0, 0, 0, 1, 1, 2, 7])
    g = np.array([[10.0, 20.0], [30.0, 40.0], [50.0, 60.0], [70.0, 80.0]])   # segment 3 is empty
    got = R.seg_reduce_grad(g, row, "max", src=src)
    want = np.array([[10.0, 20.0], [0, 0], [0, 0], [30.0, 0], [0, 40.0], [50.0, 60.0], [0, 0]])
    assert np.array_equal(got, want)
    # the same from an arg-max handed in, and the parked row gets nothing under sum / mean either
    lst, ptr, _ = R.rows_to_csr(row, 4)
    vals, arg = R.seg_reduce_seq(src, ptr, 4, "max", list=lst)
    assert np.array_equal(arg, [[0, 0], [3, 4], [5, 5], [-1, -1]]) and np.array_equal(vals, [[0, 2], [3, 0.5], [-1, -1], [0, 0]])
    assert np.array_equal(R.seg_reduce_grad(g, row, "max", argmax=arg), want)
    assert not R.seg_reduce_grad(g, row, "sum")[6].any() and not R.seg_reduce_grad(g, row, "mean")[6].any()
    assert np.array_equal(R.seg_reduce_grad(g, row, "mean")[0], g[0] / 3)
