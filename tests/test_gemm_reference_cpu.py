"""The float64 reference of tests/test_gpu_gemm.py, checked without a GPU: on the plain cases (one group, no gather, no second K
segment, bias and ReLU only) it is torch.nn.functional.linear in float64, bit for bit up to the summation order of one matmul; the
other terms against a per-element loop."""
import numpy as np
import torch

from mpntrackseg_amd import synth
from test_gpu_gemm import reference


def normal(seed, shape, stream, std=1.0):
    return torch.from_numpy(synth.normal(seed, shape, stream=stream, std=std))


def test_reference_is_linear_on_the_plain_cases():
    for m, n, k, relu in ((1, 1, 1, 0), (5, 3, 6, 1), (130, 80, 160, 1), (64, 33, 37, 0), (200, 100, 72, 1)):
        x, w, b = normal(1, (m, k), 1), normal(1, (n, k), 2, std=(2.0 / k) ** 0.5), normal(1, (n,), 3, std=0.1)
        want = torch.nn.functional.linear(x.double(), w.double(), b.double())
        want = want.relu() if relu else want
        got = reference(torch.full((m, n), float("nan"), dtype=torch.float64), torch.arange(m), x, None, k, None, w.t(), b, None, None,
                        None, None, relu, 0, None, None)
        assert float((got - want).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max()))
        # two K segments of the same operand are the same product
        for ks in (0, k // 2):
            got2 = reference(torch.zeros((m, n), dtype=torch.float64), torch.arange(m), x[:, :ks], x[:, ks:], ks, None, w.t(), b, None,
                             None, None, None, relu, 0, None, None)
            assert float((got2 - want).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max()))


def test_reference_every_term_against_a_loop():
    m, n, k, ks, T = 9, 5, 7, 3, 4
    A, A2, B = normal(2, (6, ks), 1), normal(2, (6, k - ks), 2), normal(2, (k, n), 3)
    bias, G1, G2, mask = normal(2, (n,), 4), normal(2, (T, n), 5), normal(2, (m, n), 6), normal(2, (m, n), 7)
    mask.view(-1)[::4] = 0.0
    a_idx = torch.tensor([0, 5, 5, 2, 1, 0, 3, 4, 2], dtype=torch.int32)
    g1_idx = torch.tensor([3, 3, 0, 1, 2, 0, 1, 2, 3], dtype=torch.int32)
    c_idx = torch.from_numpy(np.array([11, 0, 7, 3, 9, 1, 4, 10, 6], dtype=np.int32))
    old = normal(2, (12, n), 8).double()
    rows = torch.arange(2, m)                     # rows 0 and 1 belong to no group
    got = reference(old.clone(), rows, A, A2, ks, a_idx, B, bias, G1, g1_idx, G2, None, 1, 1, mask, c_idx)
    want = old.clone()
    for r in rows.tolist():
        a = torch.cat([A[a_idx[r]], A2[a_idx[r]]]).double()
        for c in range(n):
            v = float((a * B[:, c].double()).sum()) + float(bias[c]) + float(G1[g1_idx[r], c]) + float(G2[r, c])
            v = max(v, 0.0) + float(old[c_idx[r], c])
            want[c_idx[r], c] = v if float(mask[r, c]) > 0 else 0.0
    assert float((got - want).abs().max()) <= 1e-13
    untouched = sorted(set(range(12)) - set(c_idx[2:].tolist()))
    assert torch.equal(got[untouched], old[untouched])
    # bf16 operands: rounded before the product, nothing else
    got16 = reference(torch.zeros((6, n), dtype=torch.float64), torch.arange(6), A, A2, ks, None, B, None, None, None, None, None, 0, 0,
                      None, None, bf16=True)
    want16 = torch.cat([A, A2], 1).bfloat16().double() @ B.bfloat16().double()
    assert torch.equal(got16, want16)
