"""Pins tests/wgrad_ref.py (the float64 reference of the weight-gradient tests) on the CPU: against torch.autograd of
F.linear(torch.cat([H, H2], 1)[h_idx], W) with the upstream gradient dZ[dz_idx], and against a plain Python loop over the documented
formula on a tiny case with a row range, both gathers, csplit, paddings and batch strides."""
import numpy as np
import torch
import torch.nn.functional as F

from mpntrackseg_amd import synth
from wgrad_ref import Product, reference, reference_float32


def rnd(seed, shape, stream):
    return torch.from_numpy(synth.normal(seed, shape, stream=stream))


def flat(t, ld):
    """[b, r, c] -> flat buffer with leading dimension ld, NaN in the padding; (buffer, batch stride)"""
    b, r, c = t.shape
    buf = torch.full((b, r, ld), float("nan"))
    buf[:, :, :c] = t
    return buf.reshape(-1), r * ld


def test_reference_matches_autograd():
    rows, src, nb, n_out, k_in, csplit = 37, 23, 3, 5, 12, 8
    dz, h = rnd(1, (nb, src, n_out), 1), rnd(1, (nb, src, k_in), 2)
    perm = torch.from_numpy(np.argsort(synth.uniform01(1, rows, stream=3)).astype(np.int32)) % src
    hidx = torch.from_numpy((synth.uniform01(1, rows, stream=4) * src).astype(np.int32))
    zb, zs = flat(dz, n_out + 4)
    h1, s1 = flat(h[:, :, :csplit], csplit + 8)
    h2, s2 = flat(h[:, :, csplit:], k_in - csplit + 4)
    p = Product(zb, n_out + 4, zs, h1, csplit + 8, s1, rows, nb, n_out, k_in, groups=((0, 20), (20, rows)), dz_idx=perm, h_idx=hidx,
                H2=h2, ldh2=k_in - csplit + 4, h2_bstride=s2, csplit=csplit)
    ref = reference(p)
    for g, (b, e) in enumerate(p.groups):
        W = torch.zeros((n_out, k_in), dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(n_out, dtype=torch.float64, requires_grad=True)
        for i in range(nb):
            x = torch.cat([h[i, :, :csplit], h[i, :, csplit:]], 1).double()[hidx.long()][b:e]
            F.linear(x, W, bias).backward(dz[i].double()[perm.long()][b:e])
        assert torch.allclose(ref[g][0], W.grad, rtol=1e-13, atol=1e-13)
        assert torch.allclose(ref[g][1], bias.grad, rtol=1e-13, atol=1e-13)
    # the float32 evaluation is the same function: within fp32 rounding of it
    for (w64, b64), (w32, b32) in zip(ref, reference_float32(p)):
        assert float((w32.double() - w64).abs().max()) < 1e-5 * float(w64.abs().max())
        assert float((b32.double() - b64).abs().max()) < 1e-5 * float(b64.abs().max())


def test_reference_matches_plain_loop():
    rows, nb, n_out, k_in, csplit, ldz, ldh, ldh2 = 7, 2, 3, 4, 1, 5, 2, 6
    zb_stride, hb_stride, h2b_stride = 0, rows * ldh, rows * ldh2 + 3
    dZ = rnd(2, (rows * ldz,), 1)
    H = rnd(2, (nb * hb_stride,), 2)
    H2 = rnd(2, (nb * h2b_stride,), 3)
    dz_idx = torch.tensor([6, 0, 3, 3, 1, 5, 2], dtype=torch.int32)
    h_idx = torch.tensor([1, 1, 4, 0, 6, 2, 5], dtype=torch.int32)
    groups = ((2, 6), (6, 9))     # the second range ends past `rows`: clipped
    p = Product(dZ, ldz, zb_stride, H, ldh, hb_stride, rows, nb, n_out, k_in, groups=groups, dz_idx=dz_idx, h_idx=h_idx, H2=H2, ldh2=ldh2,
                h2_bstride=h2b_stride, csplit=csplit)
    for bf16 in (False, True):
        rd = (lambda v: float(torch.tensor(v).to(torch.bfloat16))) if bf16 else (lambda v: v)
        ref = reference(p, bf16=bf16)
        for g, (rb, re) in enumerate(groups):
            gw = [[0.0] * k_in for _ in range(n_out)]
            gb = [0.0] * n_out
            for b in range(nb):
                for r in range(rb, min(re, rows)):
                    for o in range(n_out):
                        z = float(dZ[b * zb_stride + int(dz_idx[r]) * ldz + o])
                        gb[o] += z
                        for c in range(k_in):
                            i = int(h_idx[r])
                            h = float(H[b * hb_stride + i * ldh + c]) if c < csplit else float(H2[b * h2b_stride + i * ldh2 + c - csplit])
                            gw[o][c] += rd(z) * rd(h)
            assert torch.allclose(ref[g][0], torch.tensor(gw, dtype=torch.float64), rtol=1e-14, atol=1e-14)
            assert torch.allclose(ref[g][1], torch.tensor(gb, dtype=torch.float64), rtol=1e-14, atol=1e-14)


def test_exact_family_guard():
    """the exact family's precondition is asserted by the reference itself"""
    import pytest
    q = torch.tensor([0.25, -4.0, 1.5, 0.0])
    ok = Product(q, 1, 0, q, 1, 0, 4, 1, 1, 1)
    assert float(reference(ok, exact=True)[0][0]) == 0.0625 + 16.0 + 2.25
    with pytest.raises(AssertionError):
        reference(Product(q * 0.5, 1, 0, q, 1, 0, 4, 1, 1, 1), exact=True)      # 1/8 is no multiple of 1/4
    with pytest.raises(AssertionError):
        reference(Product(q.repeat(20000), 1, 0, q.repeat(20000), 1, 0, 80000, 1, 1, 1), exact=True)   # 80000 * 256 >= 2^24
