"""The feature pyramid's lateral convolution (csrc/conv_strided.hip: conv_affine_tile_kernel's UP epilogue) through the C ABI
(mpnhip_conv2d_affine_up_forward) against conv2d + bias + F.interpolate(coarser, size, mode='nearest') evaluated on the CPU in
float64 on the same float32 inputs.

Error measure and bound as in tests/test_gpu_conv_strided.py: nerr = max |got - ref64| / max |ref64| below max(2e-6, 4 x max(nerr of
torch's float32 CPU evaluation, nerr of torch's float32 device evaluation)).  With a residual of the output's own size the entry
point must give the bits of mpnhip_conv2d_affine_forward."""
import math

import pytest
import torch
import torch.nn.functional as F

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.fpn_net import conv2d_affine_up_native
from mpntrackseg_amd.reid_net import conv2d_affine_native

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 2e-6

# (label, n, cin, cout, Hout, Wout, rh, rw, k)
CASES = [
    ("odd_13x9_from_7x5", 2, 40, 24, 13, 9, 7, 5, 1),         # no factor of two; row 12 and column 8 read the last source cell
    ("double_8x6_from_4x3", 2, 40, 24, 8, 6, 4, 3, 1),
    ("lateral_2048_4x6_from_2x3", 2, 2048, 256, 4, 6, 2, 3, 1),    # the longest lateral chain
    ("k3_grouped_9x7_from_3x2", 1, 260, 70, 9, 7, 3, 2, 3),      # the other kernel size, K = 2340: the grouped chain, M and K tails
]
BY_LABEL = {c[0]: c for c in CASES}


def nerr(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def normal(seed, shape, std=1.0, stream=0):
    return torch.from_numpy(synth.normal(seed, shape, stream=stream, std=std))


def make_case(seed, n, cin, cout, h, w, rh, rw, k):
    x = normal(seed, (n, cin, h, w), stream=10)
    wt = normal(seed, (cout, cin, k, k), std=math.sqrt(2.0 / (cin * k * k)), stream=1)
    bias = normal(seed, (cout,), std=0.05, stream=3)
    res = normal(seed, (n, cout, rh, rw), stream=4)
    return x, wt, bias, res


def reference(x, wt, bias, res, dtype, device="cpu"):
    x, wt, bias, res = (t.to(device).to(dtype) for t in (x, wt, bias, res))
    y = F.conv2d(x, wt, bias, padding=wt.shape[2] // 2)
    return y + F.interpolate(res, size=y.shape[-2:], mode='nearest')


def run(x, wt, bias, res):
    return conv2d_affine_up_native(x.to(dev()), wt.to(dev()), None, bias.to(dev()), res.to(dev()))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_lateral_against_float64(case):
    label, n, cin, cout, h, w, rh, rw, k = case
    x, wt, bias, res = make_case(61, n, cin, cout, h, w, rh, rw, k)
    ref = reference(x, wt, bias, res, torch.float64)
    capi.path_counters(reset=True)
    got = run(x, wt, bias, res)
    torch.cuda.synchronize()
    c = capi.path_counters()
    e_gpu = nerr(got.cpu(), ref)
    e_cpu = nerr(reference(x, wt, bias, res, torch.float32), ref)
    e_dev = nerr(reference(x, wt, bias, res, torch.float32, dev()).cpu(), ref)
    bound = max(TOL, 4 * max(e_cpu, e_dev))
    print("%s: kernel %.3g, float32 CPU %.3g, stock device %.3g (bound %.3g)" % (label, e_gpu, e_cpu, e_dev, bound))
    assert c["conv_affine_up"] == 1 and c["conv_affine_tile"] == 1 and c["conv_affine_small_grid"] == 1 and c["conv_tile"] == 0, c
    assert c["conv_affine_grouped"] == int(cin * k * k > 2048)
    assert tuple(got.shape) == tuple(ref.shape) == (n, cout, h, w)
    assert e_gpu < bound


def test_the_source_cells_are_atens():
    """a convolution of zeros leaves the upsampled map alone: every output equals F.interpolate's cell exactly, for sizes whose
    ratio is no integer in either direction (the residual may also be the LARGER map)"""
    for (h, w, rh, rw) in ((13, 9, 7, 5), (5, 7, 13, 3), (1, 1, 4, 4), (6, 10, 1, 1)):
        x = torch.zeros((2, 8, h, w))
        wt = normal(62, (33, 8, 1, 1), stream=1)
        res = normal(62, (2, 33, rh, rw), stream=4)
        got = conv2d_affine_up_native(x.to(dev()), wt.to(dev()), None, None, res.to(dev())).cpu()
        assert torch.equal(got, F.interpolate(res, size=(h, w), mode='nearest')), (h, w, rh, rw)


@pytest.mark.parametrize("label", ["odd_13x9_from_7x5", "k3_grouped_9x7_from_3x2"])
def test_a_residual_of_the_outputs_size_is_the_plain_entry_point(label):
    _, n, cin, cout, h, w, _, _, k = BY_LABEL[label]
    x, wt, bias, res = make_case(63, n, cin, cout, h, w, h, w, k)
    scale = torch.from_numpy((0.75 + 0.5 * synth.uniform01(63, cout, stream=2)).astype("float32"))
    dx, dw, dsc, db, dres = (t.to(dev()) for t in (x, wt, scale, bias, res))
    for sc in (None, dsc):
        for relu in (False, True):
            plain = conv2d_affine_native(dx, dw, sc, db, residual=dres, relu=relu)
            up = conv2d_affine_up_native(dx, dw, sc, db, dres, relu=relu)
            assert torch.equal(up, plain), (label, sc is None, relu)


def test_bits_do_not_depend_on_the_batch():
    _, _, cin, cout, h, w, rh, rw, k = BY_LABEL["odd_13x9_from_7x5"]
    x, wt, bias, res = make_case(64, 5, cin, cout, h, w, rh, rw, k)
    whole = run(x, wt, bias, res)
    for i in (0, 2, 4):
        one = run(x[i:i + 1], wt, bias, res[i:i + 1])
        assert torch.equal(one[0], whole[i]), i


def test_large_blocks_and_channel_slices():
    """enough columns for the 128 x 128 block (the full-size laterals): its bits are the small block's; the residual read from,
    and the output written into, a channel slice of wider tensors"""
    n, cin, cout, h, w, rh, rw = 24, 32, 256, 56, 50, 28, 25          # 67200 columns: 525 x 2 blocks of 128 x 128
    x, wt, bias, res = make_case(65, n, cin, cout, h, w, rh, rw, 1)
    dx, dw, db, dres = (t.to(dev()) for t in (x, wt, bias, res))
    capi.path_counters(reset=True)
    whole = conv2d_affine_up_native(dx, dw, None, db, dres)
    c = capi.path_counters()
    assert c["conv_affine_up"] == 1 and c["conv_affine_small_grid"] == 0 and c["conv_affine_wide"] == 0, c
    wide_res = torch.full((1, cout + 6, rh, rw), 3.0, dtype=torch.float32, device=dev())
    wide_res[:, 4:4 + cout] = dres[n - 1:]
    wide = torch.full((1, cout + 3, h, w), -7.5, dtype=torch.float32, device=dev())
    capi.path_counters(reset=True)
    one = conv2d_affine_up_native(dx[n - 1:], dw, None, db, wide_res[:, 4:4 + cout], out=wide[:, 2:2 + cout])
    assert capi.path_counters()["conv_affine_small_grid"] == 1
    assert torch.equal(one[0], whole[n - 1])
    assert torch.equal(wide[:, :2].cpu(), torch.full((1, 2, h, w), -7.5)) and torch.equal(wide[:, 2 + cout:].cpu(), torch.full((1, 1, h, w), -7.5))
    ref = reference(x[n - 1:], wt, bias, res[n - 1:], torch.float64)
    e_gpu, e_cpu = nerr(whole[n - 1:].cpu(), ref), nerr(reference(x[n - 1:], wt, bias, res[n - 1:], torch.float32), ref)
    print("large blocks: kernel %.3g, float32 CPU %.3g" % (e_gpu, e_cpu))
    assert e_gpu < max(TOL, 4 * e_cpu)
