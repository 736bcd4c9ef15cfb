"""Operator-level parity of the ReID network's native layers (csrc/conv_strided.hip: conv_affine_tile_kernel, maxpool3s2_kernel)
through the C ABI (mpnhip_conv2d_affine_forward, mpnhip_maxpool2d_forward) against torch.nn.functional.conv2d(..., stride,
padding), the affine, the residual and the ReLU evaluated on the CPU in float64 on the same float32 inputs.

Error measure: nerr of tests/test_gpu_conv.py, max |got - ref64| / max |ref64|.  Bound per case: max(2e-6, 4 x nerr of torch's
float32 CPU evaluation of the same case) -- 2e-6 is what the project holds the same exact-fp32 MFMA chain to up to K = 2048; the
second term is the LayerNorm rule of test_gpu_conv.py, there because two cases have K = 4608, where nobody has measured the chain.
Every case prints both errors and asserts through capi.path_counters which variant ran (conv_affine_grouped counts, beside
conv_affine_tile, the launches whose K is above 2048 and whose chain is therefore cut into groups of four chunks: as ONE chain
layer4_3x3_k4608 measured 2.53e-6 on the MI355X against its bound of 2e-6, layer4_1x1_k2048 1.53e-6).  Inputs: synth.normal;
weights He-scaled; scale in [0.75, 1.25], shift std 0.1.  The max-pool must equal torch's bit for bit."""
import math

import pytest
import torch
import torch.nn.functional as F

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.reid_net import conv2d_affine_native, maxpool2d_native

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 2e-6
COUNTERS = ("conv_affine_tile", "conv_affine_grouped", "conv_affine_small_grid", "conv_affine_wide", "maxpool", "conv_tile", "conv_small_cout")
GROUP_MIN_K = 2048      # CA_GROUP_MIN_K of csrc/conv_strided.hip: K above it takes the grouped summation
SMALL_GRID = 512        # CA_SMALL_GRID: fewer blocks of the large shape than this take the 64 x 64 block


def nerr(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def normal(seed, shape, std=1.0, stream=0):
    return torch.from_numpy(synth.normal(seed, shape, stream=stream, std=std))


def make_case(seed, n, cin, cout, h, w, k, s, affine=True, residual=False):
    """float32 CPU tensors: input, He-scaled weight, scale in [0.75, 1.25], shift N(0, 0.1^2), residual N(0, 1)"""
    x = normal(seed, (n, cin, h, w), stream=10)
    wt = normal(seed, (cout, cin, k, k), std=math.sqrt(2.0 / (cin * k * k)), stream=1)
    scale = torch.from_numpy((0.75 + 0.5 * synth.uniform01(seed, cout, stream=2)).astype("float32")) if affine else None
    shift = normal(seed, (cout,), std=0.1, stream=3) if affine else None
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    res = normal(seed, (n, cout, ho, wo), stream=4) if residual else None
    return x, wt, scale, shift, res


def reference(x, wt, scale, shift, res, s, relu, dtype):
    y = F.conv2d(x.to(dtype), wt.to(dtype), None, stride=s, padding=wt.shape[2] // 2)
    if scale is not None:
        y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    if res is not None:
        y = y + res.to(dtype)
    return y.relu() if relu else y


def counters_after(fn):
    capi.path_counters(reset=True)
    out = fn()
    torch.cuda.synchronize()
    c = capi.path_counters()
    return out, {k: c[k] for k in COUNTERS}


def only(name, grouped=False, small=False, wide=False):
    extra = {"conv_affine_grouped": grouped, "conv_affine_small_grid": small, "conv_affine_wide": wide}
    return {k: int(k == name or bool(extra.get(k))) for k in COUNTERS}


def small_grid(n, cout, h, w, k, s):
    """the launch takes the 64 x 64 block: conv_strided.hip's rule (never for the 7 x 7)"""
    cols = n * ((h - 1) // s + 1) * ((w - 1) // s + 1)
    blocks = -(-cols // 256) if cout <= 64 else -(-cols // 128) * -(-cout // 128)
    return k != 7 and blocks < SMALL_GRID


def to_dev(t):
    return None if t is None else t.to(dev())


def run(x, wt, scale, shift, res, s, relu, out=None):
    return conv2d_affine_native(to_dev(x), to_dev(wt), to_dev(scale), to_dev(shift), stride=s, residual=to_dev(res), relu=relu, out=out)


# (label, n, cin, cout, H, W, k, stride, affine, residual, relu)
CASES = [
    ("stem_7x7_s2", 2, 3, 64, 128, 64, 7, 2, True, False, True),                 # the real stem
    ("stem_odd", 1, 3, 33, 13, 9, 7, 2, True, False, True),                      # odd sizes, M tail
    ("s2_3x3_straddle", 3, 20, 40, 15, 9, 3, 2, True, False, True),              # 40 pixels per image: tiles straddle images; K tail
    ("down_1x1_s2", 5, 24, 72, 16, 8, 1, 2, False, False, False),                # no scale, no residual, no ReLU
    ("one_pixel", 1, 5, 65, 1, 1, 3, 2, True, False, True),                      # smallest possible image
    ("layer4_1x1_k2048", 3, 2048, 512, 8, 4, 1, 1, True, False, True),           # residual absent, ReLU
    ("layer4_expand_residual", 3, 512, 2048, 8, 4, 1, 1, True, True, True),      # residual + ReLU
    ("layer4_3x3_k4608", 2, 512, 512, 8, 4, 3, 1, True, False, True),            # the longest chain of the network
    ("layer3_3x3_s2", 2, 256, 256, 16, 8, 3, 2, True, False, True),              # a real strided layer
    ("layer1_1x1_cout64", 2, 256, 64, 32, 16, 1, 1, True, False, True),          # cout <= 64 (4 blocks: the 64 x 64 block, as every case here but the stem)
]
BY_LABEL = {c[0]: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_affine_against_float64(case):
    label, n, cin, cout, h, w, k, s, affine, residual, relu = case
    x, wt, scale, shift, res = make_case(26, n, cin, cout, h, w, k, s, affine, residual)
    ref = reference(x, wt, scale, shift, res, s, relu, torch.float64)
    got, counts = counters_after(lambda: run(x, wt, scale, shift, res, s, relu))
    e_gpu, e_cpu = nerr(got.cpu(), ref), nerr(reference(x, wt, scale, shift, res, s, relu, torch.float32), ref)
    bound = max(TOL, 4 * e_cpu)
    print("%s: kernel %.3g, float32 CPU %.3g (bound %.3g)" % (label, e_gpu, e_cpu, bound))
    assert counts == only("conv_affine_tile", grouped=cin * k * k > GROUP_MIN_K, small=small_grid(n, cout, h, w, k, s)), counts
    assert tuple(got.shape) == tuple(ref.shape) == (n, cout, (h - 1) // s + 1, (w - 1) // s + 1)
    assert e_gpu < bound


def test_conv_affine_into_and_out_of_channel_slices():
    """3 x 3 s2 20 -> 40 read from channels 4 .. 23 of a [3, 30, 15, 9] tensor and written into channels 8 .. 47 of a
    [3, 56, 8, 5] tensor: the other output channels keep their sentinel bit for bit, and the bits are those of the dense call."""
    label, n, cin, cout, h, w, k, s, affine, residual, relu = BY_LABEL["s2_3x3_straddle"]
    x, wt, scale, shift, res = make_case(27, n, cin, cout, h, w, k, s, affine, True)
    dense = run(x, wt, scale, shift, res, s, relu)
    sentinel = -12345.678
    wide_in = torch.full((n, 30, h, w), 7.0, dtype=torch.float32, device=dev())
    wide_in[:, 4:24] = x.to(dev())
    wide_res = torch.full((n, 50, 8, 5), 3.0, dtype=torch.float32, device=dev())
    wide_res[:, 10:50] = res.to(dev())
    wide = torch.full((n, 56, 8, 5), sentinel, dtype=torch.float32, device=dev())
    got, counts = counters_after(lambda: conv2d_affine_native(wide_in[:, 4:24], to_dev(wt), to_dev(scale), to_dev(shift), stride=s,
                                                              residual=wide_res[:, 10:50], relu=relu, out=wide[:, 8:48]))
    assert counts == only("conv_affine_tile", small=True), counts
    assert got.data_ptr() == wide[:, 8:48].data_ptr()
    assert torch.equal(wide[:, 8:48], dense)
    rest = torch.cat([wide[:, :8], wide[:, 48:]], dim=1).cpu()
    assert torch.equal(rest, torch.full((n, 16, 8, 5), sentinel, dtype=torch.float32))
    ref = reference(x, wt, scale, shift, res, s, relu, torch.float64)
    e_gpu, e_cpu = nerr(dense.cpu(), ref), nerr(reference(x, wt, scale, shift, res, s, relu, torch.float32), ref)
    print("slices: kernel %.3g, float32 CPU %.3g" % (e_gpu, e_cpu))
    assert e_gpu < max(TOL, 4 * e_cpu)


@pytest.mark.parametrize("label", ["s2_3x3_straddle", "layer4_expand_residual"])
def test_bits_do_not_depend_on_the_batch(label):
    """image i of a 5-image call equals the 1-image call on image i under torch.equal"""
    _, _, cin, cout, h, w, k, s, affine, residual, relu = BY_LABEL[label]
    x, wt, scale, shift, res = make_case(28, 5, cin, cout, h, w, k, s, affine, residual)
    whole = run(x, wt, scale, shift, res, s, relu)
    for i in (0, 2, 4):
        one = run(x[i:i + 1], wt, scale, shift, None if res is None else res[i:i + 1], s, relu)
        assert torch.equal(one[0], whole[i]), (label, i)


# (label, n, cin, cout, H, W, k): enough columns for the large blocks -- 128 x 128, or 64 rows x 256 columns for cout <= 64
LARGE_GRIDS = [
    ("tile128_1x1", 128, 64, 2048, 8, 4, 1),
    ("tile128_3x3_grouped", 512, 256, 512, 8, 4, 3),
    ("wide256_1x1", 64, 32, 64, 64, 32, 1),
    ("wide256_3x3", 64, 8, 64, 64, 32, 3),
]


@pytest.mark.parametrize("case", LARGE_GRIDS, ids=[c[0] for c in LARGE_GRIDS])
def test_large_blocks_have_the_bits_of_the_small_ones(case):
    """The cases above run on the 64 x 64 block; a launch with 512 or more large blocks takes those.  The chain of an output is
    the same in every block shape: image i of the large launch equals the 1-image launch (64 x 64 blocks, held to float64 above
    and here) under torch.equal."""
    label, n, cin, cout, h, w, k = case
    assert not small_grid(n, cout, h, w, k, 1) and small_grid(1, cout, h, w, k, 1)
    x, wt, scale, shift, res = make_case(31, n, cin, cout, h, w, k, 1, True, True)
    dx, dw, dsc, dsh, dres = (to_dev(t) for t in (x, wt, scale, shift, res))
    grouped = cin * k * k > GROUP_MIN_K
    whole, counts = counters_after(lambda: conv2d_affine_native(dx, dw, dsc, dsh, residual=dres, relu=True))
    assert counts == only("conv_affine_tile", grouped=grouped, wide=cout <= 64), counts    # neither small nor wide: 128 x 128
    for i in (0, n // 2 + 1, n - 1):
        one, counts = counters_after(lambda: conv2d_affine_native(dx[i:i + 1], dw, dsc, dsh, residual=dres[i:i + 1], relu=True))
        assert counts == only("conv_affine_tile", grouped=grouped, small=True), counts
        assert torch.equal(one[0], whole[i]), (label, i)
    i = n - 1
    ref = reference(x[i:i + 1], wt, scale, shift, res[i:i + 1], 1, True, torch.float64)
    e_gpu, e_cpu = nerr(whole[i:i + 1].cpu(), ref), nerr(reference(x[i:i + 1], wt, scale, shift, res[i:i + 1], 1, True, torch.float32), ref)
    print("%s: kernel %.3g, float32 CPU %.3g" % (label, e_gpu, e_cpu))
    assert e_gpu < max(TOL, 4 * e_cpu)


@pytest.mark.parametrize("shape", [(2, 64, 64, 32), (3, 7, 13, 9), (1, 1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_maxpool_equals_torch(shape):
    x = normal(29, shape, stream=5)
    got, counts = counters_after(lambda: maxpool2d_native(x.to(dev())))
    assert counts == only("maxpool"), counts
    assert torch.equal(got.cpu(), F.max_pool2d(x, 3, 2, 1))


def test_maxpool_of_negative_values_is_negative():
    x = -normal(30, (2, 5, 9, 7), stream=6).abs() - 0.5
    got = maxpool2d_native(x.to(dev())).cpu()
    assert float(got.max()) < 0
    assert torch.equal(got, F.max_pool2d(x, 3, 2, 1))
    # ... and a channel slice in, a channel slice out
    wide_in = torch.zeros((2, 9, 9, 7), dtype=torch.float32, device=dev())
    wide_in[:, 2:7] = x.to(dev())
    wide = torch.full((2, 8, 5, 4), 99.0, dtype=torch.float32, device=dev())
    maxpool2d_native(wide_in[:, 2:7], out=wide[:, 1:6])
    assert torch.equal(wide[:, 1:6].cpu(), got)
    assert torch.equal(wide[:, :1].cpu(), torch.full((2, 1, 5, 4), 99.0)) and torch.equal(wide[:, 6:].cpu(), torch.full((2, 2, 5, 4), 99.0))
