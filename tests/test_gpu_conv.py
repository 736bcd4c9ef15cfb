"""Operator-level parity of the mask branch's native inference layers (csrc/conv.hip: conv_tile_kernel in its convolution and
transposed-convolution modes, conv_small_cout_kernel, layer_norm_kernel) through the C ABI (mpnhip_conv2d_forward,
mpnhip_layer_norm_forward) against torch.nn.functional.conv2d / conv_transpose2d / layer_norm evaluated on the CPU in float64 on
the same float32 inputs.

Error measure (as in the other operator tests): max |got - ref64| / max |ref64|.  Convolutions: 2e-6, what tests/test_gpu_gemm.py
holds the same exact-fp32 MFMA chain to up to K = 2048 (every case here has K <= 1728).  LayerNorm: max(2e-6, 4 x the error of
torch's float32 CPU layer_norm on the same inputs) -- with inputs of mean 10 the rounding of the mean dominates, and the float32
CPU evaluation shares it.  Every case prints its error beside the error of torch's float32 CPU evaluation, and asserts through
capi.path_counters which kernel variant ran.  Inputs: synth.normal; weights He-scaled."""
import math

import pytest
import torch
import torch.nn.functional as F

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.cnn import conv2d_native, layer_norm_native

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 2e-6
CONV_COUNTERS = ("conv_tile", "conv_small_cout", "conv_transpose", "layer_norm")


def nerr(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def normal(seed, shape, std=1.0, stream=0):
    return torch.from_numpy(synth.normal(seed, shape, stream=stream, std=std))


def conv_case(seed, n, seg_channels, cout, h, w, k, transposed=False):
    """float32 CPU tensors: one input per segment, He-scaled weight, small bias."""
    cin = sum(seg_channels)
    xs = [normal(seed, (n, c, h, w), stream=10 + i) for i, c in enumerate(seg_channels)]
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    wt = normal(seed, wshape, std=math.sqrt(2.0 / (cin * (1 if transposed else k * k))), stream=1)
    b = normal(seed, (cout,), std=0.05, stream=2)
    return xs, wt, b


def conv_reference(xs, wt, b, relu, transposed, dtype):
    x = torch.cat(xs, 1).to(dtype)
    if transposed:
        y = F.conv_transpose2d(x, wt.to(dtype), b.to(dtype), stride=2)
    else:
        y = F.conv2d(x, wt.to(dtype), b.to(dtype), padding=wt.shape[2] // 2)
    return y.relu() if relu else y


def counters_after(fn):
    capi.path_counters(reset=True)
    out = fn()
    torch.cuda.synchronize()
    c = capi.path_counters()
    return out, {k: c[k] for k in CONV_COUNTERS}


def only(name):
    return {k: int(k == name) for k in CONV_COUNTERS}


def run_conv(xs, wt, b, relu, transposed=False, out=None):
    # every segment is its own device allocation
    dx = [x.to(dev()) for x in xs]
    return conv2d_native(dx, wt.to(dev()), b.to(dev()), relu=relu, transposed=transposed, out=out)


def check_conv(label, xs, wt, b, relu, variant, transposed=False):
    ref = conv_reference(xs, wt, b, relu, transposed, torch.float64)
    got, counts = counters_after(lambda: run_conv(xs, wt, b, relu, transposed))
    e_gpu, e_cpu = nerr(got.cpu(), ref), nerr(conv_reference(xs, wt, b, relu, transposed, torch.float32), ref)
    print("%s: kernel %.3g, float32 CPU %.3g (bound %.1g)" % (label, e_gpu, e_cpu, TOL))
    assert counts == only(variant), counts
    assert tuple(got.shape) == tuple(ref.shape)
    assert e_gpu < TOL
    return got


# (label, n, segments, cout, H, W, k, relu, variant)
CONV_CASES = [
    ("node_model_192_96", 3, (64, 64, 64), 96, 14, 14, 3, True, "conv_tile"),
    ("four_tiles_28", 2, (64,), 64, 28, 28, 3, True, "conv_tile"),
    ("tails_15x17_cout5", 1, (12, 8), 5, 15, 17, 3, False, "conv_small_cout"),
    ("one_pixel", 1, (3,), 33, 1, 1, 3, False, "conv_tile"),
    ("two_by_three", 1, (3,), 33, 2, 3, 3, False, "conv_tile"),
    ("encoder_1x1_256_128", 2, (256,), 128, 14, 14, 1, True, "conv_tile"),
    ("last_1x1_64_1_at_56", 2, (64,), 1, 56, 56, 1, False, "conv_small_cout"),
    ("tiny_1x1_5_7", 2, (5,), 7, 3, 3, 1, True, "conv_small_cout"),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_against_float64(case):
    label, n, segs, cout, h, w, k, relu, variant = case
    xs, wt, b = conv_case(21, n, segs, cout, h, w, k)
    check_conv(label, xs, wt, b, relu, variant)


def test_conv_into_a_channel_slice_leaves_the_rest_alone():
    """3x3 96 -> 32 written into channels 32 .. 63 of a [N, 64, 14, 14] tensor: channels 0 .. 31 keep their sentinel bit for bit."""
    xs, wt, b = conv_case(22, 3, (96,), 32, 14, 14, 3)
    ref = conv_reference(xs, wt, b, True, False, torch.float64)
    sentinel = -12345.678
    wide = torch.full((3, 64, 14, 14), sentinel, dtype=torch.float32, device=dev())
    got, counts = counters_after(lambda: run_conv(xs, wt, b, True, out=wide[:, 32:]))
    assert counts == only("conv_tile"), counts
    assert got.data_ptr() == wide[:, 32:].data_ptr()
    e_gpu, e_cpu = nerr(wide[:, 32:].cpu(), ref), nerr(conv_reference(xs, wt, b, True, False, torch.float32), ref)
    print("slice_96_32: kernel %.3g, float32 CPU %.3g (bound %.1g)" % (e_gpu, e_cpu, TOL))
    assert e_gpu < TOL
    assert torch.equal(wide[:, :32].cpu(), torch.full((3, 32, 14, 14), sentinel, dtype=torch.float32))


def test_conv_reads_a_channel_slice():
    """A segment that is a channel slice of a wider tensor (image stride above its own size), as the step loop passes it."""
    xs, wt, b = conv_case(23, 2, (20, 12), 16, 14, 14, 3)
    ref = conv_reference(xs, wt, b, False, False, torch.float64)
    wide = torch.full((2, 40, 14, 14), float("nan"), dtype=torch.float32, device=dev())
    wide[:, 20:32] = xs[1].to(dev())
    got, counts = counters_after(lambda: conv2d_native([xs[0].to(dev()), wide[:, 20:32]], wt.to(dev()), b.to(dev())))
    assert counts == only("conv_tile"), counts
    e_gpu = nerr(got.cpu(), ref)
    print("read_slice: kernel %.3g (bound %.1g)" % (e_gpu, TOL))
    assert e_gpu < TOL


TRANSPOSED_CASES = [("convT_64_64_14", 2, (64,), 64, 14, 14, True), ("convT_6_3_3x5", 2, (6,), 3, 3, 5, False)]


@pytest.mark.parametrize("case", TRANSPOSED_CASES, ids=[c[0] for c in TRANSPOSED_CASES])
def test_conv_transpose_against_float64(case):
    label, n, segs, cout, h, w, relu = case
    xs, wt, b = conv_case(24, n, segs, cout, h, w, 2, transposed=True)
    got = check_conv(label, xs, wt, b, relu, "conv_transpose", transposed=True)
    assert tuple(got.shape) == (n, cout, 2 * h, 2 * w)


def test_conv_result_does_not_depend_on_the_batch():
    """The node-model layer on 5 images, then image 3 alone: bitwise equal."""
    xs, wt, b = conv_case(21, 5, (64, 64, 64), 96, 14, 14, 3)
    full, counts = counters_after(lambda: run_conv(xs, wt, b, True))
    assert counts == only("conv_tile"), counts
    alone, counts = counters_after(lambda: run_conv([x[3:4].clone() for x in xs], wt, b, True))
    assert counts == only("conv_tile"), counts
    assert torch.equal(full[3:4].cpu(), alone.cpu())
    # and the small-cout and transposed variants
    xs, wt, b = conv_case(25, 4, (64,), 1, 56, 56, 1)
    assert torch.equal(run_conv(xs, wt, b, False)[2:3].cpu(), run_conv([x[2:3].clone() for x in xs], wt, b, False).cpu())
    xs, wt, b = conv_case(26, 4, (64,), 64, 14, 14, 2, transposed=True)
    assert torch.equal(run_conv(xs, wt, b, True, transposed=True)[1:2].cpu(),
                       run_conv([x[1:2].clone() for x in xs], wt, b, True, transposed=True).cpu())


def layer_norm_check(label, xs, weight, bias, eps=1e-5):
    x = torch.cat(xs, 1)
    shape = tuple(x.shape[1:])
    ref = F.layer_norm(x.double(), shape, weight.double(), bias.double(), eps)
    e_cpu = nerr(F.layer_norm(x, shape, weight, bias, eps), ref)
    got, counts = counters_after(lambda: layer_norm_native([t.to(dev()) for t in xs], weight.to(dev()), bias.to(dev()), eps))
    e_gpu = nerr(got.cpu(), ref)
    bound = max(TOL, 4 * e_cpu)
    print("%s: kernel %.3g, float32 CPU %.3g (bound %.3g)" % (label, e_gpu, e_cpu, bound))
    assert counts == only("layer_norm"), counts
    assert e_gpu < bound


def mask_affine():
    w = synth.make_mask_weights(seed=17)
    return torch.from_numpy(w["mask_predictor.layer_norm.weight"]), torch.from_numpy(w["mask_predictor.layer_norm.bias"])


def test_layer_norm_against_float64():
    weight, bias = mask_affine()
    layer_norm_check("layer_norm_64x14x14", [normal(31, (3, 32, 14, 14), stream=s) for s in (0, 1)], weight, bias)


def test_layer_norm_with_offset_inputs():
    """Inputs of mean 10 and std 1: E[x^2] - E[x]^2 would lose the variance's low bits; the centred second pass does not."""
    weight, bias = mask_affine()
    layer_norm_check("layer_norm_offset", [10.0 + normal(32, (3, 32, 14, 14), stream=s) for s in (0, 1)], weight, bias)
