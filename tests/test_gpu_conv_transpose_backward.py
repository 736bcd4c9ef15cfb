"""Operator-level parity of the native ConvTranspose2d(2, stride 2) backward (csrc/conv_backward.hip: the gate / space-to-depth /
bias pre-pass, the data gradient as a 1 x 1 product through the forward's own kernels, convt_wgrad_kernel and at cin <= 8 the plain
weight-gradient kernel with the roles swapped) through mpnhip_conv_transpose2d_backward and ``conv_transpose2d_native_autograd``, against
torch.nn.functional.conv_transpose2d (+ relu) under autograd on the CPU in float64 on the same float32 values.

Measure and bound are those of tests/test_gpu_conv_backward.py: max |got - ref64| / max |ref64| per quantity, bound
max(2e-6, 4 x the error of torch's float32 CPU autograd on the same inputs against the same reference).  Every case prints both.

With a ReLU the operator-level cases hand the kernel the float64 reference's output rounded to float32 as ``y``, and the float32 CPU
evaluation is checked to gate the same elements (the seed was picked on the CPU so that it does)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.cnn import conv2d_native, conv_transpose2d_native_autograd, conv_transpose2d_native_backward

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 2e-6
WG_IMAGES = 8            # csrc/conv_backward.hip: images per block of the weight gradient (and of the bias partial sums)
SEED = 41
COUNTERS = ("conv_tile", "conv_small_cout", "conv_transpose", "layer_norm", "conv_bwd_gate", "conv_wgrad", "conv_wgrad_plain",
            "conv_transpose_bwd", "layer_norm_bwd")


def nerr(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def normal(seed, shape, std=1.0, stream=0):
    return torch.from_numpy(synth.normal(seed, shape, stream=stream, std=std))


def bwd_case(seed, n, seg_channels, cout, h, w):
    """float32 CPU tensors: one input per segment, He-scaled weight [cin, cout, 2, 2], small bias, grad_out [n, cout, 2 h, 2 w]."""
    cin = sum(seg_channels)
    xs = [normal(seed, (n, c, h, w), stream=10 + i) for i, c in enumerate(seg_channels)]
    wt = normal(seed, (cin, cout, 2, 2), std=math.sqrt(2.0 / cin), stream=1)
    b = normal(seed, (cout,), std=0.05, stream=2)
    go = normal(seed, (n, cout, 2 * h, 2 * w), stream=3)
    return xs, wt, b, go


def reference(xs, wt, b, go, relu, dtype):
    """(y, [grad per segment], grad_weight, grad_bias) of conv_transpose2d (+ relu) under torch autograd on the CPU in ``dtype``."""
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in list(xs) + [wt, b]]
    y = F.conv_transpose2d(torch.cat(leaves[:len(xs)], 1), leaves[-2], leaves[-1], stride=2)
    if relu:
        y = y.relu()
    grads = torch.autograd.grad(y, leaves, go.to(dtype))
    return y.detach(), list(grads[:len(xs)]), grads[-2], grads[-1]


def counters_after(fn):
    capi.path_counters(reset=True)
    out = fn()
    torch.cuda.synchronize()
    c = capi.path_counters()
    return out, {k: c[k] for k in COUNTERS}


def expected_counts(cin, cout, need_input=True, need_weight=True, forwards=0):
    """One conv_transpose_bwd per call; the data gradient is a 1 x 1 forward product with cin output channels; the weight gradient
    has a kernel of its own (no counter but the call's) except at cin <= 8, where it is the Conv2d backward's plain kernel;
    ``forwards``: launches of the transposed forward."""
    want = dict.fromkeys(COUNTERS, 0)
    want["conv_transpose_bwd"] = 1
    if need_weight and cin <= 8:
        want["conv_wgrad_plain"] = 1
    if need_input:
        want["conv_small_cout" if cin <= 8 else "conv_tile"] = 1
    want["conv_transpose"] = forwards
    return want


# (label, n, segments, cout, H, W, relu)
CASES = [
    ("predictor_64_64", 3, (64,), 64, 14, 14, True),
    ("four_tiles_28", 2, (64,), 64, 28, 28, True),
    ("tails_15x17_cout5", 1, (12, 8), 5, 15, 17, False),
    ("tails_15x17_cin5", 2, (5,), 33, 15, 17, True),
    ("one_pixel", 1, (3,), 33, 1, 1, False),
    ("splits_one_more", WG_IMAGES + 1, (8,), 40, 14, 14, True),
    ("splits_exactly", WG_IMAGES, (8,), 40, 14, 14, True),
]
BY_LABEL = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def case_data(label):
    """Inputs, float64 reference and the float32 CPU evaluation's errors of a case, computed once; nobody writes into them."""
    _, n, segs, cout, h, w, relu = BY_LABEL[label]
    xs, wt, b, go = bwd_case(SEED, n, segs, cout, h, w)
    y64, gi64, gw64, gb64 = reference(xs, wt, b, go, relu, torch.float64)
    y32, gi32, gw32, gb32 = reference(xs, wt, b, go, relu, torch.float32)
    if relu:
        assert torch.equal(y32 > 0, y64 > 0), "the float32 CPU evaluation gates other elements than the reference: pick another seed"
    e_cpu = dict(grad_in=[nerr(a, r) for a, r in zip(gi32, gi64)], grad_weight=nerr(gw32, gw64), grad_bias=nerr(gb32, gb64))
    return dict(xs=xs, wt=wt, b=b, go=go, relu=relu, y=y64.float(), gi=gi64, gw=gw64, gb=gb64, e_cpu=e_cpu)


def run_bwd(d, **need):
    y = d["y"].to(dev()) if d["relu"] else None
    return conv_transpose2d_native_backward([x.to(dev()) for x in d["xs"]], d["wt"].to(dev()), y, d["go"].to(dev()), relu=d["relu"], **need)


def check_against_reference(label, d, gi_segments, gw, gb):
    for s, (got, ref, e32) in enumerate(zip(gi_segments, d["gi"], d["e_cpu"]["grad_in"])):
        e, bound = nerr(got.cpu(), ref), max(TOL, 4 * e32)
        print("%s: grad_in segment %d: kernel %.3g, float32 CPU %.3g (bound %.3g)" % (label, s, e, e32, bound))
        assert tuple(got.shape) == tuple(ref.shape) and e < bound
    for name, got, ref in (("grad_weight", gw, d["gw"]), ("grad_bias", gb, d["gb"])):
        e, e32 = nerr(got.cpu(), ref), d["e_cpu"][name]
        bound = max(TOL, 4 * e32)
        print("%s: %s: kernel %.3g, float32 CPU %.3g (bound %.3g)" % (label, name, e, e32, bound))
        assert tuple(got.shape) == tuple(ref.shape) and e < bound


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_transpose_backward_against_float64(case):
    label, n, segs, cout, h, w, relu = case
    d = case_data(label)
    (gi, gw, gb), counts = counters_after(lambda: run_bwd(d))
    assert counts == expected_counts(sum(segs), cout), counts
    assert tuple(gi.shape) == (n, sum(segs), h, w) and gi.is_contiguous()
    offs = [sum(segs[:i]) for i in range(len(segs) + 1)]
    check_against_reference(label, d, [gi[:, offs[i]:offs[i + 1]] for i in range(len(segs))], gw, gb)


def test_outputs_are_overwritten_and_optional():
    """Each output alone: the others' kernels do not run, and what comes back is what the full call gives, bit for bit."""
    d = case_data("splits_one_more")
    full = run_bwd(d)
    for which in range(3):
        need = dict(need_input=which == 0, need_weight=which == 1, need_bias=which == 2)
        got, counts = counters_after(lambda: run_bwd(d, **need))
        assert counts == expected_counts(8, 40, need_input=which == 0, need_weight=which == 1), counts
        assert [g is not None for g in got] == [which == i for i in range(3)]
        assert torch.equal(got[which], full[which])


def test_backward_is_bitwise_repeatable_and_grad_in_batch_independent():
    d3 = case_data("predictor_64_64")
    a, b = run_bwd(d3), run_bwd(d3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    d1 = dict(d3, xs=[x[:1].clone() for x in d3["xs"]], go=d3["go"][:1].clone(), y=d3["y"][:1].clone())     # image 0 alone
    assert torch.equal(run_bwd(d1, need_weight=False, need_bias=False)[0], a[0][:1])


def test_no_images_zero_fills_weight_and_bias_gradients():
    l = capi.load()
    gw = torch.full((8, 40, 2, 2), 7.0, device=dev())
    gb = torch.full((40,), 7.0, device=dev())
    keep = torch.full((16,), 3.0, device=dev())
    a = capi.ConvBwdArgs()
    a.n_segments, a.H, a.W, a.cout, a.ksize, a.transposed, a.n_images, a.relu = 1, 14, 14, 40, 2, 1, 0, 1
    a.seg_data[0], a.seg_stride[0], a.seg_channels[0] = keep.data_ptr(), 8 * 196, 8
    a.weight = a.y = a.grad_out = a.grad_in = keep.data_ptr()
    a.grad_weight, a.grad_bias = gw.data_ptr(), gb.data_ptr()
    assert l.mpnhip_conv_transpose2d_backward_workspace_bytes(ctypes.byref(a)) == 0
    _, counts = counters_after(lambda: capi.check(l.mpnhip_conv_transpose2d_backward(ctypes.byref(a), None, 0, capi.stream_ptr()),
                                                  "mpnhip_conv_transpose2d_backward"))
    assert counts == dict.fromkeys(COUNTERS, 0), counts
    assert float(gw.abs().max()) == 0.0 and float(gb.abs().max()) == 0.0 and bool((keep == 3.0).all())


def autograd_problem():
    """Segments of 20 and 12 channels -> 16 at 14 x 14, N = 2, ReLU; the second segment is a channel slice of a wider tensor."""
    xs, wt, b, go = bwd_case(43, 2, (20, 12), 16, 14, 14)
    wide = torch.full((2, 40, 14, 14), float("nan"), dtype=torch.float32)
    wide[:, 20:32] = xs[1]
    return xs, wt, b, go, wide


def test_autograd_function_against_float64():
    xs, wt, b, go, wide = autograd_problem()
    y64, gi64, gw64, gb64 = reference(xs, wt, b, go, True, torch.float64)
    _, gi32, gw32, gb32 = reference(xs, wt, b, go, True, torch.float32)
    x0 = xs[0].to(dev()).requires_grad_(True)
    wd = wide.to(dev()).requires_grad_(True)
    w_, b_ = wt.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
    y, counts = counters_after(lambda: conv_transpose2d_native_autograd([x0, wd[:, 20:32]], w_, b_, relu=True))
    assert counts == dict(dict.fromkeys(COUNTERS, 0), conv_transpose=1), counts
    assert torch.equal(y.detach(), conv2d_native([x0.detach(), wd.detach()[:, 20:32]], w_.detach(), b_.detach(), relu=True, transposed=True))
    assert torch.equal(y.detach().cpu() > 0, y64 > 0), "the native forward gates other elements than the reference: pick another seed"
    _, counts = counters_after(lambda: y.backward(go.to(dev())))
    assert counts == expected_counts(32, 16), counts
    pairs = [("segment 0", x0.grad, gi64[0], gi32[0]), ("segment 1 (slice)", wd.grad[:, 20:32], gi64[1], gi32[1]),
             ("weight", w_.grad, gw64, gw32), ("bias", b_.grad, gb64, gb32)]
    for name, got, ref, r32 in pairs:
        e, e32 = nerr(got.cpu(), ref), nerr(r32, ref)
        bound = max(TOL, 4 * e32)
        print("autograd %s: kernel %.3g, float32 CPU %.3g (bound %.3g)" % (name, e, e32, bound))
        assert e < bound
    # the rest of the wider tensor received no gradient
    assert float(wd.grad[:, :20].abs().max()) == 0.0 and float(wd.grad[:, 32:].abs().max()) == 0.0


def test_autograd_function_with_an_expanded_grad_out():
    """``.sum().backward()`` hands over an expanded scalar (every stride 0): the gradient of sum(y)."""
    xs, wt, b, go, _ = autograd_problem()
    ones = torch.ones_like(go)
    _, gi64, gw64, gb64 = reference(xs, wt, b, ones, True, torch.float64)
    _, gi32, gw32, gb32 = reference(xs, wt, b, ones, True, torch.float32)
    leaves = [t.to(dev()).requires_grad_(True) for t in xs + [wt, b]]
    y = conv_transpose2d_native_autograd(leaves[:2], leaves[2], leaves[3], relu=True)
    y.sum().backward()
    for name, got, ref, r32 in zip(("segment 0", "segment 1", "weight", "bias"), [t.grad for t in leaves], gi64 + [gw64, gb64],
                                   gi32 + [gw32, gb32]):
        e, e32 = nerr(got.cpu(), ref), nerr(r32, ref)
        print("expanded grad_out %s: kernel %.3g, float32 CPU %.3g" % (name, e, e32))
        assert e < max(TOL, 4 * e32)


def test_needs_input_grad_decides_what_runs():
    xs, wt, b, go, _ = autograd_problem()
    # inputs that need no gradient: no data gradient
    w_, b_ = wt.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)

    def fwd_bwd(bias):
        y = conv_transpose2d_native_autograd([x.to(dev()) for x in xs], w_, bias, relu=True)
        y.backward(go.to(dev()))
    _, counts = counters_after(lambda: fwd_bwd(b_))
    assert counts == expected_counts(32, 16, need_input=False, forwards=1), counts
    assert w_.grad is not None and b_.grad is not None
    # a layer without a bias: no grad_bias
    w_.grad = b_.grad = None
    _, counts = counters_after(lambda: fwd_bwd(None))
    assert counts == expected_counts(32, 16, need_input=False, forwards=1), counts
    assert w_.grad is not None and b_.grad is None
    # the data gradient alone: no weight-gradient kernel
    x0 = xs[0].to(dev()).requires_grad_(True)
    _, counts = counters_after(lambda: conv_transpose2d_native_autograd([x0, xs[1].to(dev())], w_.detach(), None).backward(go.to(dev())))
    assert counts == expected_counts(32, 16, need_weight=False, forwards=1), counts
    assert x0.grad is not None


def test_relu_gate_at_exactly_zero():
    """A channel whose bias is very negative: its output is exactly 0 everywhere, torch's ReLU backward gives it no gradient, and
    its columns of grad_weight and its grad_bias are exactly 0.0."""
    xs, wt, b, go, _ = autograd_problem()
    b = b.clone()
    b[5] = -1e4
    leaves = [t.to(dev()).requires_grad_(True) for t in xs + [wt, b]]
    y = conv_transpose2d_native_autograd(leaves[:2], leaves[2], leaves[3], relu=True)
    assert float(y.detach()[:, 5].abs().max()) == 0.0 and float(y.detach()[:, 4].abs().max()) > 0
    y.backward(go.to(dev()))
    gw, gb = leaves[2].grad, leaves[3].grad
    assert float(gw[:, 5].abs().max()) == 0.0 and float(gb[5]) == 0.0
    assert float(gw[:, 4].abs().max()) > 0 and float(gb[4].abs()) > 0
