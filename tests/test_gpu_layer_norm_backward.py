"""Operator-level parity of the native LayerNorm backward (csrc/conv.hip: layer_norm_bwd_image_kernel, the per-element affine
gradients over blocks of 8 images and their fixed-order sum) through mpnhip_layer_norm_backward and ``layer_norm_native_autograd``,
against torch.nn.functional.layer_norm over [C, H, W] under autograd on the CPU in float64 on the same float32 values.

Measure and bound are those of tests/test_gpu_conv_backward.py: max |got - ref64| / max |ref64| per quantity, bound
max(2e-6, 4 x the error of torch's float32 CPU autograd on the same inputs against the same reference).  Every case prints both."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.cnn import layer_norm_native, layer_norm_native_autograd, layer_norm_native_backward

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 2e-6
EPS = 1e-5


def nerr(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def normal(seed, shape, std=1.0, stream=0):
    return torch.from_numpy(synth.normal(seed, shape, stream=stream, std=std))


def reference(xs, w, go, dtype):
    """([grad per segment], grad_weight, grad_bias) of F.layer_norm over the trailing [C, H, W] on the CPU in ``dtype``."""
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in xs]
    x = torch.cat(leaves, 1)
    if w is None:
        return list(torch.autograd.grad(F.layer_norm(x, x.shape[1:], None, None, EPS), leaves, go.to(dtype))), None, None
    wl = w.detach().clone().to(dtype).requires_grad_(True)
    bl = torch.zeros_like(wl).requires_grad_(True)
    grads = torch.autograd.grad(F.layer_norm(x, x.shape[1:], wl, bl, EPS), leaves + [wl, bl], go.to(dtype))
    return list(grads[:len(xs)]), grads[-2], grads[-1]


# (label, segments, (h, w), n, mean, affine)
CASES = [
    ("model_64x196", (32, 32), (14, 14), 3, 0.0, True),
    ("splits_n9", (32, 32), (14, 14), 9, 0.0, True),
    ("less_than_a_block", (3, 2), (1, 7), 2, 0.0, True),
    ("one_pixel_per_channel", (5,), (1, 1), 1, 0.0, True),
    ("mean_10", (32, 32), (14, 14), 2, 10.0, True),
    ("no_affine", (32, 32), (14, 14), 2, 0.0, False),
]
BY_LABEL = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def case_data(label):
    """Inputs, float64 reference and the float32 CPU evaluation's errors of a case, computed once; nobody writes into them."""
    _, segs, (h, wd), n, mean, affine = BY_LABEL[label]
    c = sum(segs)
    xs = [normal(51, (n, cs, h, wd), stream=10 + i) + mean for i, cs in enumerate(segs)]
    w = 1.0 + normal(51, (c, h, wd), std=0.3, stream=1) if affine else None
    go = normal(51, (n, c, h, wd), stream=3)
    gi64, gw64, gb64 = reference(xs, w, go, torch.float64)
    gi32, gw32, gb32 = reference(xs, w, go, torch.float32)
    e_cpu = dict(grad_in=[nerr(a, r) for a, r in zip(gi32, gi64)])
    if affine:
        e_cpu.update(grad_weight=nerr(gw32, gw64), grad_bias=nerr(gb32, gb64))
    return dict(xs=xs, w=w, go=go, gi=gi64, gw=gw64, gb=gb64, e_cpu=e_cpu, affine=affine)


def run_bwd(d, xs=None, **need):
    if not d["affine"]:
        need = dict(dict(need_weight=False, need_bias=False), **need)
    xs = [x.to(dev()) for x in d["xs"]] if xs is None else xs
    return layer_norm_native_backward(xs, d["w"].to(dev()) if d["affine"] else None, EPS, d["go"].to(dev()), **need)


def counted(fn):
    capi.path_counters(reset=True)
    out = fn()
    torch.cuda.synchronize()
    c = capi.path_counters()
    return out, {k: v for k, v in c.items() if v}


def check_against_reference(label, d, gi, gw, gb):
    segs = [x.shape[1] for x in d["xs"]]
    offs = [sum(segs[:i]) for i in range(len(segs) + 1)]
    for s, (ref, e32) in enumerate(zip(d["gi"], d["e_cpu"]["grad_in"])):
        got = gi[:, offs[s]:offs[s + 1]]
        e, bound = nerr(got.cpu(), ref), max(TOL, 4 * e32)
        print("%s: grad_in segment %d: kernel %.3g, float32 CPU %.3g (bound %.3g)" % (label, s, e, e32, bound))
        assert tuple(got.shape) == tuple(ref.shape) and e < bound
    if not d["affine"]:
        assert gw is None and gb is None
        return
    for name, got, ref in (("grad_weight", gw, d["gw"]), ("grad_bias", gb, d["gb"])):
        e, e32 = nerr(got.cpu(), ref), d["e_cpu"][name]
        bound = max(TOL, 4 * e32)
        print("%s: %s: kernel %.3g, float32 CPU %.3g (bound %.3g)" % (label, name, e, e32, bound))
        assert tuple(got.shape) == tuple(ref.shape) and e < bound


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_layer_norm_backward_against_float64(case):
    label = case[0]
    d = case_data(label)
    (gi, gw, gb), counts = counted(lambda: run_bwd(d))
    assert counts == {"layer_norm_bwd": 1}, counts
    assert gi.is_contiguous()
    check_against_reference(label, d, gi, gw, gb)


def test_a_segment_that_is_a_channel_slice_of_a_wider_tensor():
    d = case_data("model_64x196")
    d = dict(d, xs=[x[:2] for x in d["xs"]], go=d["go"][:2])
    gi64, gw64, gb64 = reference(d["xs"], d["w"], d["go"], torch.float64)
    gi32, gw32, gb32 = reference(d["xs"], d["w"], d["go"], torch.float32)
    d.update(gi=gi64, gw=gw64, gb=gb64, e_cpu=dict(grad_in=[nerr(a, r) for a, r in zip(gi32, gi64)], grad_weight=nerr(gw32, gw64),
                                                     grad_bias=nerr(gb32, gb64)))
    wide = torch.full((2, 50, 14, 14), float("nan"), dtype=torch.float32)
    wide[:, 7:39] = d["xs"][1]
    wide = wide.to(dev())
    gi, gw, gb = run_bwd(d, xs=[d["xs"][0].to(dev()), wide[:, 7:39]])
    check_against_reference("channel slice", d, gi, gw, gb)
    dense = run_bwd(d)
    for a, b in zip((gi, gw, gb), dense):
        assert torch.equal(a, b)


def test_autograd_forward_is_the_native_forward_and_gradients_reach_the_leaves():
    d = case_data("model_64x196")
    x0 = d["xs"][0].to(dev()).requires_grad_(True)
    wide = torch.full((3, 50, 14, 14), float("nan"), dtype=torch.float32)
    wide[:, 7:39] = d["xs"][1]
    wide = wide.to(dev()).requires_grad_(True)
    w = d["w"].to(dev()).requires_grad_(True)
    b = normal(51, tuple(d["w"].shape), std=0.1, stream=2).to(dev()).requires_grad_(True)
    y, counts = counted(lambda: layer_norm_native_autograd([x0, wide[:, 7:39]], w, b, EPS))
    assert counts == {"layer_norm": 1}, counts
    assert torch.equal(y.detach(), layer_norm_native([x0.detach(), wide.detach()[:, 7:39]], w.detach(), b.detach(), EPS))
    _, counts = counted(lambda: y.backward(d["go"].to(dev())))
    assert counts == {"layer_norm_bwd": 1}, counts
    assert tuple(w.grad.shape) == tuple(w.shape) and tuple(b.grad.shape) == tuple(b.shape)
    gi = torch.cat((x0.grad, wide.grad[:, 7:39]), 1)
    check_against_reference("autograd", d, gi, w.grad, b.grad)
    assert float(wide.grad[:, :7].abs().max()) == 0.0 and float(wide.grad[:, 39:].abs().max()) == 0.0
    # the direct call gives the same bits
    for a, r in zip((gi, w.grad, b.grad), run_bwd(d)):
        assert torch.equal(a, r)
    # nothing but the affine wants a gradient: grad_in is not computed; an expanded grad_out (.sum().backward())
    w.grad = b.grad = None
    y = layer_norm_native_autograd([x0.detach(), wide.detach()[:, 7:39]], w, b, EPS)
    _, counts = counted(lambda: y.sum().backward())
    assert counts == {"layer_norm_bwd": 1}, counts
    assert float((b.grad - 3.0).abs().max()) == 0.0 and w.grad is not None


def test_backward_is_bitwise_repeatable_and_grad_in_batch_independent():
    d9 = case_data("splits_n9")
    a, b = run_bwd(d9), run_bwd(d9)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    d1 = dict(d9, xs=[x[:1].clone() for x in d9["xs"]], go=d9["go"][:1].clone())     # image 0 alone
    assert torch.equal(run_bwd(d1, need_weight=False, need_bias=False)[0], a[0][:1])


def test_outputs_are_optional():
    """Each output alone is what the full call gives, bit for bit."""
    d = case_data("splits_n9")
    full = run_bwd(d)
    for which in range(3):
        got, counts = counted(lambda: run_bwd(d, need_input=which == 0, need_weight=which == 1, need_bias=which == 2))
        assert counts == {"layer_norm_bwd": 1}, counts
        assert [g is not None for g in got] == [which == i for i in range(3)]
        assert torch.equal(got[which], full[which])


def test_no_images_zero_fills_the_affine_gradients():
    l = capi.load()
    gw = torch.full((35,), 7.0, device=dev())
    gb = torch.full((35,), 7.0, device=dev())
    keep = torch.full((16,), 3.0, device=dev())
    data = (ctypes.c_void_p * 2)(keep.data_ptr(), keep.data_ptr())
    stride = (ctypes.c_int64 * 2)(21, 14)
    chans = (ctypes.c_int * 2)(3, 2)
    head = (data, stride, chans, 2, 0, 7, capi.ptr(keep), EPS, capi.ptr(keep), 35, capi.ptr(keep), capi.ptr(gw), capi.ptr(gb))
    assert l.mpnhip_layer_norm_backward_workspace_bytes(*head) == 0
    _, counts = counted(lambda: capi.check(l.mpnhip_layer_norm_backward(*(head + (None, 0, capi.stream_ptr()))),
                                           "mpnhip_layer_norm_backward"))
    assert counts == {}, counts
    assert float(gw.abs().max()) == 0.0 and float(gb.abs().max()) == 0.0 and bool((keep == 3.0).all())
