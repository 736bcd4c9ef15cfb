"""The host side of the native Conv2d backward, without a GPU: the ctypes image of mpnhip_conv_bwd_args against the header, the
argument checks of mpnhip_conv2d_backward (everything below returns before a kernel is launched: the non-null pointers are host
dummies that are never followed), the workspace size query, and the default of the ``mask_conv_grads`` selector."""
import ctypes
import os
import re

import pytest

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.mpn import MOTMPNet

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
BIG = 1 << 40        # a workspace size no layout below reaches (the buffer is never touched)


def test_conv_bwd_args_layout_matches_c():
    # 4 pointers, 4 int64, 4 ints, 7 ints (+ 4 bytes of padding), int64, pointer, pointer + int64, pointer + int64, 3 pointers
    A = capi.ConvBwdArgs
    assert ctypes.sizeof(A) == 4 * 8 + 4 * 8 + 4 * 4 + 7 * 4 + 4 + 8 + 8 + 16 + 16 + 3 * 8 == 184
    offsets = dict(seg_data=0, seg_stride=32, seg_channels=64, n_segments=80, H=84, W=88, cout=92, ksize=96, transposed=100, relu=104,
                   n_images=112, weight=120, y=128, y_stride=136, grad_out=144, grad_out_stride=152, grad_in=160, grad_weight=168,
                   grad_bias=176)
    assert [f[0] for f in A._fields_] == list(offsets)
    for name, off in offsets.items():
        assert getattr(A, name).offset == off, name
    src = open(os.path.join(REPO, "include", "mpnhip.h")).read()
    body = re.search(r"typedef struct mpnhip_conv_bwd_args \{(.*?)\} mpnhip_conv_bwd_args;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[4\])?;", body) == list(offsets)
    assert re.findall(r"(\w+)\[4\];", body) == ["seg_data", "seg_stride", "seg_channels"]
    # the leading fields are those of mpnhip_conv_args, at the same offsets: one segment list for both directions
    for name in ("seg_data", "seg_stride", "seg_channels", "n_segments", "H", "W", "cout", "ksize", "transposed", "relu", "n_images", "weight"):
        assert getattr(A, name).offset == getattr(capi.ConvArgs, name).offset, name


@pytest.fixture(scope="module")
def dummy():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.cast(buf, ctypes.c_void_p).value


def bwd_args(p, **kw):
    a = capi.ConvBwdArgs()
    a.n_segments, a.H, a.W, a.cout, a.ksize, a.n_images, a.relu = 2, 14, 14, 32, 3, 3, 1
    for i in range(2):
        a.seg_data[i], a.seg_stride[i], a.seg_channels[i] = p, 32 * 196, 32
    a.weight, a.y, a.grad_out, a.grad_in, a.grad_weight, a.grad_bias = p, p, p, p, p, p
    a.y_stride = a.grad_out_stride = 32 * 196
    for k, v in kw.items():
        if isinstance(v, tuple):     # (index, value) of one of the three segment lists
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def test_conv2d_backward_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy
    assert l.mpnhip_conv2d_backward(None, p, BIG, None) == -1
    assert b"mpnhip_conv2d_backward: null args" in l.mpnhip_last_error()
    bad_cases = [
        # what mpnhip_conv2d_forward refuses
        (dict(n_images=-1), b"n_images"),
        (dict(seg_data=(1, None)), b"segment 1: null pointer"), (dict(weight=None), b"null weight"),
        (dict(ksize=2), b"kernel size"), (dict(ksize=5), b"kernel size"), (dict(ksize=0), b"kernel size"),
        (dict(n_segments=5), b"n_segments"), (dict(n_segments=0), b"n_segments"), (dict(n_segments=-1), b"n_segments"),
        (dict(seg_channels=(0, 0)), b"segment 0: 0 channels"), (dict(seg_channels=(1, -3)), b"segment 1: -3 channels"),
        (dict(H=0), b"must be positive"), (dict(W=-2), b"must be positive"), (dict(cout=0), b"must be positive"),
        (dict(seg_stride=(0, INT32_MAX + 1)), b"segment 0: image stride"), (dict(seg_stride=(1, -1)), b"segment 1: image stride"),
        (dict(H=50000, W=50000), b"input image"),
        (dict(H=4096, W=4096, seg_channels=(0, 64), seg_stride=(0, 0), cout=200), b"output image"),
        (dict(seg_channels=(0, 30000), seg_stride=(0, 0), H=1, W=1, cout=30000), b"weight"),
        # the backward's own
        (dict(transposed=1), b"transposed"), (dict(transposed=1, ksize=2), b"transposed"),
        (dict(y=None), b"relu needs"), (dict(grad_out=None), b"null grad_out"),
        (dict(grad_in=None, grad_weight=None, grad_bias=None), b"no output wanted"),
        (dict(grad_out_stride=INT32_MAX + 1), b"grad_out_stride"), (dict(grad_out_stride=-5), b"grad_out_stride"),
        (dict(y_stride=INT32_MAX + 1), b"y_stride"),
        (dict(n_images=1 << 40, H=1, W=1), b"more than one launch holds"),
    ]
    for bad, msg in bad_cases:
        a = bwd_args(p, **bad)
        assert l.mpnhip_conv2d_backward(ctypes.byref(a), p, BIG, None) == -1, bad
        err = l.mpnhip_last_error()
        assert b"mpnhip_conv2d_backward" in err and msg in err, (bad, err)
        assert l.mpnhip_conv2d_backward_workspace_bytes(ctypes.byref(a)) == 0, bad
    # y is not looked at without a ReLU (that call gets as far as the workspace check)
    a = bwd_args(p, relu=0, y=None)
    need = l.mpnhip_conv2d_backward_workspace_bytes(ctypes.byref(a))
    assert need > 0
    # the workspace: null, or smaller than the size query says
    for ws, nbytes in ((None, BIG), (p, need - 1), (p, 0)):
        assert l.mpnhip_conv2d_backward(ctypes.byref(a), ws, nbytes, None) == -1
        assert b"mpnhip_conv2d_backward: workspace" in l.mpnhip_last_error()


def test_conv2d_backward_workspace_layout():
    """The size query: g [N][cout][hw], W' [cin][cout][taps], the weight partial sums [splits][cout][cin taps] and the bias partial
    sums [splits][cout], every region padded to 256 bytes; the split is 8 images per block, a function of N alone."""
    l = capi.load()
    buf = ctypes.create_string_buffer(8)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    up = lambda floats: (4 * floats + 255) // 256 * 256
    for n in (1, 8, 9, 280):
        splits = (n + 7) // 8
        got = l.mpnhip_conv2d_backward_workspace_bytes(ctypes.byref(bwd_args(p, n_images=n)))
        assert got == up(n * 32 * 196) + up(64 * 32 * 9) + up(splits * 32 * 64 * 9) + up(splits * 32), n
    assert l.mpnhip_conv2d_backward_workspace_bytes(None) == 0


def test_conv2d_backward_without_images_succeeds(dummy):
    """n_images == 0 with no weight / bias gradient wanted touches nothing: success without a device (with them it zero-fills
    them on the device, tests/test_gpu_conv_backward.py).  The other arguments are still checked."""
    l = capi.load()
    _, p = dummy
    a = bwd_args(p, n_images=0, grad_weight=None, grad_bias=None)
    assert l.mpnhip_conv2d_backward_workspace_bytes(ctypes.byref(a)) == 0
    assert l.mpnhip_conv2d_backward(ctypes.byref(a), None, 0, None) == 0
    assert l.mpnhip_conv2d_backward(ctypes.byref(bwd_args(p, n_images=0, grad_weight=None, grad_bias=None, ksize=7)), None, 0, None) == -1


def test_counters_of_the_backward_exist():
    names = set(capi.path_counters())
    assert {"conv_bwd_gate", "conv_wgrad", "conv_wgrad_plain"} <= names


def test_mask_conv_grads_defaults_to_stock():
    params = synth.model_params(32, 2, "sum", num_class_steps=2, node_in_dim=64)
    params.update(synth.MASK_PARAMS)
    model = MOTMPNet(params)
    assert model.mask_conv_grads == 'stock' and model.mask_convs == 'stock'
    for m in model._mask_modules():
        assert hasattr(m, "forward_native_autograd")
