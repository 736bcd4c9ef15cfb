"""The host side of the ReID network's native layers, without a GPU: the ctypes image of mpnhip_conv_affine_args against the
header, the argument checks of mpnhip_conv2d_affine_forward / mpnhip_maxpool2d_forward (everything below returns before a kernel
is launched: the non-null pointers are host dummies that are never followed), and the path-counter names."""
import ctypes
import os
import re

import pytest

from mpntrackseg_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
CONV = b"mpnhip_conv2d_affine_forward"
POOL = b"mpnhip_maxpool2d_forward"


def test_conv_affine_args_layout_matches_c():
    # 7 pointers / int64, int (+ 4 bytes of padding), pointer, 2 int64, 6 ints
    A = capi.ConvAffineArgs
    assert ctypes.sizeof(A) == 7 * 8 + 4 + 4 + 3 * 8 + 6 * 4 == 112
    offsets = dict(x=0, x_stride=8, weight=16, scale=24, shift=32, residual=40, residual_stride=48, relu=56, out=64, out_stride=72,
                   n_images=80, cin=88, cout=92, H=96, W=100, ksize=104, stride=108)
    assert [f[0] for f in A._fields_] == list(offsets)
    for name, off in offsets.items():
        assert getattr(A, name).offset == off, name
    src = open(os.path.join(REPO, "include", "mpnhip.h")).read()
    body = re.search(r"typedef struct mpnhip_conv_affine_args \{(.*?)\} mpnhip_conv_affine_args;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == list(offsets)
    # the types, in order: what ctypes mirrors
    kinds = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int}
    decl = re.findall(r"(const float\*|float\*|int64_t|int)\s+(\w+);", body)
    assert [n for _, n in decl] == list(offsets)
    assert [kinds[t] for t, _ in decl] == [f[1] for f in A._fields_]
    # the mask branch's struct is untouched
    assert ctypes.sizeof(capi.ConvArgs) == 152


@pytest.fixture(scope="module")
def dummy():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.cast(buf, ctypes.c_void_p).value


def affine_args(p, **kw):
    a = capi.ConvAffineArgs()
    a.x, a.x_stride, a.weight, a.scale, a.shift = p, 16 * 128, p, p, p
    a.residual, a.residual_stride, a.relu, a.out, a.out_stride = p, 32 * 32, 1, p, 32 * 32
    a.n_images, a.cin, a.cout, a.H, a.W, a.ksize, a.stride = 3, 16, 32, 16, 8, 3, 2
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_conv2d_affine_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy
    capi.path_counters(reset=True)
    assert l.mpnhip_conv2d_affine_forward(None, None) == -1
    assert CONV + b": null args" in l.mpnhip_last_error()
    bad_cases = [
        (dict(n_images=-1), b"n_images"),
        (dict(x=None), b"null x, weight or out"), (dict(weight=None), b"null x, weight or out"), (dict(out=None), b"null x, weight or out"),
        (dict(ksize=2), b"kernel size"), (dict(ksize=5), b"kernel size"), (dict(ksize=0), b"kernel size"), (dict(ksize=-3), b"kernel size"),
        (dict(stride=0), b"stride 0"), (dict(stride=3), b"stride 3"), (dict(stride=-1), b"stride -1"),
        (dict(H=0), b"must be positive"), (dict(W=-2), b"must be positive"), (dict(cin=0), b"must be positive"),
        (dict(cout=0), b"must be positive"), (dict(cout=-7), b"must be positive"),
        (dict(x_stride=INT32_MAX + 1), b"x_stride"), (dict(x_stride=-1), b"x_stride"),
        (dict(out_stride=INT32_MAX + 1), b"out_stride"), (dict(out_stride=-5), b"out_stride"),
        (dict(residual_stride=INT32_MAX + 1), b"residual_stride"), (dict(residual_stride=-1), b"residual_stride"),
        (dict(H=50000, W=50000, x_stride=0), b"input image"),                              # 16 channels x 2.5e9 pixels
        (dict(H=4096, W=4096, stride=1, cin=64, cout=200, x_stride=0), b"output image"),    # the input fits, the output does not
        (dict(cin=30000, cout=30000, H=1, W=1, ksize=3), b"weight"),
        (dict(cin=1, cout=1, H=2048, W=2048, stride=1, ksize=1, n_images=1024), b"column index"),   # 2^32 output pixels
        # the last block's column indices run up to 255 past the last column: they must fit an int as well
        (dict(cin=1, cout=1, H=1, W=1, stride=1, ksize=1, n_images=INT32_MAX - 255), b"column index"),
        (dict(cin=1, cout=1, H=1, W=1, stride=1, ksize=1, n_images=INT32_MAX), b"column index"),
        (dict(cin=1, cout=5000000, H=1, W=1, ksize=1, stride=1), b"more than one launch holds"),
    ]
    for bad, msg in bad_cases:
        assert l.mpnhip_conv2d_affine_forward(ctypes.byref(affine_args(p, **bad)), None) == -1, bad
        err = l.mpnhip_last_error()
        assert CONV in err and msg in err, (bad, err)
    # no images: a successful no-op whatever else the struct holds
    assert l.mpnhip_conv2d_affine_forward(ctypes.byref(affine_args(p, n_images=0)), None) == 0
    assert l.mpnhip_conv2d_affine_forward(ctypes.byref(affine_args(p, n_images=0, x=None, weight=None, out=None, ksize=4, stride=9, H=0)),
                                          None) == 0
    assert all(v == 0 for v in capi.path_counters().values())


def test_maxpool_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy
    capi.path_counters(reset=True)

    def call(x=p, x_stride=64 * 64 * 32, n_images=2, C=64, H=64, W=32, out=p, out_stride=64 * 32 * 16):
        return l.mpnhip_maxpool2d_forward(x, x_stride, n_images, C, H, W, out, out_stride, None)

    for bad, msg in ((dict(n_images=-1), b"n_images"), (dict(x=None), b"null x or out"), (dict(out=None), b"null x or out"),
                     (dict(C=0), b"must be positive"), (dict(H=0), b"must be positive"), (dict(W=-1), b"must be positive"),
                     (dict(x_stride=INT32_MAX + 1), b"x_stride"), (dict(x_stride=-1), b"x_stride"),
                     (dict(out_stride=INT32_MAX + 1), b"out_stride"), (dict(out_stride=-2), b"out_stride"),
                     (dict(C=30000, H=1000, W=1000), b"input image"),
                     (dict(C=512, H=2048, W=1024, n_images=2 ** 20, x_stride=0, out_stride=0), b"more than one launch holds")):
        assert call(**bad) == -1, bad
        err = l.mpnhip_last_error()
        assert POOL in err and msg in err, (bad, err)
    assert call(n_images=0) == 0
    assert call(n_images=0, x=None, out=None, C=0) == 0
    assert all(v == 0 for v in capi.path_counters().values())


def test_counter_names():
    names = list(capi.path_counters())
    assert "conv_affine_tile" in names and "maxpool" in names
    assert names[-2:] == ["conv_transpose_bwd", "layer_norm_bwd"]
    assert names.index("conv_affine_tile") < names.index("conv_affine_grouped") < names.index("conv_affine_small_grid") < names.index("conv_affine_wide") < names.index("maxpool") < names.index("conv_transpose_bwd")
