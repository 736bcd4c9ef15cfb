"""The host side of the native mask-branch layers, without a GPU: the ctypes image of mpnhip_conv_args against the header, the
argument checks of mpnhip_conv2d_forward / mpnhip_layer_norm_forward (everything below returns before a kernel is launched: the
non-null pointers are host dummies that are never followed), and the ``native_supported`` predicates."""
import copy
import ctypes
import os
import re

import pytest

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.cnn import CNN, MaskRCNNPredictor
from mpntrackseg_amd.mpn import MaskModel, MOTMPNet

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1


def test_conv_args_layout_matches_c():
    # mpnhip_conv_args: 4 pointers, 4 int64, 4 ints, 7 ints (+ 4 bytes of padding), int64, 3 pointers, int64
    A = capi.ConvArgs
    assert ctypes.sizeof(A) == 4 * 8 + 4 * 8 + 4 * 4 + 7 * 4 + 4 + 8 + 3 * 8 + 8 == 152
    offsets = dict(seg_data=0, seg_stride=32, seg_channels=64, n_segments=80, H=84, W=88, cout=92, ksize=96, transposed=100, relu=104,
                   n_images=112, weight=120, bias=128, out=136, out_stride=144)
    assert [f[0] for f in A._fields_] == list(offsets)
    for name, off in offsets.items():
        assert getattr(A, name).offset == off, name
    # the header declares the fields in the same order, the three lists with MPNHIP_CONV_MAX_SEGMENTS entries
    src = open(os.path.join(REPO, "include", "mpnhip.h")).read()
    body = re.search(r"typedef struct mpnhip_conv_args \{(.*?)\} mpnhip_conv_args;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[4\])?;", body) == list(offsets)
    assert re.findall(r"(\w+)\[4\];", body) == ["seg_data", "seg_stride", "seg_channels"]
    assert int(re.search(r"#define MPNHIP_CONV_MAX_SEGMENTS (\d+)", src).group(1)) == capi.CONV_MAX_SEGMENTS == 4


@pytest.fixture(scope="module")
def dummy():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.cast(buf, ctypes.c_void_p).value


def conv_args(p, **kw):
    a = capi.ConvArgs()
    a.n_segments, a.H, a.W, a.cout, a.ksize, a.n_images = 2, 14, 14, 32, 3, 3
    for i in range(2):
        a.seg_data[i], a.seg_stride[i], a.seg_channels[i] = p, 32 * 196, 32
    a.weight, a.bias, a.out, a.out_stride = p, p, p, 32 * 196
    for k, v in kw.items():
        if isinstance(v, tuple):     # (index, value) of one of the three segment lists
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def test_conv2d_forward_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy
    assert l.mpnhip_conv2d_forward(None, None) == -1
    assert b"mpnhip_conv2d_forward: null args" in l.mpnhip_last_error()
    bad_cases = [
        (dict(n_images=-1), b"n_images"),
        (dict(seg_data=(1, None)), b"segment 1: null pointer"), (dict(weight=None), b"null weight or out"), (dict(out=None), b"null weight or out"),
        (dict(ksize=2), b"kernel size"), (dict(ksize=5), b"kernel size"), (dict(ksize=0), b"kernel size"),
        (dict(transposed=1, ksize=3), b"transposed"), (dict(transposed=1, ksize=1), b"transposed"),
        (dict(n_segments=5), b"n_segments"), (dict(n_segments=0), b"n_segments"), (dict(n_segments=-1), b"n_segments"),
        (dict(seg_channels=(0, 0)), b"segment 0: 0 channels"), (dict(seg_channels=(1, -3)), b"segment 1: -3 channels"),
        (dict(H=0), b"must be positive"), (dict(W=-2), b"must be positive"), (dict(cout=0), b"must be positive"),
        (dict(seg_stride=(0, INT32_MAX + 1)), b"segment 0: image stride"), (dict(seg_stride=(1, -1)), b"segment 1: image stride"),
        (dict(out_stride=INT32_MAX + 1), b"out_stride"), (dict(out_stride=-5), b"out_stride"),
        (dict(H=50000, W=50000), b"input image"),                           # 64 channels x 2.5e9 pixels
        (dict(H=4096, W=4096, seg_channels=(0, 64), seg_stride=(0, 0), cout=200), b"output image"),   # the input fits, the output does not
        (dict(transposed=1, ksize=2, H=2048, W=2048, seg_channels=(0, 64), seg_stride=(0, 0), cout=200), b"output image"),   # only x 4
        (dict(seg_channels=(0, 30000), seg_stride=(0, 0), H=1, W=1, cout=30000), b"weight"),
    ]
    for bad, msg in bad_cases:
        assert l.mpnhip_conv2d_forward(ctypes.byref(conv_args(p, **bad)), None) == -1, bad
        err = l.mpnhip_last_error()
        assert b"mpnhip_conv2d_forward" in err and msg in err, (bad, err)
    # no images: a successful no-op whatever else the struct holds
    assert l.mpnhip_conv2d_forward(ctypes.byref(conv_args(p, n_images=0)), None) == 0
    assert l.mpnhip_conv2d_forward(ctypes.byref(conv_args(p, n_images=0, weight=None, out=None, ksize=7, n_segments=9)), None) == 0


def test_layer_norm_forward_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy

    def call(n_images=3, k=2, data=(p, p), stride=(6272, 6272), chans=(32, 32), hw=196, weight=p, bias=p, eps=1e-5, out=p, out_stride=12544,
             lists=True):
        d = (ctypes.c_void_p * 4)(*data) if lists else None
        s = (ctypes.c_int64 * 4)(*stride)
        c = (ctypes.c_int * 4)(*chans)
        return l.mpnhip_layer_norm_forward(d, s, c, k, n_images, hw, weight, bias, ctypes.c_float(eps), out, out_stride, None)

    for bad, msg in ((dict(n_images=-1), b"n_images"), (dict(lists=False), b"null segment lists"), (dict(k=0), b"n_segments"),
                     (dict(k=5), b"n_segments"), (dict(data=(p, None)), b"segment 1: null pointer"), (dict(chans=(32, 0)), b"segment 1: 0 channels"),
                     (dict(hw=0), b"hw"), (dict(hw=INT32_MAX + 1), b"hw"), (dict(eps=-1.0), b"eps"), (dict(eps=float("nan")), b"eps"),
                     (dict(out=None), b"null out"), (dict(bias=None), b"both"), (dict(weight=None), b"both"),
                     (dict(stride=(INT32_MAX + 1, 0)), b"image stride"), (dict(out_stride=INT32_MAX + 1), b"out_stride"),
                     (dict(chans=(30000, 30000), hw=100000), b"input image")):
        assert call(**bad) == -1, bad
        err = l.mpnhip_last_error()
        assert b"mpnhip_layer_norm_forward" in err and msg in err, (bad, err)
    assert call(n_images=0) == 0
    assert call(n_images=0, lists=False, out=None, k=0) == 0


def cnn_cfg(**kw):
    cfg = copy.deepcopy(synth.MASK_PARAMS["node_ext_model_feats_dict"])
    cfg.update(kw)
    return cfg


def test_native_supported_predicates():
    # the shipped configuration: every stack of the mask branch is covered
    for name in ("node_ext_encoder_feats_dict", "node_ext_model_feats_dict"):
        cfg = dict(synth.MASK_PARAMS[name])
        cfg.setdefault("input_dim", 192)
        assert CNN(**cfg).native_supported(), name
    mm = MaskModel(synth.MASK_PARAMS["mask_model_feats_dict"])
    assert mm.feature_encoder.native_supported() and mm.mask_head.native_supported() and mm.mask_predictor.native_supported()
    assert mm.native_supported()
    params = synth.model_params(32, 2, "sum", num_class_steps=2, node_in_dim=64)
    params.update(synth.MASK_PARAMS)
    model = MOTMPNet(params)
    assert model.mask_convs == 'stock'
    assert all(m.native_supported() for m in model._mask_modules())
    # stride 2, a kernel the tile kernel does not have, padding other than k // 2
    assert not CNN(input_dim=192, **cnn_cfg(strides=[2, 1])).native_supported()
    assert not CNN(input_dim=192, **cnn_cfg(kernel_sizes=[5, 3], paddings=[2, 1])).native_supported()
    assert not CNN(input_dim=192, **cnn_cfg(paddings=[0, 1])).native_supported()
    assert not CNN(input_dim=192, **cnn_cfg(kernel_sizes=[1, 3], paddings=[1, 1])).native_supported()
    # BatchNorm, in any mode
    bn = CNN(input_dim=192, **cnn_cfg(use_batchnorm=True))
    assert not bn.native_supported() and not bn.eval().native_supported()
    # Dropout: off in eval mode, on in training mode; p = 0 builds no Dropout at all
    dr = CNN(input_dim=192, **cnn_cfg(dropout_p=0.4))
    assert dr.training and not dr.native_supported()
    assert dr.eval().native_supported()
    assert CNN(input_dim=192, **cnn_cfg(dropout_p=0)).train().native_supported()
    # the predictor: a transposed convolution must be 2 x 2 / stride 2 / padding 0
    pred = synth.MASK_PARAMS["mask_model_feats_dict"]["mask_predictor_feats_dict"]
    assert MaskRCNNPredictor(**pred).native_supported()
    assert not MaskRCNNPredictor(**dict(pred, kernel_sizes=[4, 3, 2, 1], paddings=[1, 1, 0, 0])).native_supported()
    assert not MaskRCNNPredictor(**dict(pred, strides=[1, 1, 2, 1])).native_supported()
    # an unsupported stack refuses forward_native before it looks at its input
    with pytest.raises(capi.MpnhipError):
        bn.forward_native([])
