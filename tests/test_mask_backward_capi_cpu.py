"""The host side of mpnhip_conv_transpose2d_backward and mpnhip_layer_norm_backward without a GPU: the symbols, every refusal
(all of them return before a kernel is launched: the non-null pointers are host dummies that are never followed), the workspace
size queries against the layout include/mpnhip.h documents, the two path counters, and the ``mask_conv_grads = 'native_all'``
selector on a CPU model (the stock fall-back)."""
import ctypes

import pytest
import torch

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.mpn import MOTMPNet

INT32_MAX = 2 ** 31 - 1
BIG = 1 << 40        # a workspace size no layout below reaches (the buffer is never touched)
up = lambda floats: (4 * floats + 255) // 256 * 256     # a region: floats, padded to 256 bytes


@pytest.fixture(scope="module")
def dummy():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.cast(buf, ctypes.c_void_p).value


def test_symbols_exist():
    l = capi.load()
    for name in ("mpnhip_conv_transpose2d_backward", "mpnhip_conv_transpose2d_backward_workspace_bytes", "mpnhip_layer_norm_backward",
                 "mpnhip_layer_norm_backward_workspace_bytes"):
        assert name in capi.SIGNATURES and getattr(l, name) is not None


def test_counters_exist_at_the_end():
    names = list(capi.path_counters())
    assert names[-2:] == ["conv_transpose_bwd", "layer_norm_bwd"]
    assert {"conv_transpose", "layer_norm", "conv_bwd_gate", "conv_wgrad", "conv_wgrad_plain"} <= set(names)


# ------------------------------------------------------------------------------------ ConvTranspose2d backward
def convt_args(p, **kw):
    """ConvTranspose2d(64 -> 32, 2, stride 2) on two segments of 32 channels at 14 x 14, N = 3, with the ReLU."""
    a = capi.ConvBwdArgs()
    a.n_segments, a.H, a.W, a.cout, a.ksize, a.transposed, a.n_images, a.relu = 2, 14, 14, 32, 2, 1, 3, 1
    for i in range(2):
        a.seg_data[i], a.seg_stride[i], a.seg_channels[i] = p, 32 * 196, 32
    a.weight, a.y, a.grad_out, a.grad_in, a.grad_weight, a.grad_bias = p, p, p, p, p, p
    a.y_stride = a.grad_out_stride = 32 * 4 * 196
    for k, v in kw.items():
        if isinstance(v, tuple):     # (index, value) of one of the three segment lists
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def test_conv_transpose2d_backward_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy
    assert l.mpnhip_conv_transpose2d_backward(None, p, BIG, None) == -1
    assert b"mpnhip_conv_transpose2d_backward: null args" in l.mpnhip_last_error()
    assert l.mpnhip_conv_transpose2d_backward_workspace_bytes(None) == 0
    bad_cases = [
        (dict(transposed=0), b"transposed"), (dict(transposed=0, ksize=3), b"transposed"),
        (dict(ksize=1), b"kernel size"), (dict(ksize=3), b"kernel size"), (dict(ksize=0), b"kernel size"),
        (dict(y=None), b"relu needs"), (dict(grad_out=None), b"null grad_out"),
        (dict(grad_in=None, grad_weight=None, grad_bias=None), b"no output wanted"),
        (dict(grad_out_stride=INT32_MAX + 1), b"grad_out_stride"), (dict(grad_out_stride=-5), b"grad_out_stride"),
        (dict(y_stride=INT32_MAX + 1), b"y_stride"), (dict(y_stride=-1), b"y_stride"),
        (dict(seg_stride=(0, INT32_MAX + 1)), b"segment 0: image stride"), (dict(seg_stride=(1, -1)), b"segment 1: image stride"),
        # what the forward refuses
        (dict(n_images=-1), b"n_images"), (dict(seg_data=(1, None)), b"segment 1: null pointer"), (dict(weight=None), b"null weight"),
        (dict(n_segments=5), b"n_segments"), (dict(n_segments=0), b"n_segments"),
        (dict(seg_channels=(0, 0)), b"segment 0: 0 channels"),
        (dict(H=0), b"must be positive"), (dict(W=-2), b"must be positive"), (dict(cout=0), b"must be positive"),
        (dict(H=50000, W=50000), b"input image"),
        (dict(H=4096, W=4096, cout=64), b"output image"),            # 4 cout H W floats per output image
        (dict(seg_channels=(0, 30000), seg_stride=(0, 0), H=1, W=1, cout=30000), b"weight"),
        (dict(n_images=1 << 40, H=1, W=1), b"more than one launch holds"),
    ]
    for bad, msg in bad_cases:
        a = convt_args(p, **bad)
        assert l.mpnhip_conv_transpose2d_backward(ctypes.byref(a), p, BIG, None) == -1, bad
        err = l.mpnhip_last_error()
        assert b"mpnhip_conv_transpose2d_backward" in err and msg in err, (bad, err)
        assert l.mpnhip_conv_transpose2d_backward_workspace_bytes(ctypes.byref(a)) == 0, bad
    # y is not looked at without a ReLU (that call gets as far as the workspace check)
    a = convt_args(p, relu=0, y=None)
    need = l.mpnhip_conv_transpose2d_backward_workspace_bytes(ctypes.byref(a))
    assert need > 0
    # the workspace: null, or smaller than the size query says
    for ws, nbytes in ((None, BIG), (p, need - 1), (p, 0)):
        assert l.mpnhip_conv_transpose2d_backward(ctypes.byref(a), ws, nbytes, None) == -1
        assert b"mpnhip_conv_transpose2d_backward: workspace" in l.mpnhip_last_error()


def test_conv_transpose2d_backward_workspace_layout(dummy):
    """g' [N][4 cout][hw], the gathered input [N][cin][hw] with more than one segment only, the weight partial sums
    [splits][cin][4 cout], the bias partial sums [splits][cout]; 8 images per split."""
    l = capi.load()
    _, p = dummy
    for n in (1, 8, 9, 280):
        splits = (n + 7) // 8
        got = l.mpnhip_conv_transpose2d_backward_workspace_bytes(ctypes.byref(convt_args(p, n_images=n)))
        assert got == up(n * 128 * 196) + up(n * 64 * 196) + up(splits * 64 * 128) + up(splits * 32), n
        one = convt_args(p, n_images=n, n_segments=1, seg_channels=(0, 64))
        got = l.mpnhip_conv_transpose2d_backward_workspace_bytes(ctypes.byref(one))
        assert got == up(n * 128 * 196) + up(splits * 64 * 128) + up(splits * 32), n
        # the size does not depend on which outputs are wanted
        assert got == l.mpnhip_conv_transpose2d_backward_workspace_bytes(ctypes.byref(
            convt_args(p, n_images=n, n_segments=1, seg_channels=(0, 64), grad_in=None, grad_bias=None)))


def test_conv_transpose2d_backward_without_images_succeeds(dummy):
    l = capi.load()
    _, p = dummy
    a = convt_args(p, n_images=0, grad_weight=None, grad_bias=None)
    assert l.mpnhip_conv_transpose2d_backward_workspace_bytes(ctypes.byref(a)) == 0
    assert l.mpnhip_conv_transpose2d_backward(ctypes.byref(a), None, 0, None) == 0
    assert l.mpnhip_conv_transpose2d_backward(ctypes.byref(convt_args(p, n_images=0, grad_weight=None, grad_bias=None, ksize=3)), None, 0,
                                              None) == -1


# ------------------------------------------------------------------------------------ LayerNorm backward
def ln_call(p, ws=None, ws_bytes=BIG, size_only=False, **kw):
    """LayerNorm over two segments of 32 channels at hw = 196, N = 3, with an affine; every pointer is the dummy ``p``."""
    a = dict(n_segments=2, n_images=3, hw=196, weight=p, eps=1e-5, grad_out=p, grad_out_stride=64 * 196, grad_in=p, grad_weight=p,
             grad_bias=p, data=[p, p, p, p], stride=[32 * 196] * 4, channels=[32, 32, 32, 32], lists=True)
    a.update(kw)
    k = 4
    data = (ctypes.c_void_p * k)(*a["data"]) if a["lists"] else None
    stride = (ctypes.c_int64 * k)(*a["stride"]) if a["lists"] else None
    chans = (ctypes.c_int * k)(*a["channels"]) if a["lists"] else None
    head = (data, stride, chans, a["n_segments"], a["n_images"], a["hw"], a["weight"], a["eps"], a["grad_out"], a["grad_out_stride"],
            a["grad_in"], a["grad_weight"], a["grad_bias"])
    l = capi.load()
    if size_only:
        return l.mpnhip_layer_norm_backward_workspace_bytes(*head)
    return l.mpnhip_layer_norm_backward(*(head + (ws if ws is not None else None, ws_bytes, None)))


def test_layer_norm_backward_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy
    bad_cases = [
        (dict(n_segments=0), b"n_segments"), (dict(n_segments=5), b"n_segments"), (dict(n_segments=-1), b"n_segments"),
        (dict(hw=0), b"hw"), (dict(hw=-3), b"hw"), (dict(hw=INT32_MAX + 1), b"hw"),
        (dict(eps=-1e-5), b"eps"), (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps"),
        (dict(weight=None), b"without a weight"), (dict(weight=None, grad_bias=None), b"without a weight"),
        (dict(weight=None, grad_weight=None), b"without a weight"),
        (dict(grad_out=None), b"null grad_out"),
        (dict(grad_in=None, grad_weight=None, grad_bias=None), b"no output wanted"),
        (dict(grad_out_stride=INT32_MAX + 1), b"grad_out_stride"), (dict(grad_out_stride=-1), b"grad_out_stride"),
        (dict(stride=[INT32_MAX + 1] * 4), b"segment 0: image stride"), (dict(stride=[0, -1, 0, 0]), b"segment 1: image stride"),
        (dict(data=[p, None, p, p]), b"segment 1: null pointer"), (dict(channels=[0, 32, 32, 32]), b"segment 0: 0 channels"),
        (dict(hw=1 << 20, channels=[4096] * 4), b"input image"),
        (dict(n_images=-1), b"n_images"), (dict(n_images=1 << 40), b"more than one launch holds"),
        (dict(lists=False), b"null segment lists"),
    ]
    for bad, msg in bad_cases:
        assert ln_call(p, ws=p, **bad) == -1, bad
        err = l.mpnhip_last_error()
        assert b"mpnhip_layer_norm_backward" in err and msg in err, (bad, err)
        assert ln_call(p, size_only=True, **bad) == 0, bad
    # no affine and grad_in alone is a call (it gets as far as the workspace check)
    need = ln_call(p, size_only=True, weight=None, grad_weight=None, grad_bias=None)
    assert need > 0
    for ws, nbytes in ((None, BIG), (p, need - 1), (p, 0)):
        assert ln_call(p, ws=ws, ws_bytes=nbytes, weight=None, grad_weight=None, grad_bias=None) == -1
        assert b"mpnhip_layer_norm_backward: workspace" in l.mpnhip_last_error()


def test_layer_norm_backward_workspace_layout(dummy):
    """(mean, rstd) [N][2]; with an affine the two partial-sum regions [splits][C hw] each; 8 images per split."""
    _, p = dummy
    feat = 64 * 196
    for n in (1, 8, 9, 280):
        splits = (n + 7) // 8
        assert ln_call(p, size_only=True, n_images=n) == up(2 * n) + 2 * up(splits * feat), n
        assert ln_call(p, size_only=True, n_images=n, grad_in=None, grad_bias=None) == up(2 * n) + 2 * up(splits * feat), n
        assert ln_call(p, size_only=True, n_images=n, weight=None, grad_weight=None, grad_bias=None) == up(2 * n), n


def test_layer_norm_backward_without_images_succeeds(dummy):
    _, p = dummy
    assert ln_call(p, size_only=True, n_images=0, grad_weight=None, grad_bias=None) == 0
    assert ln_call(p, ws=None, ws_bytes=0, n_images=0, grad_weight=None, grad_bias=None) == 0
    assert ln_call(p, ws=None, ws_bytes=0, n_images=0, grad_weight=None, grad_bias=None, hw=0) == -1


# ------------------------------------------------------------------------------------ the selector
def test_native_all_on_a_cpu_model_takes_the_stock_fallback():
    """Tensors that are not on a device: 'native_all' falls back to the stock modules, silently, as 'native' does.  L = 0, where
    the branch is the encoder and the mask predictor alone: the attention aggregation of a step has no CPU form."""
    params = synth.model_params(32, 0, "sum", num_class_steps=0, node_in_dim=64)
    params.update(synth.MASK_PARAMS)
    model = MOTMPNet(params).train()
    assert model.mask_conv_grads == 'stock'
    x_ext = torch.from_numpy(synth.normal(8, (3, 256, 14, 14), stream=1, std=0.5))
    ei = torch.tensor([[0, 0, 1, 1], [1, 2, 2, 0]], dtype=torch.int64)
    logits = torch.zeros(1, 4, requires_grad=True)
    model.mask_conv_grads = 'native_all'
    preds = model.mask_predictions(x_ext, ei, logits)
    assert len(preds) == 1 and tuple(preds[0].shape) == (3, 1, 56, 56)
    preds[0].sum().backward()
    assert all(p.grad is not None for p in model.mask_predictor.parameters())
    model.mask_conv_grads = 'fast'
    with pytest.raises(capi.MpnhipError, match="mask_conv_grads"):
        model.mask_predictions(x_ext, ei, logits)
    with pytest.raises(capi.MpnhipError, match="native_all"):
        model.mask_predictions(x_ext, ei, logits)
