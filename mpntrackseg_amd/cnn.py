"""Host-side mirror of the reference's conv stacks of the mask branch
(``/root/reference/src/mot_neural_solver/models/cnn.py``): same constructor arguments and the same
``layers`` Sequential indices, so the reference's ``state_dict`` keys load.

``forward`` runs the stock PyTorch-ROCm (MIOpen) modules: training and everything that records gradients goes there by default.
``forward_native_autograd`` is the opt-in training route: the same native forward per Conv2d, recorded by autograd, its backward
one ``mpnhip_conv2d_backward`` call (csrc/conv_backward.hip); a ConvTranspose2d stays the stock module there unless
``transposed_native`` sends it through ``conv_transpose2d_native_autograd`` (``mpnhip_conv_transpose2d_backward``).
``layer_norm_native_autograd`` is the LayerNorm of MaskModel the same way (``mpnhip_layer_norm_backward``, csrc/conv.hip).
``forward_native`` is the no-grad inference forward through ``mpnhip_conv2d_forward`` (csrc/conv.hip): one native call per
(transposed) convolution with its bias and ReLU fused, the input given as a list of channel segments so that a ``torch.cat`` in
front of the stack is never materialised.  ``native_supported()`` says whether the stack is one the kernels cover."""
import ctypes as C

import torch
from torch import nn

from . import capi


def _check_lists(**kw):
    for name, v in kw.items():
        assert isinstance(v, (list, tuple)), '%s must be either a list or a tuple, but got %s' % (name, type(v))
    lens = {len(v) for v in kw.values()}
    assert len(lens) == 1, 'Number of elements mismatch between dims, kernel_sizes and strides'


def _image_dense(t):
    """[N, C, H, W] float32 whose images are dense [C][H][W] blocks at any image stride (a channel slice of a wider tensor is)."""
    n, c, h, w = t.shape
    if t.dtype != torch.float32:
        return False
    return t.numel() == 0 or ((w == 1 or t.stride(3) == 1) and (h == 1 or t.stride(2) == w) and (c == 1 or t.stride(1) == h * w))


def _segments(tensors):
    """The segment list of a native call: the tensors themselves where their images are dense, contiguous copies otherwise."""
    capi.require_device(*tensors)
    if not 1 <= len(tensors) <= capi.CONV_MAX_SEGMENTS:
        raise capi.MpnhipError("a native convolution takes 1 .. %d channel segments, not %d" % (capi.CONV_MAX_SEGMENTS, len(tensors)))
    segs = [t if _image_dense(t) else capi.f32c(t) for t in tensors]
    if any(s.dim() != 4 or s.shape[0] != segs[0].shape[0] or s.shape[2:] != segs[0].shape[2:] or s.device != segs[0].device
           for s in segs):
        raise capi.MpnhipError("channel segments must be [N, C_s, H, W] tensors of one N, H, W and device")
    return segs


def _out_tensor(out, shape, like):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if tuple(out.shape) != tuple(shape) or not out.is_cuda or out.device != like.device or not _image_dense(out):
        raise capi.MpnhipError("out must be a float32 %s device tensor with dense images (a channel slice is)" % (tuple(shape),))
    return out


def conv2d_native(segments, weight, bias, relu=False, transposed=False, out=None):
    """``mpnhip_conv2d_forward`` on the channel concatenation of ``segments``: Conv2d(k = 1 | 3, stride 1, padding k // 2) with
    ``weight`` [cout, cin, k, k], or ConvTranspose2d(2, stride 2) with ``weight`` [cin, cout, 2, 2].  No autograd."""
    segs = _segments(list(segments))
    w = capi.f32c(weight.detach())
    b = capi.f32c(bias.detach()) if bias is not None else None
    capi.require_device(w, b)
    n, _, h, wd = segs[0].shape
    cin = sum(int(s.shape[1]) for s in segs)
    cout = int(w.shape[1] if transposed else w.shape[0])
    if int(w.shape[0] if transposed else w.shape[1]) != cin or w.shape[2] != w.shape[3]:
        raise capi.MpnhipError("weight %s does not fit %d input channels" % (tuple(w.shape), cin))
    scale = 2 if transposed else 1
    y = _out_tensor(out, (n, cout, scale * h, scale * wd), segs[0])
    a = capi.ConvArgs()
    for i, s in enumerate(segs):
        a.seg_data[i], a.seg_stride[i], a.seg_channels[i] = s.data_ptr(), s.stride(0), int(s.shape[1])
    a.n_segments, a.H, a.W, a.cout, a.ksize, a.transposed, a.relu = len(segs), int(h), int(wd), cout, int(w.shape[2]), int(transposed), int(relu)
    a.n_images, a.weight, a.bias, a.out, a.out_stride = int(n), w.data_ptr(), (b.data_ptr() if b is not None else None), y.data_ptr(), y.stride(0)
    with torch.cuda.device(y.device):
        capi.check(capi.load().mpnhip_conv2d_forward(C.byref(a), capi.stream_ptr()), "mpnhip_conv2d_forward")
    return y


def conv2d_native_backward(segments, weight, y, grad_out, relu=False, need_input=True, need_weight=True, need_bias=True):
    """``mpnhip_conv2d_backward`` (csrc/conv_backward.hip) for Conv2d(k = 1 | 3, stride 1, padding k // 2) with its fused ReLU:
    ``(grad_in, grad_weight, grad_bias)``, None where ``need_*`` is false.  ``grad_in`` is ONE dense [N, cin, H, W] tensor over the
    channel concatenation of ``segments``; ``y``: the layer's output (read only with ``relu``, else it may be None)."""
    segs = _segments(list(segments))
    w = capi.f32c(weight.detach())
    capi.require_device(w, y, grad_out)
    n, _, h, wd = segs[0].shape
    cin = sum(int(s.shape[1]) for s in segs)
    cout = int(w.shape[0])
    if w.dim() != 4 or int(w.shape[1]) != cin or w.shape[2] != w.shape[3]:
        raise capi.MpnhipError("weight %s does not fit %d input channels" % (tuple(w.shape), cin))
    if tuple(grad_out.shape) != (n, cout, h, wd) or (relu and (y is None or tuple(y.shape) != (n, cout, h, wd))):
        raise capi.MpnhipError("grad_out (and y, with relu) must be [%d, %d, %d, %d]" % (n, cout, h, wd))
    go = grad_out if _image_dense(grad_out) else capi.f32c(grad_out)     # (an expanded scalar, as .sum().backward() hands over, is copied)
    yy = None if not relu else (y if _image_dense(y) else capi.f32c(y))
    dev = segs[0].device
    gi = torch.empty((n, cin, h, wd), dtype=torch.float32, device=dev) if need_input else None
    gw = torch.empty_like(w) if need_weight else None
    gb = torch.empty((cout,), dtype=torch.float32, device=dev) if need_bias else None
    a = capi.ConvBwdArgs()
    for i, s in enumerate(segs):
        a.seg_data[i], a.seg_stride[i], a.seg_channels[i] = s.data_ptr(), s.stride(0), int(s.shape[1])
    a.n_segments, a.H, a.W, a.cout, a.ksize, a.transposed, a.relu = len(segs), int(h), int(wd), cout, int(w.shape[2]), 0, int(relu)
    a.n_images, a.weight = int(n), w.data_ptr()
    a.y, a.y_stride = (yy.data_ptr(), yy.stride(0)) if yy is not None else (None, 0)
    a.grad_out, a.grad_out_stride = go.data_ptr(), go.stride(0)
    a.grad_in, a.grad_weight, a.grad_bias = (t.data_ptr() if t is not None else None for t in (gi, gw, gb))
    lib = capi.load()
    with torch.cuda.device(dev):
        ws = capi.workspace(lib.mpnhip_conv2d_backward_workspace_bytes(C.byref(a)), dev, "conv_bwd")
        capi.check(lib.mpnhip_conv2d_backward(C.byref(a), capi.ptr(ws), ws.numel(), capi.stream_ptr()), "mpnhip_conv2d_backward")
    return gi, gw, gb


class _Conv2dNative(torch.autograd.Function):
    """One Conv2d (+ fused ReLU) of the mask branch: ``conv2d_native`` forward, one ``mpnhip_conv2d_backward`` call backward."""

    @staticmethod
    def forward(ctx, weight, bias, relu, *segments):
        y = conv2d_native(segments, weight, bias, relu=relu)
        ctx.relu, ctx.has_bias, ctx.channels = bool(relu), bias is not None, [int(s.shape[1]) for s in segments]
        # the segments as the caller holds them (channel slices stay views of their tensors), the weight, and with relu the
        # output: y is this call's own allocation, never a view of a buffer a later step overwrites
        ctx.save_for_backward(weight, *(segments + ((y,) if relu else ())))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        weight, k = saved[0], len(ctx.channels)
        segments, y = saved[1:1 + k], (saved[1 + k] if ctx.relu else None)
        need = ctx.needs_input_grad
        need_input = any(need[3:])
        gi, gw, gb = conv2d_native_backward(segments, weight, y, grad_out, relu=ctx.relu, need_input=need_input, need_weight=need[0],
                                            need_bias=ctx.has_bias and need[1])
        grads, c0 = [], 0
        for i, c in enumerate(ctx.channels):
            grads.append(gi[:, c0:c0 + c] if need_input and need[3 + i] else None)
            c0 += c
        return (gw, gb, None) + tuple(grads)


def conv2d_native_autograd(segments, weight, bias, relu=False):
    """``conv2d_native`` (Conv2d only) as a ``torch.autograd.Function``: the gradients of the segments (channel slices of one
    dense ``grad_in``), of ``weight`` and of ``bias`` come from one ``mpnhip_conv2d_backward`` call that skips whatever
    ``needs_input_grad`` does not want.  It takes no ``out=``: a saved tensor must not alias a buffer that is written again."""
    segments = tuple(segments)
    capi.require_device(weight, bias, *segments)
    if not 1 <= len(segments) <= capi.CONV_MAX_SEGMENTS:
        raise capi.MpnhipError("a native convolution takes 1 .. %d channel segments, not %d" % (capi.CONV_MAX_SEGMENTS, len(segments)))
    return _Conv2dNative.apply(weight, bias, bool(relu), *segments)


def conv_transpose2d_native_backward(segments, weight, y, grad_out, relu=False, need_input=True, need_weight=True, need_bias=True):
    """``mpnhip_conv_transpose2d_backward`` (csrc/conv_backward.hip) for ConvTranspose2d(2, stride 2, padding 0) with its fused
    ReLU: ``(grad_in, grad_weight, grad_bias)``, None where ``need_*`` is false.  ``segments`` are [N, C_s, H, W], ``weight``
    [cin, cout, 2, 2], ``y`` (read only with ``relu``) and ``grad_out`` [N, cout, 2 H, 2 W]; ``grad_in`` is ONE dense
    [N, cin, H, W] tensor over the channel concatenation of ``segments``."""
    segs = _segments(list(segments))
    w = capi.f32c(weight.detach())
    capi.require_device(w, y, grad_out)
    n, _, h, wd = segs[0].shape
    cin = sum(int(s.shape[1]) for s in segs)
    if w.dim() != 4 or int(w.shape[0]) != cin or w.shape[2] != w.shape[3]:
        raise capi.MpnhipError("weight %s does not fit %d input channels" % (tuple(w.shape), cin))
    cout = int(w.shape[1])
    if tuple(grad_out.shape) != (n, cout, 2 * h, 2 * wd) or (relu and (y is None or tuple(y.shape) != (n, cout, 2 * h, 2 * wd))):
        raise capi.MpnhipError("grad_out (and y, with relu) must be [%d, %d, %d, %d]" % (n, cout, 2 * h, 2 * wd))
    go = grad_out if _image_dense(grad_out) else capi.f32c(grad_out)     # (an expanded scalar, as .sum().backward() hands over, is copied)
    yy = None if not relu else (y if _image_dense(y) else capi.f32c(y))
    dev = segs[0].device
    gi = torch.empty((n, cin, h, wd), dtype=torch.float32, device=dev) if need_input else None
    gw = torch.empty_like(w) if need_weight else None
    gb = torch.empty((cout,), dtype=torch.float32, device=dev) if need_bias else None
    a = capi.ConvBwdArgs()
    for i, s in enumerate(segs):
        a.seg_data[i], a.seg_stride[i], a.seg_channels[i] = s.data_ptr(), s.stride(0), int(s.shape[1])
    a.n_segments, a.H, a.W, a.cout, a.ksize, a.transposed, a.relu = len(segs), int(h), int(wd), cout, int(w.shape[2]), 1, int(relu)
    a.n_images, a.weight = int(n), w.data_ptr()
    a.y, a.y_stride = (yy.data_ptr(), yy.stride(0)) if yy is not None else (None, 0)
    a.grad_out, a.grad_out_stride = go.data_ptr(), go.stride(0)
    a.grad_in, a.grad_weight, a.grad_bias = (t.data_ptr() if t is not None else None for t in (gi, gw, gb))
    lib = capi.load()
    with torch.cuda.device(dev):
        ws = capi.workspace(lib.mpnhip_conv_transpose2d_backward_workspace_bytes(C.byref(a)), dev, "conv_bwd")
        capi.check(lib.mpnhip_conv_transpose2d_backward(C.byref(a), capi.ptr(ws), ws.numel(), capi.stream_ptr()),
                   "mpnhip_conv_transpose2d_backward")
    return gi, gw, gb


class _ConvTranspose2dNative(torch.autograd.Function):
    """One ConvTranspose2d(2, stride 2) (+ fused ReLU) of the mask branch: ``conv2d_native(transposed=True)`` forward, one
    ``mpnhip_conv_transpose2d_backward`` call backward."""

    @staticmethod
    def forward(ctx, weight, bias, relu, *segments):
        y = conv2d_native(segments, weight, bias, relu=relu, transposed=True)
        ctx.relu, ctx.has_bias, ctx.channels = bool(relu), bias is not None, [int(s.shape[1]) for s in segments]
        ctx.save_for_backward(weight, *(segments + ((y,) if relu else ())))     # (as _Conv2dNative)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        weight, k = saved[0], len(ctx.channels)
        segments, y = saved[1:1 + k], (saved[1 + k] if ctx.relu else None)
        need = ctx.needs_input_grad
        need_input = any(need[3:])
        gi, gw, gb = conv_transpose2d_native_backward(segments, weight, y, grad_out, relu=ctx.relu, need_input=need_input,
                                                      need_weight=need[0], need_bias=ctx.has_bias and need[1])
        grads, c0 = [], 0
        for i, c in enumerate(ctx.channels):
            grads.append(gi[:, c0:c0 + c] if need_input and need[3 + i] else None)
            c0 += c
        return (gw, gb, None) + tuple(grads)


def conv_transpose2d_native_autograd(segments, weight, bias, relu=False):
    """``conv2d_native(..., transposed=True)`` as a ``torch.autograd.Function``: the gradients of the segments (channel slices of
    one dense ``grad_in``), of ``weight`` and of ``bias`` come from one ``mpnhip_conv_transpose2d_backward`` call that skips
    whatever ``needs_input_grad`` does not want.  No ``out=``, as ``conv2d_native_autograd``."""
    segments = tuple(segments)
    capi.require_device(weight, bias, *segments)
    if not 1 <= len(segments) <= capi.CONV_MAX_SEGMENTS:
        raise capi.MpnhipError("a native convolution takes 1 .. %d channel segments, not %d" % (capi.CONV_MAX_SEGMENTS, len(segments)))
    return _ConvTranspose2dNative.apply(weight, bias, bool(relu), *segments)


def layer_norm_native_backward(segments, weight, eps, grad_out, need_input=True, need_weight=True, need_bias=True):
    """``mpnhip_layer_norm_backward`` (csrc/conv.hip): ``(grad_in, grad_weight, grad_bias)`` of ``layer_norm_native`` on the same
    ``segments``, None where ``need_*`` is false.  ``grad_in`` is ONE dense [N, C, H, W] tensor over the channel concatenation;
    ``weight`` None: no affine, ``grad_in`` only."""
    segs = _segments(list(segments))
    n, _, h, wd = segs[0].shape
    c = sum(int(s.shape[1]) for s in segs)
    w = capi.f32c(weight.detach()) if weight is not None else None
    capi.require_device(w, grad_out)
    if w is not None and w.numel() != c * h * wd:
        raise capi.MpnhipError("the LayerNorm affine must have the input's [%d, %d, %d] elements" % (c, h, wd))
    if w is None and (need_weight or need_bias):
        raise capi.MpnhipError("a LayerNorm without an affine has no weight or bias gradient")
    if tuple(grad_out.shape) != (n, c, h, wd):
        raise capi.MpnhipError("grad_out must be [%d, %d, %d, %d]" % (n, c, h, wd))
    go = grad_out if _image_dense(grad_out) else capi.f32c(grad_out)
    dev = segs[0].device
    gi = torch.empty((n, c, h, wd), dtype=torch.float32, device=dev) if need_input else None
    gw = torch.empty((c, h, wd), dtype=torch.float32, device=dev) if need_weight else None
    gb = torch.empty((c, h, wd), dtype=torch.float32, device=dev) if need_bias else None
    k = len(segs)
    data = (C.c_void_p * k)(*[s.data_ptr() for s in segs])
    stride = (C.c_int64 * k)(*[s.stride(0) for s in segs])
    chans = (C.c_int * k)(*[int(s.shape[1]) for s in segs])
    head = (data, stride, chans, k, int(n), int(h * wd), capi.ptr(w), float(eps), capi.ptr(go), go.stride(0), capi.ptr(gi), capi.ptr(gw),
            capi.ptr(gb))
    lib = capi.load()
    with torch.cuda.device(dev):
        ws = capi.workspace(lib.mpnhip_layer_norm_backward_workspace_bytes(*head), dev, "conv_bwd")
        capi.check(lib.mpnhip_layer_norm_backward(*(head + (capi.ptr(ws), ws.numel(), capi.stream_ptr()))), "mpnhip_layer_norm_backward")
    return gi, gw, gb


class _LayerNormNative(torch.autograd.Function):
    """``layer_norm_native`` forward on the segments as the caller holds them, one ``mpnhip_layer_norm_backward`` call backward."""

    @staticmethod
    def forward(ctx, weight, bias, eps, *segments):
        y = layer_norm_native(segments, weight, bias, eps)
        ctx.eps, ctx.affine, ctx.channels = float(eps), weight is not None, [int(s.shape[1]) for s in segments]
        ctx.save_for_backward(*(((weight,) if weight is not None else ()) + segments))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        weight, segments = (saved[0], saved[1:]) if ctx.affine else (None, saved)
        need = ctx.needs_input_grad
        need_input = any(need[3:])
        if not (need_input or (ctx.affine and (need[0] or need[1]))):
            return (None,) * (3 + len(ctx.channels))
        gi, gw, gb = layer_norm_native_backward(segments, weight, ctx.eps, grad_out, need_input=need_input,
                                                need_weight=ctx.affine and need[0], need_bias=ctx.affine and need[1])
        grads, c0 = [], 0
        for i, c in enumerate(ctx.channels):
            grads.append(gi[:, c0:c0 + c] if need_input and need[3 + i] else None)
            c0 += c
        shape = weight.shape if ctx.affine else None
        return (gw.view(shape) if gw is not None else None, gb.view(shape) if gb is not None else None, None) + tuple(grads)


def layer_norm_native_autograd(segments, weight, bias, eps):
    """``layer_norm_native`` as a ``torch.autograd.Function``.  The segments are read where they are (no ``torch.cat``); their
    gradients are channel slices of one dense ``grad_in``, those of ``weight`` / ``bias`` (both or neither) have their shape."""
    segments = tuple(segments)
    capi.require_device(weight, bias, *segments)
    if not 1 <= len(segments) <= capi.CONV_MAX_SEGMENTS:
        raise capi.MpnhipError("a native LayerNorm takes 1 .. %d channel segments, not %d" % (capi.CONV_MAX_SEGMENTS, len(segments)))
    if (weight is None) != (bias is None):
        raise capi.MpnhipError("the LayerNorm affine needs weight and bias, or neither")
    return _LayerNormNative.apply(weight, bias, float(eps), *segments)


def layer_norm_native(segments, weight, bias, eps, out=None):
    """``mpnhip_layer_norm_forward``: nn.LayerNorm over the trailing [C, H, W] of the channel concatenation of ``segments``."""
    segs = _segments(list(segments))
    n, _, h, wd = segs[0].shape
    c = sum(int(s.shape[1]) for s in segs)
    w = capi.f32c(weight.detach()) if weight is not None else None
    b = capi.f32c(bias.detach()) if bias is not None else None
    capi.require_device(w, b)
    if w is not None and (b is None or w.numel() != c * h * wd or b.numel() != w.numel()):
        raise capi.MpnhipError("the LayerNorm affine must have the input's [%d, %d, %d] elements" % (c, h, wd))
    y = _out_tensor(out, (n, c, h, wd), segs[0])
    k = len(segs)
    data = (C.c_void_p * k)(*[s.data_ptr() for s in segs])
    stride = (C.c_int64 * k)(*[s.stride(0) for s in segs])
    chans = (C.c_int * k)(*[int(s.shape[1]) for s in segs])
    with torch.cuda.device(y.device):
        capi.check(capi.load().mpnhip_layer_norm_forward(data, stride, chans, k, int(n), int(h * wd), capi.ptr(w), capi.ptr(b), float(eps),
                                                         capi.ptr(y), y.stride(0), capi.stream_ptr()), "mpnhip_layer_norm_forward")
    return y


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _conv_native_supported(m):
    if m.weight.dtype != torch.float32 or _pair(m.dilation) != (1, 1) or m.groups != 1:
        return False
    k, st, pad = _pair(m.kernel_size), _pair(m.stride), _pair(m.padding)
    if isinstance(m, nn.ConvTranspose2d):
        return k == (2, 2) and st == (2, 2) and pad == (0, 0) and _pair(m.output_padding) == (0, 0)
    return k in ((1, 1), (3, 3)) and st == (1, 1) and pad == (k[0] // 2, k[0] // 2) and m.padding_mode == 'zeros'


def _layers_native_supported(layers):
    """The predicate of ``native_supported`` on a ``layers`` Sequential."""
    for m in layers:
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            if not _conv_native_supported(m):
                return False
        elif isinstance(m, (nn.Dropout, nn.Dropout2d)):
            if m.p != 0 and m.training:
                return False
        elif not isinstance(m, nn.ReLU):
            return False       # BatchNorm2d and anything else the kernels do not cover
    return True


def _layers_forward_native(layers, segments, out):
    """One native call per convolution of ``layers``, the ReLU that follows it fused; ``out``: where the LAST one writes."""
    mods = list(layers)
    convs = [i for i, m in enumerate(mods) if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]
    if not convs:
        raise capi.MpnhipError("forward_native: the stack has no convolution")
    x = list(segments)
    for i in convs:
        m = mods[i]
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
        y = conv2d_native(x, m.weight, m.bias, relu=relu, transposed=isinstance(m, nn.ConvTranspose2d),
                          out=out if i == convs[-1] else None)
        x = [y]
    return x[0]


def _layers_forward_native_autograd(layers, segments, transposed_native=False):
    """``_layers_forward_native`` with gradients: every Conv2d through ``conv2d_native_autograd`` with its ReLU fused.  A
    ConvTranspose2d (and the ReLU behind it) runs as the stock modules on the materialised tensor, or, with ``transposed_native``,
    through ``conv_transpose2d_native_autograd`` with that ReLU fused."""
    mods = list(layers)
    if not any(isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) for m in mods):
        raise capi.MpnhipError("forward_native_autograd: the stack has no convolution")
    x = list(segments)
    for i, m in enumerate(mods):
        if not isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            continue
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
        if isinstance(m, nn.ConvTranspose2d) and transposed_native:
            x = [conv_transpose2d_native_autograd(x, m.weight, m.bias, relu=relu)]
        elif isinstance(m, nn.ConvTranspose2d):              # the stock modules, the ReLU behind it included
            y = m(x[0] if len(x) == 1 else torch.cat(x, dim=1))
            x = [mods[i + 1](y) if relu else y]
        else:
            x = [conv2d_native_autograd(x, m.weight, m.bias, relu=relu)]
    return x[0]


class CNN(nn.Module):
    """cnn.py:4-44: Conv2d (+BatchNorm2d) + ReLU (+Dropout2d) per entry of ``dims``."""

    def __init__(self, input_dim, dims, kernel_sizes, strides, paddings, dropout_p=0.4, use_batchnorm=False):
        super(CNN, self).__init__()
        _check_lists(dims=dims, kernel_sizes=kernel_sizes, strides=strides, paddings=paddings)
        mods = []
        c_in = input_dim
        for c_out, k, st, pad in zip(dims, kernel_sizes, strides, paddings):
            mods.append(nn.Conv2d(c_in, c_out, kernel_size=k, stride=st, padding=pad))
            if use_batchnorm and c_out != 1:
                mods.append(nn.BatchNorm2d(c_out))
            if c_out != 0:
                mods.append(nn.ReLU(inplace=True))
            if dropout_p != 0 and c_out != 1:
                mods.append(nn.Dropout2d(p=dropout_p))
            c_in = c_out
        self.layers = nn.Sequential(*mods)

    def forward(self, input):
        return self.layers(input)

    def native_supported(self):
        """Whether ``forward_native`` covers this stack: every convolution has stride 1 and kernel 1 or 3 with padding k // 2, there
        is no BatchNorm, and Dropout is off (p = 0 or eval mode)."""
        return _layers_native_supported(self.layers)

    def forward_native(self, segments, out=None):
        """Inference forward (no autograd) on the channel concatenation of ``segments`` (a list of [N, C_s, H, W] device tensors,
        channel slices allowed); the last convolution writes into ``out`` when given (it may be a channel slice too)."""
        if not self.native_supported():
            raise capi.MpnhipError("this CNN is not covered by the native convolutions (see native_supported)")
        return _layers_forward_native(self.layers, segments, out)

    def forward_native_autograd(self, segments):
        """``forward_native`` for training: the same native forward, recorded by autograd, the backward of every Conv2d one
        ``mpnhip_conv2d_backward`` call (``conv2d_native_autograd``).  No ``out=``: the outputs are saved for the backward."""
        if not self.native_supported():
            raise capi.MpnhipError("this CNN is not covered by the native convolutions (see native_supported)")
        return _layers_forward_native_autograd(self.layers, segments)


class MaskRCNNPredictor(nn.Module):
    """cnn.py:47-84: (transposed) convolutions with a ReLU after every layer but the last."""

    def __init__(self, input_dim, dims, kernel_sizes, strides, paddings, transposed):
        super(MaskRCNNPredictor, self).__init__()
        _check_lists(dims=dims, kernel_sizes=kernel_sizes, strides=strides, paddings=paddings)
        mods = []
        c_in = input_dim
        n = len(dims)
        for i, (c_out, k, st, pad) in enumerate(zip(dims, kernel_sizes, strides, paddings)):
            conv = nn.ConvTranspose2d if transposed[i] else nn.Conv2d
            mods.append(conv(c_in, c_out, kernel_size=k, stride=st, padding=pad))
            if i < n - 1:
                mods.append(nn.ReLU(inplace=True))
            c_in = c_out
        self.layers = nn.Sequential(*mods)

    def forward(self, input):
        return self.layers(input)

    def native_supported(self):
        """As ``CNN.native_supported``; a transposed convolution must have kernel 2, stride 2, padding 0."""
        return _layers_native_supported(self.layers)

    def forward_native(self, segments, out=None):
        """As ``CNN.forward_native``."""
        if not self.native_supported():
            raise capi.MpnhipError("this MaskRCNNPredictor is not covered by the native convolutions (see native_supported)")
        return _layers_forward_native(self.layers, segments, out)

    def forward_native_autograd(self, segments, transposed_native=False):
        """As ``CNN.forward_native_autograd``; a transposed convolution runs as the stock module, or with ``transposed_native``
        through ``conv_transpose2d_native_autograd`` (backward: ``mpnhip_conv_transpose2d_backward``)."""
        if not self.native_supported():
            raise capi.MpnhipError("this MaskRCNNPredictor is not covered by the native convolutions (see native_supported)")
        return _layers_forward_native_autograd(self.layers, segments, transposed_native=transposed_native)
