"""The host side of csrc/conv_strided.hip, shared by the networks built on it (``reid_net``, ``fpn_net``, ``rcnn_heads``): the
single-launch operators, the BatchNorm folds, the ResNet ``Bottleneck`` with its layer walk, and the launch plan of a ResNet body
with the executor that runs it.

A plan is a list of ``Launch`` and ``Stage`` records over named buffers; ``resnet_body_steps`` builds the body's part under the
one buffer rule stated there, a network appends what is its own, and ``run_steps`` issues the launches of one slice of the batch
-- the same entry points with the same arguments in the same order whichever network the plan belongs to."""
import ctypes as C
from typing import Any, NamedTuple, Optional, Tuple

import torch
from torch import nn

from . import capi
from .capi import MpnhipError
from .cnn import _image_dense, _out_tensor


# ------------------------------------------------------------------------------------------------ operators
def _conv_out(size, stride):
    return (int(size) - 1) // int(stride) + 1


def _dense_input(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise MpnhipError("%s must be a float32 [N, C, H, W] device tensor" % what)
    capi.require_device(x)
    return x if _image_dense(x) else capi.f32c(x)


def _vec(t, n, like, what):
    if t is None:
        return None
    t = capi.f32c(t.detach())
    capi.require_device(t)
    if t.numel() != n or t.device != like.device:
        raise MpnhipError("%s must hold %d floats on %s" % (what, n, like.device))
    return t


def fill_conv_args(a, x, x_stride, weight, scale, shift, residual, residual_stride, relu, out, out_stride, n_images, geometry, up=None):
    """Fills ``a``, a ``capi.ConvAffineArgs`` or (``up`` given) a ``capi.ConvAffineUpArgs``, which is the former plus the
    residual's size ``up = (rh, rw)``.  ``x``, ``residual`` (or None) and ``out`` are addresses; ``weight``, ``scale`` and
    ``shift`` tensors (the last two or None); ``geometry = (cin, cout, H, W, ksize, stride)``."""
    a.x, a.x_stride, a.weight = x, x_stride, weight.data_ptr()
    a.scale = scale.data_ptr() if scale is not None else None
    a.shift = shift.data_ptr() if shift is not None else None
    a.residual, a.residual_stride = residual, residual_stride
    a.relu, a.out, a.out_stride, a.n_images = relu, out, out_stride, n_images
    a.cin, a.cout, a.H, a.W, a.ksize, a.stride = geometry
    if up is not None:
        a.residual_H, a.residual_W = up


def _conv2d_affine(x, weight, scale, shift, stride, residual, relu, out, up):
    """one launch of either entry point after the checks both share; ``up``: the residual is a map of another size"""
    xx = _dense_input(x, "x")
    w = capi.f32c(weight.detach())
    capi.require_device(w)
    n, cin, h, wd = xx.shape
    if w.dim() != 4 or int(w.shape[1]) != cin or w.shape[2] != w.shape[3] or w.device != xx.device:
        raise MpnhipError("weight %s does not fit %d input channels on %s" % (tuple(w.shape), cin, xx.device))
    cout, k = int(w.shape[0]), int(w.shape[2])
    ho, wo = _conv_out(h, stride), _conv_out(wd, stride)
    sc, sh = _vec(scale, cout, xx, "scale"), _vec(shift, cout, xx, "shift")
    res = None
    if up or residual is not None:
        res = _dense_input(residual, "residual")
        want = (n, cout) if up else (n, cout, ho, wo)
        if tuple(res.shape[:len(want)]) != want or res.device != xx.device:
            raise MpnhipError("residual must be [%d, %d, %s] on %s" % (n, cout, "rh, rw" if up else "%d, %d" % (ho, wo), xx.device))
    y = _out_tensor(out, (n, cout, ho, wo), xx)
    a = capi.ConvAffineUpArgs() if up else capi.ConvAffineArgs()
    fill_conv_args(a, xx.data_ptr(), xx.stride(0), w, sc, sh, *((res.data_ptr(), res.stride(0)) if res is not None else (None, 0)),
                   int(bool(relu)), y.data_ptr(), y.stride(0), int(n), (int(cin), cout, int(h), int(wd), k, int(stride)),
                   (int(res.shape[2]), int(res.shape[3])) if up else None)
    entry = "mpnhip_conv2d_affine_up_forward" if up else "mpnhip_conv2d_affine_forward"
    with torch.cuda.device(y.device):
        capi.check(getattr(capi.load(), entry)(C.byref(a), capi.stream_ptr()), entry)
    return y


def conv2d_affine_native(x, weight, scale, shift, stride=1, residual=None, relu=False, out=None):
    """``mpnhip_conv2d_affine_forward``: Conv2d(k = 1 | 3 | 7, stride 1 | 2, padding k // 2, no bias) on ``x`` [N, cin, H, W]
    with ``weight`` [cout, cin, k, k], then ``* scale + shift`` per output channel (either may be None), ``+ residual``
    ([N, cout, Hout, Wout] or None) and the ReLU.  ``out`` (optional) may be a channel slice of a wider tensor; it must not
    overlap ``x`` or ``residual``.  No autograd."""
    return _conv2d_affine(x, weight, scale, shift, stride, residual, relu, out, up=False)


def conv2d_affine_up_native(x, weight, scale, shift, residual, stride=1, relu=False, out=None):
    """``mpnhip_conv2d_affine_up_forward``: ``conv2d_affine_native`` whose ``residual`` ``[N, cout, rh, rw]`` is a map of another
    size, added as ``F.interpolate(residual, size=(Hout, Wout), mode='nearest')``.  The pyramid's lateral: ``weight`` 1 x 1,
    ``scale`` None, ``shift`` the convolution's bias.  No autograd."""
    return _conv2d_affine(x, weight, scale, shift, stride, residual, relu, out, up=True)


def maxpool2d_native(x, out=None):
    """``mpnhip_maxpool2d_forward``: MaxPool2d(3, stride 2, padding 1) on ``x`` [N, C, H, W].  No autograd."""
    xx = _dense_input(x, "x")
    n, c, h, wd = xx.shape
    y = _out_tensor(out, (n, c, _conv_out(h, 2), _conv_out(wd, 2)), xx)
    with torch.cuda.device(y.device):
        capi.check(capi.load().mpnhip_maxpool2d_forward(capi.ptr(xx), xx.stride(0), int(n), int(c), int(h), int(wd), capi.ptr(y),
                                                        y.stride(0), capi.stream_ptr()), "mpnhip_maxpool2d_forward")
    return y


# ------------------------------------------------------------------------------------------------ BatchNorm folds
def _bn_terms(bn):
    """float64 ``(scale, mean, beta)`` of an eval-mode BatchNorm, ``scale = gamma / sqrt(var + eps)``"""
    var, mean = bn.running_var.detach().double(), bn.running_mean.detach().double()
    gamma = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(var)
    beta = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(var)
    return gamma / torch.sqrt(var + bn.eps), mean, beta


def fold_batchnorm(bn):
    """``(scale, shift)`` of an eval-mode BatchNorm, ``gamma / sqrt(var + eps)`` and ``beta - mean * scale``: float64 arithmetic,
    one rounding to the module's dtype."""
    scale, mean, beta = _bn_terms(bn)
    shift = beta - mean * scale
    dtype = bn.running_var.dtype
    return scale.to(dtype).contiguous(), shift.to(dtype).contiguous()


def fold_linear_batchnorm(linear, bn):
    """``(weight, bias)`` of ``bn(linear(x))`` as one Linear, float64 arithmetic, one rounding to the module's dtype."""
    scale, mean, beta = _bn_terms(bn)
    w = linear.weight.detach().double() * scale[:, None]
    b0 = linear.bias.detach().double() if linear.bias is not None else torch.zeros_like(mean)
    b = (b0 - mean) * scale + beta
    dtype = linear.weight.dtype
    return w.to(dtype).contiguous(), b.to(dtype).contiguous()


# ------------------------------------------------------------------------------------------------ modules
class Bottleneck(nn.Module):
    """1 x 1 -> 3 x 3 (carries the stride) -> 1 x 1 (x 4 channels), each with its norm layer, around a shortcut."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = norm_layer(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = norm_layer(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = norm_layer(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out = out + (x if self.downsample is None else self.downsample(x))
        return self.relu(out)


def make_layer(block, inplanes, planes, blocks, stride, norm_layer=nn.BatchNorm2d):
    """``blocks`` blocks of ``planes`` as a Sequential, the first with the stride and, where the shape changes, a 1 x 1
    downsample.  ``block`` is built with its own default norm layer unless another ``norm_layer`` is asked for."""
    kw = {} if norm_layer is nn.BatchNorm2d else dict(norm_layer=norm_layer)
    out = planes * block.expansion
    downsample = None
    if stride != 1 or inplanes != out:
        downsample = nn.Sequential(nn.Conv2d(inplanes, out, 1, stride=stride, bias=False), norm_layer(out))
    stack = [block(inplanes, planes, stride, downsample, **kw)]
    stack += [block(out, planes, **kw) for _ in range(1, blocks)]
    return nn.Sequential(*stack)


class DropsNativeCache:
    """Mixin in front of ``nn.Module``: whatever changes the parameters or the mode -- ``load_state_dict``, ``.to()`` (anything
    that goes through ``_apply``), ``.train()`` / ``.eval()`` -- drops the folded constants and plans cached in ``_native``."""

    def load_state_dict(self, *args, **kw):
        self._native = None
        return super().load_state_dict(*args, **kw)

    def _apply(self, *args, **kw):
        self._native = None
        return super()._apply(*args, **kw)

    def train(self, mode=True):
        self._native = None
        return super().train(mode)


def resnet_conv_layers(body, prefix, H, W):
    """Every convolution of a ResNet ``body`` (``conv1, bn1, layer1 .. layer4`` of Bottlenecks) in execution order for an
    ``H x W`` input, as dicts: ``name`` (the Conv2d's name in the module tree, after ``prefix``), ``bn`` (its BatchNorm's),
    ``cin, cout, k, stride, H, W`` (input size), ``Hout, Wout``."""
    out = []

    def add(name, bn, conv, h, w):
        s = int(conv.stride[0])
        out.append(dict(name=prefix + name, bn=prefix + bn, cin=conv.in_channels, cout=conv.out_channels, k=int(conv.kernel_size[0]),
                        stride=s, H=h, W=w, Hout=_conv_out(h, s), Wout=_conv_out(w, s)))
        return out[-1]["Hout"], out[-1]["Wout"]

    h, w = add("conv1", "bn1", body.conv1, H, W)
    h, w = _conv_out(h, 2), _conv_out(w, 2)
    for li in range(1, 5):
        for bi, blk in enumerate(getattr(body, "layer%d" % li)):
            p = "layer%d.%d." % (li, bi)
            add(p + "conv1", p + "bn1", blk.conv1, h, w)
            h2, w2 = add(p + "conv2", p + "bn2", blk.conv2, h, w)
            if blk.downsample is not None:
                add(p + "downsample.0", p + "downsample.1", blk.downsample[0], h, w)
            add(p + "conv3", p + "bn3", blk.conv3, h2, w2)
            h, w = h2, w2
    return out


# ------------------------------------------------------------------------------------------------ launch plans
class Launch(NamedTuple):
    """One launch: ``kind`` 'conv' | 'pool' (the 3 x 3 / 2 max-pool of ``layer``'s OUTPUT), ``layer`` a bound layer dict
    (``bind_layer``), the buffers ``src`` -> ``dst`` with ``residual`` (or None) added, ``relu``, and ``up``: None for
    ``mpnhip_conv2d_affine_forward``, the residual's ``(h, w)`` for ``mpnhip_conv2d_affine_up_forward``."""
    kind: str
    layer: dict
    src: Any
    dst: Any
    residual: Any = None
    relu: bool = False
    up: Optional[Tuple[int, int]] = None


class Stage(NamedTuple):
    """marks that ``buffer`` now holds the activation ``name`` (diagnosis: ``run_steps`` copies it out on request)"""
    name: str
    buffer: Any


def bind_layer(c, conv, scale, shift):
    """completes a layer dict for a plan: ``weight`` (the parameter itself: a deepcopy of the module keeps the tie), ``scale``
    and ``shift`` (tensors or None), ``out_shape`` of an image, its ``floats``, and ``geometry`` as ``fill_conv_args`` takes it"""
    if not conv.weight.is_contiguous():
        raise MpnhipError("forward_native: %s.weight is not contiguous" % c["name"])
    c["weight"], c["scale"], c["shift"] = conv.weight, scale, shift
    c["out_shape"] = (c["cout"], c["Hout"], c["Wout"])
    c["floats"] = c["cout"] * c["Hout"] * c["Wout"]
    c["geometry"] = (c["cin"], c["cout"], c["H"], c["W"], c["k"], c["stride"])
    return c


def resnet_body_steps(body, prefix, layers, keep, stage_names):
    """The steps of a ResNet ``body``: the stem's convolution, the max-pool and every bottleneck; ``layers``: bound layer dicts by
    name, ``keep``: {layer index 1 .. 4: name of the buffer that layer's last block writes}, ``stage_names``: the stage after
    each of the four layers (after the pool it is ``'stem'``).

    The buffer rule.  'x' is the input, 0 .. 2 are three activation buffers the blocks take turns in, a kept buffer stays alive
    for whoever reads it after the body.  The stem goes 'x' -> 0 -> (pool) 1.  Inside a bottleneck with its input in ``ci`` and
    ``a``, ``b`` the first two of the three that are not ``ci``: conv1 -> a, conv2 -> b.  Without a downsample conv3 reads b,
    adds ci and writes a (conv1's output is dead).  With one the shortcut goes to a and conv3 reads b, adds a and writes ci when
    that is one of the three (the input is dead), the third of them when ci is a kept buffer.  The last block of a layer in
    ``keep`` writes the kept buffer instead.  An output never overlaps what its launch reads."""
    stem = layers[prefix + "conv1"]
    steps = [Launch("conv", stem, 'x', 0, None, True), Launch("pool", stem, 0, 1), Stage("stem", 1)]
    ci = 1
    for li in range(1, 5):
        blocks = getattr(body, "layer%d" % li)
        for bi, blk in enumerate(blocks):
            p = "%slayer%d.%d." % (prefix, li, bi)
            free = [i for i in range(3) if i != ci]
            a, b = free[0], free[1]
            kept = keep.get(li) if bi == len(blocks) - 1 else None
            steps.append(Launch("conv", layers[p + "conv1"], ci, a, None, True))
            steps.append(Launch("conv", layers[p + "conv2"], a, b, None, True))
            if blk.downsample is None:
                dst = kept or a
                steps.append(Launch("conv", layers[p + "conv3"], b, dst, ci, True))
            else:
                dst = kept or (ci if isinstance(ci, int) else free[2])
                steps.append(Launch("conv", layers[p + "downsample.0"], ci, a, None, False))
                steps.append(Launch("conv", layers[p + "conv3"], b, dst, a, True))
            ci = dst
        steps.append(Stage(stage_names[li - 1], ci))
    return steps


class _Held:
    """What one buffer of a plan holds for the current slice: ``address`` of the slice's first image, ``stride`` (floats from one
    image to the next) and ``shape`` of an image.  ``fixed``: a caller-visible tensor (the input, a result) whose stride and
    shape never change; the others take the stride and shape of whatever is written into them.  ``tensor``: the flat storage,
    for ``view``."""
    __slots__ = ("address", "stride", "shape", "fixed", "tensor")

    def __init__(self, address, stride=0, shape=None, fixed=False, tensor=None):
        self.address, self.stride, self.shape, self.fixed, self.tensor = address, stride, shape, fixed, tensor

    def take(self, shape):
        """a dense ``[C, h, w]`` image per frame is about to be written here"""
        if not self.fixed:
            self.stride, self.shape = shape[0] * shape[1] * shape[2], shape

    def view(self, m):
        """the ``m`` images held, as a tensor (diagnosis)"""
        return self.tensor[:m * self.stride].view((m,) + self.shape)


_NO_RESIDUAL = _Held(None)


def run_steps(steps, held, m, lib, stream, stages=None):
    """Issues the launches of ``steps`` for one slice of ``m`` images over the buffers ``held`` ({name: ``_Held``}), on
    ``stream``, with one argument struct of each kind for the whole call.  ``stages``: a list that receives ``(name, copy)`` at
    every ``Stage``, or None."""
    plain, upper = capi.ConvAffineArgs(), capi.ConvAffineUpArgs()
    for st in steps:
        if st.__class__ is Stage:
            if stages is not None:
                stages.append((st.name, held[st.buffer].view(m).clone()))
            continue
        kind, c, src, dst, res, relu, up = st
        xs, ys = held[src], held[dst]
        if kind == "pool":
            cout, h, w = c["out_shape"]
            ys.take((cout, _conv_out(h, 2), _conv_out(w, 2)))
            capi.check(lib.mpnhip_maxpool2d_forward(xs.address, xs.stride, m, cout, h, w, ys.address, ys.stride, stream),
                       "mpnhip_maxpool2d_forward")
            continue
        ys.take(c["out_shape"])
        rs = held[res] if res is not None else _NO_RESIDUAL
        a = plain if up is None else upper
        fill_conv_args(a, xs.address, xs.stride, c["weight"], c["scale"], c["shift"], rs.address, rs.stride, relu, ys.address, ys.stride, m,
                       c["geometry"], up)
        if up is None:
            capi.check(lib.mpnhip_conv2d_affine_forward(C.byref(a), stream), "mpnhip_conv2d_affine_forward")
        else:
            capi.check(lib.mpnhip_conv2d_affine_up_forward(C.byref(a), stream), "mpnhip_conv2d_affine_up_forward")
