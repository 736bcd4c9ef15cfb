"""Host-side mirror of the reference's second embedding CNN: the backbone of ``MaskRCNN_FPN``
(``tracktor_masked/maskrcnn_fpn.py:14-24``: torchvision's ``resnet_fpn_backbone('resnet50', False)``), whose four feature levels
``embed_inputs.fpn_roi_align`` pools.  torchvision is not a dependency of this project and was not at hand: the modules below
restate its ``FrozenBatchNorm2d``, ``resnet50`` (the stride on the 3 x 3 convolution), ``IntermediateLayerGetter``,
``FeaturePyramidNetwork`` with ``LastLevelMaxPool`` and ``BackboneWithFPN`` with the same attribute names, so a Mask R-CNN
checkpoint's ``backbone.*`` keys load (``load_maskrcnn_state_dict``).  This module never fetches anything.

One point rests on a reading of torchvision 0.6.0 (the reference's ``environment.yml``) that could not be confirmed here:
``FrozenBatchNorm2d`` is believed to compute ``weight * running_var.rsqrt()`` with NO epsilon in that release; later releases add
``eps = 1e-5``.  ``eps`` is therefore a constructor argument, 0 by default (``resnet50_fpn_backbone(eps=1e-5)`` gives the later
form).

``BackboneWithFPN.forward`` runs the stock PyTorch-ROCm (MIOpen) modules and returns the ordered dict ``'0', '1', '2', '3',
'pool'``.  It is the comparator and the default.

``BackboneWithFPN.forward_native`` is the opt-in no-grad inference forward through the C ABI (csrc/conv_strided.hip): the body
as 53 ``mpnhip_conv2d_affine_forward`` (every frozen BatchNorm folded into ``scale`` / ``shift``, the residual add and the ReLU in
the last convolution of a block) and one ``mpnhip_maxpool2d_forward``; the pyramid as one plain launch for the top lateral, three
``mpnhip_conv2d_affine_up_forward`` for the laterals below it -- the nearest-neighbour upsample of the coarser inner map is read
in the lateral's epilogue -- and four 3 x 3 output convolutions (K = 2304: the grouped summation).  The conv biases go in as
``shift`` with no ``scale``.  ``'pool'`` is a strided slice of ``'3'`` (``max_pool2d(kernel 1, stride 2)`` picks every other
cell).  No MIOpen algorithm search, and the bits of a frame's features do not depend on the batch."""
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from . import capi
from .capi import MpnhipError
from .conv_affine import (Bottleneck, DropsNativeCache, Launch, Stage, _conv_out, _Held, bind_layer, fold_batchnorm, make_layer,
                          resnet_body_steps, resnet_conv_layers, run_steps)
from .conv_affine import conv2d_affine_up_native  # noqa: F401  (importable from here as before)

OUT_CHANNELS = 256
# forward_native's activations per frame in units of the padded input's pixels P = Hp * Wp (floats): the three buffers the
# blocks take turns in 3 x 16 P (conv1's output and layer1's blocks are 16 P each), C2 .. C5 16 + 8 + 4 + 2 = 30 P, the four
# results 21.25 P, the input 3 P -- 102.25 P floats, 409 bytes per pixel: 0.42 GB per frame at 768 x 1344.
NATIVE_FLOATS_PER_PIXEL = 102.25
MAX_IMAGES = 8        # frames per slice of forward_native: 3.4 GB of activations at 768 x 1344


class FrozenBatchNorm2d(nn.Module):
    """BatchNorm2d whose statistics and affine are fixed buffers (``weight, bias, running_mean, running_var``; no
    ``num_batches_tracked`` -- a key of that name in a loaded state dict is dropped).  ``eps``: see the module docstring."""

    def __init__(self, n, eps=0.0):
        super().__init__()
        self.eps = float(eps)
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        state_dict.pop(prefix + "num_batches_tracked", None)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x):
        scale = self.weight * (self.running_var + self.eps).rsqrt()
        bias = self.bias - self.running_mean * scale
        return x * scale.reshape(1, -1, 1, 1) + bias.reshape(1, -1, 1, 1)


class ResNetBody(nn.Module):
    """``IntermediateLayerGetter(resnet50(norm_layer=FrozenBatchNorm2d), {'layer1': '0', ..., 'layer4': '3'})``: the network
    without ``avgpool`` and ``fc``; ``forward`` returns the outputs of ``layer1 .. layer4`` as ``'0' .. '3'``."""

    def __init__(self, layers=(3, 4, 6, 3), norm_layer=FrozenBatchNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = make_layer(Bottleneck, 64, 64, layers[0], 1, norm_layer)
        self.layer2 = make_layer(Bottleneck, 256, 128, layers[1], 2, norm_layer)
        self.layer3 = make_layer(Bottleneck, 512, 256, layers[2], 2, norm_layer)
        self.layer4 = make_layer(Bottleneck, 1024, 512, layers[3], 2, norm_layer)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        out = OrderedDict()
        for i in range(4):
            x = getattr(self, "layer%d" % (i + 1))(x)
            out[str(i)] = x
        return out


class FeaturePyramidNetwork(nn.Module):
    """torchvision's ``FeaturePyramidNetwork(in_channels_list, out_channels, LastLevelMaxPool())``: ``inner_blocks`` 1 x 1 and
    ``layer_blocks`` 3 x 3, both with bias; top-down ``inner = lateral + interpolate(coarser inner, nearest)``."""

    def __init__(self, in_channels_list=(256, 512, 1024, 2048), out_channels=OUT_CHANNELS):
        super().__init__()
        self.inner_blocks = nn.ModuleList([nn.Conv2d(c, out_channels, 1) for c in in_channels_list])
        self.layer_blocks = nn.ModuleList([nn.Conv2d(out_channels, out_channels, 3, padding=1) for _ in in_channels_list])
        for m in self.children():
            for conv in m:
                nn.init.kaiming_uniform_(conv.weight, a=1)
                nn.init.constant_(conv.bias, 0)

    def inner_maps(self, x):
        """the inner maps, coarsest first (``x``: the body's ordered dict)"""
        feats = list(x.values())
        inner = [self.inner_blocks[-1](feats[-1])]
        for idx in range(len(feats) - 2, -1, -1):
            lateral = self.inner_blocks[idx](feats[idx])
            inner.append(lateral + F.interpolate(inner[-1], size=lateral.shape[-2:], mode='nearest'))
        return inner

    def forward(self, x):
        inner = self.inner_maps(x)[::-1]
        out = OrderedDict((name, self.layer_blocks[i](inner[i])) for i, name in enumerate(x.keys()))
        out['pool'] = F.max_pool2d(out[list(x.keys())[-1]], 1, 2, 0)
        return out


class BackboneWithFPN(DropsNativeCache, nn.Module):
    """``body`` + ``fpn``, see the module docstring.  State-dict names are torchvision's: ``body.conv1.weight``, ``body.bn1.*``,
    ``body.layerL.B.convK.weight``, ``body.layerL.B.bnK.*``, ``body.layerL.0.downsample.{0,1}.*``,
    ``fpn.inner_blocks.I.{weight,bias}``, ``fpn.layer_blocks.I.{weight,bias}``."""

    def __init__(self, eps=0.0):
        super().__init__()
        self.body = ResNetBody(norm_layer=lambda n: FrozenBatchNorm2d(n, eps))
        self.fpn = FeaturePyramidNetwork()
        self.out_channels = OUT_CHANNELS
        self._native = None

    def forward(self, x):
        return self.fpn(self.body(x))

    # ---- the native forward
    def conv_layers(self, H, W):
        """Every convolution of the body in execution order for an ``H x W`` input (``conv_affine.resnet_conv_layers``)"""
        return resnet_conv_layers(self.body, "body.", H, W)

    def level_shapes(self, H, W):
        """``[(h, w)]`` of the levels ``'0' .. '3'`` and ``'pool'`` for an ``H x W`` input"""
        h, w = _conv_out(_conv_out(H, 2), 2), _conv_out(_conv_out(W, 2), 2)
        out = [(h, w)]
        for _ in range(3):
            h, w = _conv_out(h, 2), _conv_out(w, 2)
            out.append((h, w))
        return out + [(_conv_out(h, 2), _conv_out(w, 2))]

    def _check_native(self):
        if self.training:
            raise MpnhipError("forward_native is the inference forward: call .eval() first")

    def prepare_native(self):
        """Folds every frozen BatchNorm in float64, rounded once: ``self._native = {'affine': {conv name: (scale, shift)},
        'plans': {(H, W): launch list}}`` on the parameters' device.  Called by ``forward_native`` when no cache exists."""
        self._check_native()
        mods = dict(self.named_modules())
        affine = OrderedDict((c["name"], fold_batchnorm(mods[c["bn"]])) for c in self.conv_layers(64, 64))
        self._native = dict(affine=affine, plans={})
        return self._native

    def _plan(self, native, H, W):
        """The launch list of one slice for an ``H x W`` input, cached beside the folded constants.  The body's steps are
        ``conv_affine.resnet_body_steps`` with every layer's output kept: 'c2' .. 'c5' stay alive until their lateral has run.
        The pyramid follows, coarsest level first: the inner maps take turns in buffers 0 and 1, which the body no longer needs,
        and the output convolutions write the results '0' .. '3'."""
        plan = native["plans"].get((H, W))
        if plan is not None:
            return plan
        mods = dict(self.named_modules())
        layers = {c["name"]: bind_layer(c, mods[c["name"]], *native["affine"][c["name"]]) for c in self.conv_layers(H, W)}
        keep = {li: 'c%d' % (li + 1) for li in range(1, 5)}
        steps = resnet_body_steps(self.body, "body.", layers, keep, ("C2", "C3", "C4", "C5"))
        kept = {st.dst: st.layer["floats"] for st in steps if isinstance(st, Launch) and st.dst in keep.values()}
        shapes = self.level_shapes(H, W)
        prev = None
        for i in range(3, -1, -1):
            h, w = shapes[i]
            for name, k in (("fpn.inner_blocks.%d" % i, 1), ("fpn.layer_blocks.%d" % i, 3)):     # the convolutions' biases go in as shift
                layers[name] = bind_layer(dict(name=name, cin=mods[name].in_channels, cout=OUT_CHANNELS, k=k, stride=1, H=h, W=w, Hout=h,
                                               Wout=w), mods[name], None, mods[name].bias)
            buf = 0 if prev != 0 else 1
            up = None if prev is None else shapes[i + 1]
            steps.append(Launch("conv", layers["fpn.inner_blocks.%d" % i], 'c%d' % (i + 2), buf, prev, False, up))
            steps.append(Stage("inner%d" % i, buf))
            steps.append(Launch("conv", layers["fpn.layer_blocks.%d" % i], buf, str(i)))
            prev = buf
        plan = dict(steps=steps, per_image=max(c["floats"] for c in layers.values()), kept=kept, shapes=shapes)
        native["plans"][(H, W)] = plan
        return plan

    @torch.no_grad()
    def forward_native(self, x, max_images=MAX_IMAGES, stages=None):
        """``forward`` without autograd through the native kernels: the ordered dict ``'0', '1', '2', '3', 'pool'``.  ``x``:
        contiguous float32 ``[n, 3, H, W]`` on the device (``embed_inputs.rcnn_transform``'s batch).  The batch is processed in
        slices of at most ``max_images`` frames; the result does not depend on it.  A slice's activations are
        ``NATIVE_FLOATS_PER_PIXEL`` = 102.25 floats per input pixel and frame with the input and the results -- 0.42 GB per frame
        at 768 x 1344, the padded size of a 1080 x 1920 frame --, so the default of 8 frames holds 3.4 GB.  ``stages``
        (diagnosis): a list that receives ``(name, copy)`` of ``'stem'`` (conv1, bn1, ReLU, max-pool), ``'C2' .. 'C5'`` (the body's
        outputs) and the inner maps ``'inner3' .. 'inner0'`` in the order they are computed, per slice."""
        self._check_native()
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise MpnhipError("forward_native takes a float32 [n, 3, H, W] tensor on the device")
        if not x.is_contiguous():
            raise MpnhipError("forward_native takes a contiguous input")
        w0 = self.body.conv1.weight
        if w0.device != x.device or w0.dtype != torch.float32:
            raise MpnhipError("forward_native: the module must be float32 on the input's device (%s)" % x.device)
        native = self._native if self._native is not None else self.prepare_native()
        n, _, H, W = (int(s) for s in x.shape)
        plan = self._plan(native, H, W)
        step = max(min(int(max_images), n), 1)
        shapes = plan["shapes"]
        lib = capi.load()
        with torch.cuda.device(x.device):
            stream = capi.stream_ptr()
            out = OrderedDict((str(i), torch.empty((n, OUT_CHANNELS) + shapes[i], dtype=torch.float32, device=x.device)) for i in range(4))
            if n == 0:
                out['pool'] = out['3'][:, :, ::2, ::2].contiguous()
                return out
            bufs = [torch.empty(step * plan["per_image"], dtype=torch.float32, device=x.device) for _ in range(3)]
            kept = {k: torch.empty(step * v, dtype=torch.float32, device=x.device) for k, v in plan["kept"].items()}
            for k0 in range(0, n, step):
                m = min(step, n - k0)
                held = {'x': _Held(x[k0:k0 + m].data_ptr(), x.stride(0), (3, H, W), fixed=True)}
                for i in range(3):
                    held[i] = _Held(bufs[i].data_ptr(), tensor=bufs[i])
                for k, t in kept.items():
                    held[k] = _Held(t.data_ptr(), tensor=t)
                for i in range(4):
                    held[str(i)] = _Held(out[str(i)][k0:k0 + m].data_ptr(), out[str(i)].stride(0), (OUT_CHANNELS,) + shapes[i], fixed=True)
                run_steps(plan["steps"], held, m, lib, stream, stages)
            out['pool'] = out['3'][:, :, ::2, ::2].contiguous()
        return out


def resnet50_fpn_backbone(eps=0.0):
    """The reference's backbone, ``resnet_fpn_backbone('resnet50', pretrained=False)``, with seeded-by-torch initial weights:
    load a checkpoint with ``load_maskrcnn_state_dict``."""
    return BackboneWithFPN(eps=eps)


IGNORED_PREFIXES = ("rpn.", "roi_heads.", "transform.")


def load_maskrcnn_state_dict(backbone, state_dict):
    """Loads the backbone's tensors out of a whole Mask R-CNN ``state_dict`` (the reference's ``MaskRCNN_FPN`` checkpoint): the
    ``backbone.`` prefix is stripped, ``rpn.*``, ``roi_heads.*`` and ``transform.*`` are ignored, ``num_batches_tracked`` entries
    are dropped.  Strict about the backbone itself: a missing key, a key the backbone does not have and a tensor of another
    shape raise ``MpnhipError``.  Returns the sorted list of the keys loaded."""
    own = backbone.state_dict()
    picked = OrderedDict()
    for k, t in state_dict.items():
        if k.startswith(IGNORED_PREFIXES) or k.rsplit(".", 1)[-1] == "num_batches_tracked":
            continue
        name = k[len("backbone."):] if k.startswith("backbone.") else k
        if name not in own:
            raise MpnhipError("load_maskrcnn_state_dict: %s is no tensor of the backbone" % k)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(own[name].shape):
            raise MpnhipError("load_maskrcnn_state_dict: %s has shape %s, the backbone's is %s"
                              % (k, tuple(getattr(t, "shape", ())), tuple(own[name].shape)))
        picked[name] = t
    missing = [k for k in own if k not in picked]
    if missing:
        raise MpnhipError("load_maskrcnn_state_dict: %d backbone tensors are missing, the first %s" % (len(missing), missing[0]))
    backbone.load_state_dict(picked, strict=True)
    return sorted(picked)
