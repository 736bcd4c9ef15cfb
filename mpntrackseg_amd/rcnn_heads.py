"""Host-side mirror of the Mask R-CNN RoI heads on GIVEN boxes: what the reference does with its detector after ``load_image``
(``tracktor_masked/frcnn_fpn.py:29-64``, ``tracktor_masked/maskrcnn_fpn.py:31-79``, ``data/preprocessing.py:19-42``,
``tracker/mpn_tracker.py:300-341``).  The RPN, anchors and ``detect()`` are not here.  torchvision is not a dependency of this
project: the modules below restate its ``TwoMLPHead``, ``FastRCNNPredictor``, ``MaskRCNNHeads`` and mask predictor with the same
member names, so a checkpoint's ``roi_heads.*`` keys load (``load_maskrcnn_state_dict``).  This module never fetches anything.

``predict_boxes``      ``FRCNN_FPN.predict_boxes``: refined boxes in the original image and the label's scores;
``predict_masks``      ``MaskRCNN_FPN.predict_masks(return_roi_masks=True)``, with ``upsample=2`` what ``_predict_nan_masks`` stores;
``predict``            ``MaskRCNN_FPN.predict`` without the paste: the masks are taken on the refined boxes;
``nms_batched``        ``scores >= thresh`` + ``torchvision.ops.nms`` for every frame of a batch (``mpnhip_nms_batched``);
``refine_detections``  ``FRCNNPreprocessor.step`` over a batch of frames + ``save_results``'s table; ``write_det_file`` its csv;
``nan_roi_masks``      frames and boxes -> the 56 x 56 RoI masks of ``_predict_nan_masks``.

Every function takes ``convs='stock' | 'native'``.  ``'stock'`` (the default, the comparator) runs the torch modules' ``forward``
and torch operators behind ``mpnhip_fpn_roi_align``.  ``'native'`` is no-grad inference through the C ABI (csrc/rcnn_heads.hip and
the kernels named below); it refuses heads in training mode.  The native route enqueues everything on the current stream and
never reads the device back; the one host read of the whole path is in ``refine_detections`` (see there).

The boxes' levels (torchvision 0.6.0's ``LevelMapper``) and ``resize_boxes`` are per-box torch float32 arithmetic on the device,
so that refined boxes never travel to the host.  A box that is not finite gets zeros from the pooler."""
import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import capi, embed_inputs
from .capi import MpnhipError, check, ptr, stream_ptr
from .cnn import _image_dense, conv2d_native
from .conv_affine import conv2d_affine_native

BBOX_REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)         # RoIHeads' default bbox_reg_weights
BBOX_XFORM_CLIP = math.log(1000.0 / 16)           # BoxCoder's bbox_xform_clip
NMS_MAX_PER_FRAME = 4096                          # MPNHIP_NMS_MAX_PER_FRAME
BOX_MAX_CLASSES = 91                              # MPNHIP_BOX_MAX_CLASSES
LEVELS = ('0', '1', '2', '3')


# ------------------------------------------------------------------------------------------------ modules
class TwoMLPHead(nn.Module):
    """torchvision's ``TwoMLPHead``: flatten, ``fc6``, ReLU, ``fc7``, ReLU"""

    def __init__(self, in_channels=256 * 7 * 7, representation_size=1024):
        super().__init__()
        self.fc6 = nn.Linear(in_channels, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)

    def forward(self, x):
        x = x.flatten(start_dim=1)
        return F.relu(self.fc7(F.relu(self.fc6(x))))


class FastRCNNPredictor(nn.Module):
    """torchvision's ``FastRCNNPredictor``: ``(cls_score(x) [n, C], bbox_pred(x) [n, 4 C])``"""

    def __init__(self, in_channels=1024, num_classes=2):
        super().__init__()
        self.cls_score = nn.Linear(in_channels, num_classes)
        self.bbox_pred = nn.Linear(in_channels, num_classes * 4)

    def forward(self, x):
        x = x.flatten(start_dim=1)
        return self.cls_score(x), self.bbox_pred(x)


class MaskRCNNHeads(nn.Sequential):
    """torchvision's ``MaskRCNNHeads``: ``mask_fcnI`` (3 x 3, padding 1) + ``reluI`` for every entry of ``layers``"""

    def __init__(self, in_channels=256, layers=(256, 256, 256, 256)):
        d = OrderedDict()
        nxt = in_channels
        for i, c in enumerate(layers, 1):
            d["mask_fcn%d" % i] = nn.Conv2d(nxt, c, 3, stride=1, padding=1)
            d["relu%d" % i] = nn.ReLU(inplace=True)
            nxt = c
        super().__init__(d)
        for name, p in self.named_parameters():
            if "weight" in name:
                nn.init.kaiming_normal_(p, mode="fan_out", nonlinearity="relu")

    def convs(self):
        return [m for m in self if isinstance(m, nn.Conv2d)]


class MaskLogitsPredictor(nn.Sequential):
    """torchvision's ``MaskRCNNPredictor`` (``cnn.MaskRCNNPredictor`` is the tracker's own mask branch): ``conv5_mask``
    (ConvTranspose2d 2 x 2, stride 2), ReLU, ``mask_fcn_logits`` (1 x 1)"""

    def __init__(self, in_channels=256, dim_reduced=256, num_classes=2):
        super().__init__(OrderedDict([
            ("conv5_mask", nn.ConvTranspose2d(in_channels, dim_reduced, 2, 2, 0)),
            ("relu", nn.ReLU(inplace=True)),
            ("mask_fcn_logits", nn.Conv2d(dim_reduced, num_classes, 1, 1, 0))]))
        for name, p in self.named_parameters():
            if "weight" in name:
                nn.init.kaiming_normal_(p, mode="fan_out", nonlinearity="relu")


class RoIHeads(nn.Module):
    """The parameters of torchvision's ``RoIHeads`` under its member names: ``box_head``, ``box_predictor`` and, with ``mask``,
    ``mask_head`` and ``mask_predictor``.  ``state_dict`` keys are a checkpoint's ``roi_heads.*`` names without the prefix.
    ``channels``: the pyramid's; ``box_resolution`` / ``mask_resolution``: the poolers' output sizes (7 and 14);
    ``mask_layers``: the mask head's widths (default four times ``channels``)."""

    def __init__(self, num_classes=2, channels=256, representation_size=1024, mask=True, box_resolution=7, mask_resolution=14,
                 mask_layers=None):
        super().__init__()
        if not 2 <= int(num_classes) <= BOX_MAX_CLASSES:
            raise ValueError("num_classes must lie in [2, %d]" % BOX_MAX_CLASSES)
        self.num_classes, self.channels = int(num_classes), int(channels)
        self.box_resolution, self.mask_resolution = int(box_resolution), int(mask_resolution)
        self.box_head = TwoMLPHead(channels * box_resolution ** 2, representation_size)
        self.box_predictor = FastRCNNPredictor(representation_size, num_classes)
        if mask:
            layers = tuple(mask_layers) if mask_layers is not None else (channels,) * 4
            self.mask_head = MaskRCNNHeads(channels, layers)
            self.mask_predictor = MaskLogitsPredictor(layers[-1], layers[-1], num_classes)

    @property
    def has_mask(self):
        return hasattr(self, "mask_head")


HEAD_PREFIX = "roi_heads."


def load_maskrcnn_state_dict(heads, state_dict):
    """Loads the heads' tensors out of a whole Mask R-CNN or Faster R-CNN ``state_dict`` (the one
    ``fpn_net.load_maskrcnn_state_dict`` takes): the ``roi_heads.`` keys, the prefix stripped; everything else is ignored.
    Strict about the heads themselves: a missing key, a ``roi_heads.`` key the heads do not have (a Mask R-CNN checkpoint into
    ``RoIHeads(mask=False)`` included) and a tensor of another shape raise ``MpnhipError``.  Returns the sorted keys loaded."""
    own = heads.state_dict()
    picked = OrderedDict()
    for k, t in state_dict.items():
        if not k.startswith(HEAD_PREFIX):
            continue
        name = k[len(HEAD_PREFIX):]
        if name not in own:
            raise MpnhipError("load_maskrcnn_state_dict: %s is no tensor of the heads" % k)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(own[name].shape):
            raise MpnhipError("load_maskrcnn_state_dict: %s has shape %s, the heads' is %s"
                              % (k, tuple(getattr(t, "shape", ())), tuple(own[name].shape)))
        picked[name] = t
    missing = [k for k in own if k not in picked]
    if missing:
        raise MpnhipError("load_maskrcnn_state_dict: %d tensors of the heads are missing, the first %s" % (len(missing), missing[0]))
    heads.load_state_dict(picked, strict=True)
    return sorted(picked)


# ------------------------------------------------------------------------------------------------ operators
def _check_convs(convs, heads):
    if convs not in ('stock', 'native'):
        raise ValueError("convs must be 'stock' or 'native', not %r" % (convs,))
    if convs == 'native' and heads is not None and heads.training:
        raise MpnhipError("convs='native' is the inference route: call .eval() first")


def _levels(features):
    """the four levels '0' .. '3' of ``fpn_features``' ordered dict (or a sequence of four tensors)"""
    if hasattr(features, "keys"):
        return [features[k] for k in LEVELS]
    return list(features)


def back_ratios(image_size, original_size):
    """``resize_boxes``' ratios from the network's image back to the frame, as Python floats: ``(ratio_h, ratio_w)``"""
    return float(original_size[0]) / float(image_size[0]), float(original_size[1]) / float(image_size[1])


def _frames_of(box_frame, n, B):
    if isinstance(box_frame, torch.Tensor):
        box_frame = box_frame.detach().cpu().numpy()
    return embed_inputs._frame_index(box_frame, n, B)


def _device_boxes(boxes, dev):
    """float32 [n, 4] on ``dev``; host boxes (an array or a table with the ``bb_*`` columns) are checked as ``map_boxes`` does"""
    if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
        return boxes.detach().to(torch.float32).reshape(-1, 4).to(dev)
    b = embed_inputs._boxes_of(boxes.detach().numpy() if isinstance(boxes, torch.Tensor) else boxes, np.float32)
    if not np.isfinite(b).all():
        raise ValueError("box %d is not finite" % int(np.flatnonzero(~np.isfinite(b).all(axis=1))[0]))
    bad = (b[:, 2] < b[:, 0]) | (b[:, 3] < b[:, 1])
    if bad.any():
        raise ValueError("box %d has x2 < x1 or y2 < y1" % int(np.flatnonzero(bad)[0]))
    return torch.from_numpy(b).to(dev)


def fpn_roi_align(features, boxes, frame_idx, image_size, output_size):
    """``mpnhip_fpn_roi_align`` for ``boxes`` float32 [n, 4] ON THE DEVICE, in the network's image: their levels are computed
    there (``embed_inputs.box_levels``), nothing is read back.  ``frame_idx``: int32 [n] on the device."""
    feats = _levels(features)
    dev, B, channels = embed_inputs._check_features(feats)
    capi.require_device(*feats)
    scales = embed_inputs.level_scales([f.shape[2:] for f in feats], image_size)
    k_min, k_max = int(-math.log2(scales[0])), int(-math.log2(scales[-1]))
    n, S = int(boxes.shape[0]), int(output_size)
    lv = capi.FpnLevels()
    with torch.cuda.device(dev):
        feats = [f.contiguous() for f in feats]
        for l, f in enumerate(feats):
            lv.data[l], lv.h[l], lv.w[l], lv.scale[l] = f.data_ptr(), int(f.shape[2]), int(f.shape[3]), scales[l]
        levels = embed_inputs.box_levels(boxes, k_min, k_max).to(torch.int32)
        b = boxes.contiguous()
        out = torch.empty((n, channels, S, S), dtype=torch.float32, device=dev)
        check(capi.load().mpnhip_fpn_roi_align(C.byref(lv), B, channels, ptr(b), ptr(frame_idx), ptr(levels), n, S, 2, None, ptr(out),
                                               stream_ptr()), "mpnhip_fpn_roi_align")
    return out


def linear_native(x, weight, bias, relu=False):
    """``mpnhip_linear``: ``act(x W^T + b)`` for ``x`` float32 [m, k] on the device (rows dense).  No autograd."""
    w, b = capi.f32c(weight.detach()), capi.f32c(bias.detach())
    capi.require_device(x, w, b)
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1 or int(x.shape[1]) != int(w.shape[1]) or w.device != x.device:
        raise MpnhipError("linear_native: x %s does not fit weight %s on %s" % (tuple(x.shape), tuple(w.shape), w.device))
    y = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
    if x.shape[0]:
        with torch.cuda.device(x.device):
            check(capi.load().mpnhip_linear(ptr(x), x.stride(0), ptr(w), ptr(b), ptr(y), y.stride(0), int(x.shape[0]), int(w.shape[0]),
                                            int(w.shape[1]), int(bool(relu)), stream_ptr()), "mpnhip_linear")
    return y


def box_predict_native(h, predictor, proposals, label=1, ratios=(1.0, 1.0), weights=BBOX_REG_WEIGHTS, clip=BBOX_XFORM_CLIP,
                       return_raw=False):
    """``mpnhip_box_predict``: ``(boxes [n, 4], scores [n])`` -- with ``return_raw`` also ``(logits [n, C], deltas [n, 4])`` --
    from the box head's output ``h`` [n, K] (any row stride), a ``FastRCNNPredictor`` and ``proposals`` float32 [n, 4] in the
    network's image, all on the device.  ``ratios = (ratio_h, ratio_w)``: ``back_ratios``, or (1, 1) to stay in that image."""
    wc, bc = capi.f32c(predictor.cls_score.weight.detach()), capi.f32c(predictor.cls_score.bias.detach())
    wb, bb = capi.f32c(predictor.bbox_pred.weight.detach()), capi.f32c(predictor.bbox_pred.bias.detach())
    capi.require_device(h, wc, bc, wb, bb, proposals)
    if h.dim() != 2 or h.dtype != torch.float32 or (h.shape[1] > 1 and h.stride(1) != 1) or int(h.shape[1]) != int(wc.shape[1]):
        raise MpnhipError("box_predict_native: h %s does not fit cls_score %s" % (tuple(h.shape), tuple(wc.shape)))
    n, k, nc = int(h.shape[0]), int(wc.shape[1]), int(wc.shape[0])
    p = capi.f32c(proposals).reshape(-1, 4)
    if int(p.shape[0]) != n or tuple(wb.shape) != (4 * nc, k):
        raise MpnhipError("box_predict_native: %d proposals for %d rows, bbox_pred %s" % (p.shape[0], n, tuple(wb.shape)))
    dev = h.device
    boxes, scores = torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)
    logits = torch.empty((n, nc), dtype=torch.float32, device=dev) if return_raw else None
    deltas = torch.empty((n, 4), dtype=torch.float32, device=dev) if return_raw else None
    wts = (C.c_float * 4)(*[float(v) for v in weights])
    with torch.cuda.device(dev):
        check(capi.load().mpnhip_box_predict(ptr(h), h.stride(0) if n > 1 else k, ptr(wc), ptr(bc), ptr(wb), ptr(bb),
                                             ptr(p), n, k, nc, int(label), wts, float(np.float32(clip)), float(np.float32(ratios[0])),
                                             float(np.float32(ratios[1])), ptr(boxes), ptr(scores), ptr(logits), ptr(deltas), stream_ptr()),
              "mpnhip_box_predict")
    return (boxes, scores, logits, deltas) if return_raw else (boxes, scores)


def roi_mask_finish_native(logits, label=0, upsample=1):
    """``mpnhip_roi_mask_finish``: ``[n, S * up, S * up]`` from mask logits float32 [n, C, S, S] on the device with dense images
    (a channel slice of a wider tensor is fine)."""
    capi.require_device(logits)
    if logits.dim() != 4 or logits.shape[2] != logits.shape[3]:
        raise MpnhipError("roi_mask_finish_native takes logits [n, C, S, S]")
    x = logits if _image_dense(logits) else capi.f32c(logits)
    n, c, s, _ = (int(v) for v in x.shape)
    up = int(upsample)
    out = torch.empty((n, s * up, s * up), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(capi.load().mpnhip_roi_mask_finish(ptr(x), x.stride(0) if n > 1 else c * s * s, n, c, int(label), s, up, ptr(out), stream_ptr()),
              "mpnhip_roi_mask_finish")
    return out


def decode_boxes(deltas, proposals, weights=BBOX_REG_WEIGHTS, clip=BBOX_XFORM_CLIP):
    """torchvision 0.6.0's ``BoxCoder.decode_single`` for ONE class in torch operators: ``deltas`` [n, 4], ``proposals`` [n, 4]"""
    wx, wy, ww, wh = weights
    widths, heights = proposals[:, 2] - proposals[:, 0], proposals[:, 3] - proposals[:, 1]
    ctr_x, ctr_y = proposals[:, 0] + 0.5 * widths, proposals[:, 1] + 0.5 * heights
    dx, dy = deltas[:, 0] / wx, deltas[:, 1] / wy
    dw, dh = torch.clamp(deltas[:, 2] / ww, max=clip), torch.clamp(deltas[:, 3] / wh, max=clip)
    pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
    pw, ph = torch.exp(dw) * widths, torch.exp(dh) * heights
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=1)


def box_branch(heads, pooled, proposals, label=1, ratios=(1.0, 1.0), convs='stock'):
    """Box head + predictor + softmax + decoding on ``pooled`` [n, C, 7, 7] and ``proposals`` [n, 4] in the network's image:
    ``(boxes * ratios, scores of label)``.  Native: ``mpnhip_linear`` twice with ReLU, ``mpnhip_box_predict``."""
    _check_convs(convs, heads)
    with torch.no_grad():
        if convs == 'native':
            h = pooled.reshape(pooled.shape[0], -1)
            h = linear_native(h, heads.box_head.fc6.weight, heads.box_head.fc6.bias, relu=True)
            h = linear_native(h, heads.box_head.fc7.weight, heads.box_head.fc7.bias, relu=True)
            return box_predict_native(h, heads.box_predictor, proposals, label, ratios)
        logits, reg = heads.box_predictor(heads.box_head(pooled))
        scores = F.softmax(logits, -1)[:, label]
        boxes = decode_boxes(reg[:, 4 * label:4 * label + 4], proposals.to(reg.dtype))
        rh, rw = float(ratios[0]), float(ratios[1])
        return torch.stack((boxes[:, 0] * rw, boxes[:, 1] * rh, boxes[:, 2] * rw, boxes[:, 3] * rh), dim=1), scores


def mask_branch(heads, pooled, label=1, upsample=1, convs='stock'):
    """Mask head + predictor + ``maskrcnn_inference`` (+ ``Upsample(scale_factor=2, mode='bilinear')``) on ``pooled``
    [n, C, 14, 14]: ``[n, 1, 28 * upsample, 28 * upsample]``.  Native: one ``mpnhip_conv2d_affine_forward`` per 3 x 3 layer (the
    bias as ``shift``, the ReLU fused), ``mpnhip_conv2d_forward`` for the transposed convolution (ReLU fused) and for the 1 x 1
    logits of the label's channel alone, ``mpnhip_roi_mask_finish``."""
    _check_convs(convs, heads)
    if not heads.has_mask:
        raise MpnhipError("these heads have no mask branch (RoIHeads(mask=False))")
    if upsample not in (1, 2):
        raise ValueError("upsample must be 1 or 2")
    with torch.no_grad():
        if convs == 'native':
            x = pooled
            for conv in heads.mask_head.convs():
                x = conv2d_affine_native(x, conv.weight, None, conv.bias, stride=1, relu=True)
            up, last = heads.mask_predictor.conv5_mask, heads.mask_predictor.mask_fcn_logits
            x = conv2d_native([x], up.weight, up.bias, relu=True, transposed=True)
            x = conv2d_native([x], last.weight[label:label + 1], last.bias[label:label + 1])
            return roi_mask_finish_native(x, 0, upsample)[:, None]
        prob = torch.sigmoid(heads.mask_predictor(heads.mask_head(pooled))[:, label])[:, None]
        if upsample == 2:
            prob = F.interpolate(prob, scale_factor=2, mode='bilinear', align_corners=False)
        return prob


# ------------------------------------------------------------------------------------------------ the reference's calls
def _inputs(features, boxes, box_frame, image_size, original_size):
    feats = _levels(features)
    dev, B, _ = embed_inputs._check_features(feats)
    b = _device_boxes(boxes, dev)
    idx = torch.from_numpy(_frames_of(box_frame, int(b.shape[0]), B)).to(dev)
    return feats, embed_inputs.resize_boxes(b, original_size, image_size), idx


def predict_boxes(heads, features, boxes, box_frame, image_size, original_size, label=1, convs='stock'):
    """``FRCNN_FPN.predict_boxes`` for a batch of frames: ``(boxes [n, 4] in the original image, scores [n])`` on the device.
    ``features``: what ``embed_inputs.fpn_features`` returns; ``boxes`` [n, 4] (left, top, right, bottom) in the ORIGINAL image, an
    array, a table with the ``bb_*`` columns or a device tensor; ``box_frame`` [n]: indices into the batch; ``image_size``: the
    network's resized ``(oh, ow)``; ``original_size``: the frames' ``(H, W)``.  Not clipped to the image, as the reference."""
    _check_convs(convs, heads)
    feats, b, idx = _inputs(features, boxes, box_frame, image_size, original_size)
    pooled = fpn_roi_align(feats, b, idx, image_size, heads.box_resolution)
    return box_branch(heads, pooled, b, label, back_ratios(image_size, original_size), convs)


def predict_masks(heads, features, boxes, box_frame, image_size, original_size, upsample=1, label=1, convs='stock'):
    """``MaskRCNN_FPN.predict_masks(boxes, return_roi_masks=True)`` for a batch of frames: ``[n, 1, 28 * upsample, 28 * upsample]``
    on the device; ``upsample=2`` adds the tracker's ``Upsample(scale_factor=2, mode='bilinear')``.  Arguments as ``predict_boxes``."""
    _check_convs(convs, heads)
    feats, b, idx = _inputs(features, boxes, box_frame, image_size, original_size)
    return mask_branch(heads, fpn_roi_align(feats, b, idx, image_size, heads.mask_resolution), label, upsample, convs)


def predict(heads, features, boxes, box_frame, image_size, original_size, upsample=1, label=1, convs='stock'):
    """``MaskRCNN_FPN.predict`` without ``paste_masks_in_image``: ``(boxes, scores, roi_masks)`` -- the boxes refined and mapped
    back to the original image, the masks pooled on the refined boxes (in the network's image, where the reference pools them)."""
    _check_convs(convs, heads)
    feats, b, idx = _inputs(features, boxes, box_frame, image_size, original_size)
    refined, scores = box_branch(heads, fpn_roi_align(feats, b, idx, image_size, heads.box_resolution), b, label, (1.0, 1.0), convs)
    masks = mask_branch(heads, fpn_roi_align(feats, refined, idx, image_size, heads.mask_resolution), label, upsample, convs)
    rh, rw = back_ratios(image_size, original_size)
    ratio = torch.tensor([rw, rh, rw, rh], dtype=torch.float32).to(refined.device, non_blocking=True)
    return refined * ratio, scores, masks


def frame_ptr(box_frame, n_frames=None):
    """``(ptr int32 [F + 1], largest frame count)`` of a non-decreasing host ``box_frame``; ``ValueError`` when it descends"""
    f = np.asarray(box_frame.detach().cpu().numpy() if isinstance(box_frame, torch.Tensor) else box_frame).reshape(-1)
    if f.size and not np.issubdtype(f.dtype, np.integer):
        raise ValueError("box_frame must hold integers")
    f = f.astype(np.int64)
    if f.size and (f.min() < 0 or (np.diff(f) < 0).any()):
        raise ValueError("box_frame must be non-negative and non-decreasing: the boxes of a frame are consecutive rows")
    F_ = int(n_frames) if n_frames is not None else (int(f[-1]) + 1 if f.size else 0)
    if f.size and f[-1] >= F_:
        raise ValueError("box_frame must hold integers in [0, %d)" % F_)
    p = np.searchsorted(f, np.arange(F_ + 1)).astype(np.int32)
    return p, (int(np.diff(p).max()) if F_ else 0)


def nms_batched_raw(boxes, scores, box_frame, iou_threshold, score_threshold=None, n_frames=None):
    """``mpnhip_nms_batched`` without any read-back: ``(keep uint8 [n], order int32 [n], count int32 [F])`` on the device (see
    include/mpnhip.h).  ``boxes`` float32 [n, 4] and ``scores`` float32 [n] on the device; ``box_frame``: host integers [n],
    non-decreasing; ``score_threshold`` None: no filter.  A frame of more than ``NMS_MAX_PER_FRAME`` boxes is refused."""
    capi.require_device(boxes, scores)
    b, s = capi.f32c(boxes.detach()).reshape(-1, 4), capi.f32c(scores.detach()).reshape(-1)
    n = int(b.shape[0])
    if int(s.shape[0]) != n:
        raise ValueError("one score per box: %d for %d" % (s.shape[0], n))
    p, most = frame_ptr(box_frame, n_frames)
    if int(p[-1]) != n:
        raise ValueError("one frame index per box: %d for %d boxes" % (int(p[-1]), n))
    dev, nf = b.device, int(p.size) - 1
    if n == 0:                                 # the operator is a no-op then: nothing kept in any frame
        return (torch.zeros((0,), dtype=torch.uint8, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev),
                torch.zeros((nf,), dtype=torch.int32, device=dev))
    keep = torch.empty((n,), dtype=torch.uint8, device=dev)            # all three are written in full by the operator
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    count = torch.empty((nf,), dtype=torch.int32, device=dev)
    lib = capi.load()
    thr = -math.inf if score_threshold is None else float(score_threshold)
    with torch.cuda.device(dev):
        ws = capi.workspace(lib.mpnhip_nms_batched_workspace_bytes(n, max(most, 1)), dev, "nms")
        pd = torch.from_numpy(p).to(dev)
        check(lib.mpnhip_nms_batched(ptr(b), ptr(s), ptr(pd), n, nf, max(most, 1), thr, float(iou_threshold), ptr(keep), ptr(order),
                                     ptr(count), ptr(ws), ws.numel(), stream_ptr()), "mpnhip_nms_batched")
    return keep, order, count


def nms_batched(boxes, scores, box_frame, iou_threshold, score_threshold=None):
    """``scores >= score_threshold`` then ``torchvision.ops.nms`` per frame: the kept rows (int64, on the device), frame after
    frame, each frame's in decreasing score (equal scores by increasing row).  ``box_frame`` must be non-decreasing
    (``ValueError``).  Sizing the result reads the device once; ``nms_batched_raw`` does not."""
    _, order, _ = nms_batched_raw(boxes, scores, box_frame, iou_threshold, score_threshold)
    return order[order >= 0].to(torch.int64)


def refine_detections(backbone, heads, frames, det, detect_score_thresh, nms_thresh, frames_index=None, label=1, convs='stock',
                      **transform_kw):
    """``FRCNNPreprocessor.step`` over a batch of frames and the table of ``save_results``: float64 ``[m, 7]`` on the host,
    ``frame, -1, bb_left + 1, bb_top + 1, bb_width, bb_height, conf`` (widths, heights and the + 1 in float32, as the reference's
    float32 columns hold them), frame after frame, each frame's rows in decreasing score.

    ``frames``: uint8 ``[B, H, W, 3]`` on the device; ``det``: the raw detections, a table with ``frame, bb_left, bb_top,
    bb_right, bb_bot``; ``frames_index``: the frame number of every entry of ``B`` (default: the sorted frame numbers of ``det``).
    A frame without detections contributes nothing, as the reference skips it.

    The route: ``embed_inputs.fpn_features`` -> ``predict_boxes`` -> ``nms_batched_raw``.  With ``convs='native'`` nothing is read
    back until the boolean index ``order >= 0`` below, whose size is the sum of ``count``: the one host synchronisation."""
    _check_convs(convs, heads)
    frame = embed_inputs._col(det, "frame", np.int64)
    numbers = np.unique(frame) if frames_index is None else np.asarray(frames_index, np.int64).reshape(-1)
    if numbers.size != int(frames.shape[0]):
        raise ValueError("%d frames for %d frame numbers" % (int(frames.shape[0]), numbers.size))
    by_number = np.argsort(numbers, kind="stable")
    pos = np.searchsorted(numbers[by_number], frame)
    if frame.size and ((pos >= numbers.size).any() or (numbers[by_number][np.minimum(pos, numbers.size - 1)] != frame).any()):
        raise ValueError("a detection lies in a frame that is not given")
    idx = by_number[pos] if frame.size else pos
    rows = np.argsort(idx, kind="stable")                      # the boxes of a frame as consecutive rows, frames in batch order
    boxes = embed_inputs._boxes_of(det, np.float32)[rows]
    idx = idx[rows]
    features, image_size = embed_inputs.fpn_features(backbone, frames, convs=convs, **transform_kw)
    refined, scores = predict_boxes(heads, features, boxes, idx, image_size, (int(frames.shape[1]), int(frames.shape[2])), label, convs)
    _, order, _ = nms_batched_raw(refined, scores, idx, nms_thresh, detect_score_thresh, n_frames=int(frames.shape[0]))
    kept = order[order >= 0].to(torch.int64)                   # the host read: the result's size
    b, s = refined[kept], scores[kept]
    one = torch.ones((), dtype=torch.float32, device=b.device)
    number = torch.from_numpy(numbers[idx]).to(b.device)[kept].to(torch.float64)
    table = torch.stack((number, torch.full_like(number, -1.0), (b[:, 0] + one).double(), (b[:, 1] + one).double(),
                         (b[:, 2] - b[:, 0]).double(), (b[:, 3] - b[:, 1]).double(), s.double()), dim=1)
    return table.cpu().numpy()


def write_det_file(path, table):
    """``save_results``' csv (no header, no index): ``frame, id, bb_left, bb_top, bb_width, bb_height, conf``, the two integers
    as integers, the five float32 values in their shortest form, as pandas writes float32 columns"""
    t = np.asarray(table, np.float64).reshape(-1, 7)
    with open(path, "w") as f:
        for r in t:
            vals = [np.format_float_positional(np.float32(v), unique=True, trim='0') for v in r[2:]]
            f.write("%d,%d,%s\n" % (int(r[0]), int(r[1]), ",".join(vals)))


def nan_roi_masks(backbone, heads, frames, boxes, box_frame, label=1, convs='stock', **transform_kw):
    """What ``MPNTracker._predict_nan_masks`` stores for boxes without a mask: ``load_image`` + ``predict_masks(boxes,
    return_roi_masks=True)`` + ``Upsample(scale_factor=2, mode='bilinear')``: float32 ``[n, 56, 56]`` on the device.
    ``frames``: uint8 ``[B, H, W, 3]`` on the device; ``boxes``, ``box_frame`` as ``predict_boxes``."""
    _check_convs(convs, heads)
    features, image_size = embed_inputs.fpn_features(backbone, frames, convs=convs, **transform_kw)
    masks = predict_masks(heads, features, boxes, box_frame, image_size, (int(frames.shape[1]), int(frames.shape[2])), 2, label, convs)
    return masks[:, 0]
