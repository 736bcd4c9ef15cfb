"""The inputs of the two embedding CNNs of the reference's ``MOTSeqProcessor._store_embeddings``
(``data/seq_processing/seq_processor.py:395-562``), on the device and without ``torchvision`` or ``PIL``.  The Mask R-CNN FPN
backbone is ``fpn_net.BackboneWithFPN`` and the torchreid ResNet50 is ``reid_net.ResNet`` (both: stock modules by default, native
kernels on request); what surrounds them is here:

``transform_sizes``, ``rcnn_transform``   ``GeneralizedRCNNTransform`` for a batch of frames: normalise, resize, pad;
``fpn_features``              ``MaskRCNN_FPN.load_image``: the transform and the backbone (``convs='stock' | 'native'``);
``node_ext_embeddings_from_frames``   frames and detections -> ``x_ext`` in its stored format;

``reid_embeddings``           crops -> the ReID CNN (``convs='stock' | 'native'``) -> node-core maps and ReID vectors;
``store_reid_embeddings``     their per-frame files (``seq_processor.py:443-475``);

``reid_crops``                ``BoundingBoxDataset.__getitem__`` (``utils/rgb.py:40-69``) for all boxes at once: crop,
                              ``np.pad(mode='mean')``, ``PIL.Image.resize`` (bilinear, bit for bit), ``ToTensor``, ``Normalize``;
``fpn_roi_align``             ``MaskRCNN_FPN.get_node_embeddings`` (``tracktor_masked/maskrcnn_fpn.py:108-115``): ``resize_boxes``
                              and ``MultiScaleRoIAlign(['0', '1', '2', '3'], 14, sampling_ratio=2)`` over the four FPN levels;
``node_ext_embeddings``       the same from a detections table, with the detection-id channel of ``seq_processor.py:545-548``;
``store_node_ext_embeddings`` the ``<frame>.pt`` files ``embeddings.load_precomputed_embeddings(..., '3D')`` reads back.

The operators are ``csrc/embed_inputs.hip`` (``include/mpnhip.h`` states their arithmetic).  What is cheap and per box stays on the
host, in the reference's own number formats: the crop geometry in numpy float64 (eight integers per box), the box mapping, the
level scales and the level of every box in torch float32.  There is no CPU fallback.

The level mapper adds its ``eps = 1e-6`` outside the logarithm, ``floor(4 + log2(s / 224) + 1e-6)``: torchvision 0.6.0's form as
far as known here -- torchvision was not at hand to confirm it.  Later releases add it inside the logarithm; the two differ only
for boxes within 1e-6 of a level boundary."""
import ctypes as C
import math
import os.path as osp

import numpy as np
import torch

from . import capi
from .capi import MpnhipError, check, ptr, stream_ptr

CROP_MAX_SIDE = 8192              # MPNHIP_CROP_MAX_SIDE
FPN_MAX_SAMPLES = 1024            # MPNHIP_FPN_MAX_SAMPLES
BOX_LTRB = ("bb_left", "bb_top", "bb_right", "bb_bot")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CANONICAL_SCALE, CANONICAL_LEVEL, LEVEL_EPS = 224, 4, 1e-6   # torchvision's LevelMapper


def _col(rows, name, dtype=None):
    v = rows[name]
    v = np.asarray(v.values if hasattr(v, "values") else v).reshape(-1)
    return v if dtype is None else v.astype(dtype)


def _boxes_of(boxes, dtype):
    """[n, 4] (left, top, right, bottom) from an array or from a table with the columns ``bb_left, bb_top, bb_right, bb_bot``"""
    if hasattr(boxes, "keys") or hasattr(boxes, "columns"):
        return np.stack([_col(boxes, c, dtype) for c in BOX_LTRB], axis=1)
    return np.ascontiguousarray(np.asarray(boxes, dtype=dtype).reshape(-1, 4))


def _frame_index(box_frame, n, n_frames):
    idx = np.asarray(box_frame).reshape(-1)
    if idx.size != n:
        raise ValueError("one frame index per box: %d for %d boxes" % (idx.size, n))
    if idx.size and (not np.issubdtype(idx.dtype, np.integer) or idx.min() < 0 or idx.max() >= n_frames):
        raise ValueError("box_frame must hold integers in [0, %d)" % n_frames)
    return idx.astype(np.int32)


def _dev(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


# ------------------------------------------------------------------------------------------------ ReID patches
def crop_geometry(boxes, H, W, pad=True):
    """The crop and the pads of ``rgb.py:51-60`` for boxes [n, 4] (float64: left, top, right, bottom) in an ``H x W`` frame, in
    numpy float64 with the reference's expressions: int32 [n, 8] = ``y0, y1, x0, x1`` (the crop is rows ``[y0, y1)`` and columns
    ``[x0, x1)``, clipped to the frame as a numpy slice clips) and ``pt, pb, pl, pr`` (all 0 with ``pad=False``).  Raises
    ``ValueError`` for a box that is not finite, an empty crop and a padded side above ``CROP_MAX_SIDE``."""
    b = _boxes_of(boxes, np.float64)
    if not np.isfinite(b).all():
        raise ValueError("box %d is not finite" % int(np.flatnonzero(~np.isfinite(b).all(axis=1))[0]))
    left, top, right, bot = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    start = lambda v, size: np.minimum(np.trunc(np.maximum(0, v)), size)          # int(max(0, v)), then the slice's clip
    g = np.zeros((b.shape[0], 8), np.float64)
    g[:, 0], g[:, 1], g[:, 2], g[:, 3] = start(top, H), start(bot, H), start(left, W), start(right, W)
    if pad:
        g[:, 4] = np.trunc(np.abs(top - np.maximum(top, 0)))
        g[:, 5] = np.trunc(np.abs(bot - np.minimum(bot, H)))
        g[:, 6] = np.trunc(np.abs(left - np.maximum(left, 0)))
        g[:, 7] = np.trunc(np.abs(right - np.minimum(right, W)))
    empty = (g[:, 1] <= g[:, 0]) | (g[:, 3] <= g[:, 2])
    if empty.any():
        k = int(np.flatnonzero(empty)[0])
        raise ValueError("box %d (%s) has an empty crop in a %d x %d frame" % (k, ", ".join("%g" % v for v in b[k]), H, W))
    side = np.maximum(g[:, 4] + (g[:, 1] - g[:, 0]) + g[:, 5], g[:, 6] + (g[:, 3] - g[:, 2]) + g[:, 7])
    if (side > CROP_MAX_SIDE).any():
        raise ValueError("the padded crop of box %d has a side above %d pixels (MPNHIP_CROP_MAX_SIDE)"
                         % (int(np.flatnonzero(side > CROP_MAX_SIDE)[0]), CROP_MAX_SIDE))
    return g.astype(np.int32)


def reid_crops(frames, boxes, box_frame, output_size=(128, 64), pad=True, mean=IMAGENET_MEAN, std=IMAGENET_STD, return_uint8=False,
               boxes_per_launch=1024):
    """The ReID CNN's input patches, float32 ``[n, 3, oh, ow]`` on the device of ``frames``.

    ``frames``: uint8 ``[B, H, W, 3]`` on the device, the frames as ``imread`` returns them (uploaded once, shared by all their
    boxes); ``boxes``: ``[n, 4]`` = ``bb_left, bb_top, bb_right, bb_bot`` as float64 numpy, or a table with those columns;
    ``box_frame``: ``[n]`` indices into ``B``, in any order.  ``pad``, ``output_size``, ``mean``, ``std``: ``BoundingBoxDataset``'s
    ``pad_``, ``output_size`` and its ``Normalize``.  ``return_uint8`` (debugging): also the resized patches before ``ToTensor``,
    uint8 ``[n, oh, ow, 3]`` -- what ``np.asarray(PIL image)`` is in the reference.  ``boxes_per_launch`` bounds the workspace;
    the result does not depend on it.  Raises ``ValueError`` before any launch for an empty crop, a box that is not finite, a
    ``box_frame`` outside ``[0, B)`` and a padded side above ``CROP_MAX_SIDE``."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise MpnhipError("frames must be a uint8 tensor [B, H, W, 3]")
    dev = frames.device
    B, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    oh, ow = int(output_size[0]), int(output_size[1])
    if not (1 <= oh <= CROP_MAX_SIDE and 1 <= ow <= CROP_MAX_SIDE):
        raise ValueError("output_size must lie in [1, %d]" % CROP_MAX_SIDE)
    geom = crop_geometry(boxes, H, W, pad)
    n = geom.shape[0]
    idx = _frame_index(box_frame, n, B)
    capi.require_device(frames)   # (after the boxes: what is wrong with them is reported without a device)
    lib = capi.load()
    mean_std = (C.c_float * 6)(*[float(v) for v in tuple(mean) + tuple(std)])
    step = max(int(boxes_per_launch), 1)
    with torch.cuda.device(dev):
        frames = frames.contiguous()
        out = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=dev)
        u8 = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev) if return_uint8 else None
        for k0 in range(0, n, step):
            g = geom[k0:k0 + step]
            m = g.shape[0]
            max_ph = int((g[:, 4] + g[:, 1] - g[:, 0] + g[:, 5]).max())
            max_pw = int((g[:, 6] + g[:, 3] - g[:, 2] + g[:, 7]).max())
            ws = capi.workspace(lib.mpnhip_reid_crops_workspace_bytes(m, max_ph, max_pw, oh, ow), dev, "reid_crops")
            gd, fd = _dev(g, np.int32, dev), _dev(idx[k0:k0 + step], np.int32, dev)
            check(lib.mpnhip_reid_crops(ptr(frames), B, H, W, ptr(gd), ptr(fd), m, max_ph, max_pw, oh, ow, mean_std, ptr(out[k0:k0 + m]),
                                        ptr(u8[k0:k0 + m]) if return_uint8 else None, ptr(ws), ws.numel(), stream_ptr()), "mpnhip_reid_crops")
    return (out, u8) if return_uint8 else out


def reid_embeddings(net, frames, det, box_frame, convs='stock', batch_size=1000):
    """The ReID CNN over the detections ``det`` (``seq_processor.py:411-441``): ``reid_crops`` -> ``net`` (a
    ``reid_net.ResNet`` in eval mode on the device of ``frames``) -> ``(node_core [n, 2048, 8, 4], reid [n, 256])`` on the device.
    ``convs='stock'`` (the default) runs ``net.forward`` -- the stock modules -- under ``no_grad`` in batches of ``batch_size``
    (the reference's ``img_batch_size``); ``convs='native'`` runs ``net.forward_native`` (csrc/conv_strided.hip) in slices of
    ``batch_size``.  ``frames``, ``det`` (boxes or a table with the ``bb_*`` columns) and ``box_frame`` as for ``reid_crops``.
    No detections give empty tensors of the right shapes on both routes."""
    if convs not in ('stock', 'native'):
        raise ValueError("convs must be 'stock' or 'native', not %r" % (convs,))
    crops = reid_crops(frames, det, box_frame)
    step = max(int(batch_size), 1)
    if crops.shape[0] == 0:                 # no detections: empty results on either route, the network is not run
        fshape, width = net.output_shapes(int(crops.shape[2]), int(crops.shape[3]))
        return crops.new_empty((0,) + tuple(fshape)), crops.new_empty((0, width))
    if convs == 'native':
        return net.forward_native(crops, max_images=step)
    with torch.no_grad():
        parts = [net(crops[k0:k0 + step]) for k0 in range(0, crops.shape[0], step)]
    return torch.cat([p[0] for p in parts], dim=0), torch.cat([p[1] for p in parts], dim=0)


def store_reid_embeddings(seq_path, det_file_name, reid_dir, node_core_dir, frame, detection_id, node_core, reid):
    """The files of ``seq_processor.py:443-475``: ``<seq_path>/processed_data/embeddings/<det_file_name>/<reid_dir>/<frame>.pt``
    ([n_f, 1 + 256], the detection id in column 0) and ``.../<node_core_dir>/<frame>.pt`` ([n_f, 1 + 2048, 8, 4], the id
    broadcast into channel 0), through ``embeddings.write_frame_embeddings``.  A directory that exists is removed first, as the
    reference does.  Returns the two directories relative to ``processed_data``: the ``embeddings_dir`` arguments of
    ``embeddings.load_precomputed_embeddings(..., '1D')`` and ``(..., '3D')``."""
    import shutil
    from .embeddings import write_frame_embeddings
    frame = np.asarray(frame).reshape(-1)
    ids = np.asarray(detection_id).reshape(-1)
    reid, node_core = torch.as_tensor(reid).detach(), torch.as_tensor(node_core).detach()
    if reid.dim() != 2 or node_core.dim() != 4 or not (reid.shape[0] == node_core.shape[0] == frame.size == ids.size):
        raise MpnhipError("reid [n, D] and node_core [n, C, H, W] need one row per entry of frame and detection_id")
    rels = []
    for sub, emb in ((reid_dir, reid), (node_core_dir, node_core)):
        rel = osp.join("embeddings", det_file_name, sub)
        d = osp.join(seq_path, "processed_data", rel)
        if osp.exists(d):
            shutil.rmtree(d)
        write_frame_embeddings(seq_path, rel, frame, ids, emb.float().cpu())
        rels.append(rel)
    return tuple(rels)


# ------------------------------------------------------------------------------------------------ FPN RoIAlign
def resize_boxes(boxes, original_size, image_size):
    """torchvision's ``resize_boxes`` in torch float32, on the device of ``boxes`` (the host for an array): boxes [n, 4] of a frame
    of ``original_size`` (H, W) mapped into the network's image of ``image_size``"""
    b = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    ratio_h, ratio_w = (torch.tensor(float(s), dtype=torch.float32) / torch.tensor(float(o), dtype=torch.float32)
                        for s, o in zip(image_size, original_size))
    return torch.stack((b[:, 0] * ratio_w, b[:, 1] * ratio_h, b[:, 2] * ratio_w, b[:, 3] * ratio_h), dim=1)


def level_scales(level_shapes, image_size):
    """``MultiScaleRoIAlign``'s scale of every level, ``2 ** round(log2(size / image size))``; the heights and the widths must give
    the same one (``ValueError``)"""
    scales = []
    for h, w in level_shapes:
        sh, sw = (2.0 ** round(math.log2(float(s) / float(i))) for s, i in zip((h, w), image_size))
        if sh != sw:
            raise ValueError("a level of %d x %d has no one scale in an image of %d x %d (%g from the heights, %g from the widths)"
                             % (h, w, image_size[0], image_size[1], sh, sw))
        scales.append(sh)
    return scales


def box_levels(boxes, k_min=2, k_max=5):
    """torchvision 0.6.0's ``LevelMapper`` in torch float32, on the device of ``boxes`` (the host for an array; ``rcnn_heads`` maps
    refined boxes where they are): ``floor(4 + log2(sqrt(area) / 224) + 1e-6)`` clamped to
    ``[k_min, k_max]``, minus ``k_min`` (int64 [n])"""
    b = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    s = torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    k = torch.floor(CANONICAL_LEVEL + torch.log2(s / CANONICAL_SCALE) + torch.tensor(LEVEL_EPS, dtype=torch.float32))
    return torch.clamp(k, min=k_min, max=k_max).to(torch.int64) - k_min


def _check_features(features):
    if len(features) != capi.FPN_LEVELS:
        raise MpnhipError("features must be the backbone's four levels '0' .. '3' (%d given)" % len(features))
    f0 = features[0]
    for f in features:
        if not isinstance(f, torch.Tensor) or f.dtype != torch.float32 or f.dim() != 4:
            raise MpnhipError("every level must be a float32 tensor [B, C, h, w]")
        if f.device != f0.device or f.shape[:2] != f0.shape[:2]:
            raise MpnhipError("the levels must share their device, frames and channels")
    return f0.device, int(f0.shape[0]), int(f0.shape[1])


def map_boxes(boxes, level_shapes, image_size, original_size=None):
    """The host side of ``fpn_roi_align``: ``(boxes in the network's image [n, 4] float32, scales, level of every box)``.  Raises
    ``ValueError`` for a box that is not finite or has ``x2 < x1`` or ``y2 < y1``, and for levels without one scale."""
    b = torch.from_numpy(_boxes_of(boxes, np.float32))
    bad = ~torch.isfinite(b).all(dim=1)
    if bool(bad.any()):
        raise ValueError("box %d is not finite" % int(torch.nonzero(bad)[0]))
    bad = (b[:, 2] < b[:, 0]) | (b[:, 3] < b[:, 1])
    if bool(bad.any()):
        raise ValueError("box %d has x2 < x1 or y2 < y1" % int(torch.nonzero(bad)[0]))
    scales = level_scales(level_shapes, image_size)
    if original_size is not None:
        b = resize_boxes(b, original_size, image_size)
    k_min, k_max = int(-math.log2(scales[0])), int(-math.log2(scales[-1]))
    return b.contiguous(), scales, box_levels(b, k_min, k_max)


def fpn_roi_align(features, boxes, box_frame, image_size, original_size=None, output_size=14, sampling_ratio=2, detection_id=None):
    """``MultiScaleRoIAlign`` over the four FPN levels, float32 ``[n, C (+ 1), S, S]`` on the features' device.

    ``features``: four float32 NCHW tensors ``[B, C, h_l, w_l]`` on the device, the backbone's levels ``'0' .. '3'`` in that order
    (the ``'pool'`` level is not passed); ``boxes``: ``[n, 4]`` (left, top, right, bottom) or a table with the ``bb_*`` columns;
    ``box_frame``: ``[n]`` indices into ``B``; ``image_size``: ``(H, W)`` of the network's resized image
    (``preprocessed_images.image_sizes[0]``); ``original_size``: the frame's own ``(H, W)`` -- when given, the boxes are first
    mapped as ``resize_boxes`` maps them.  ``detection_id`` (ints in ``[0, 2^24)``): when given, channel 0 of the result holds
    the ids, the stored format of ``seq_processor.py:545-548``."""
    dev, B, channels = _check_features(features)
    S, grid = int(output_size), int(sampling_ratio)
    if S < 1 or grid < 1 or S * grid > FPN_MAX_SAMPLES:
        raise ValueError("output_size and sampling_ratio must be positive, their product at most %d" % FPN_MAX_SAMPLES)
    b, scales, levels = map_boxes(boxes, [f.shape[2:] for f in features], image_size, original_size)
    n = b.shape[0]
    idx = _frame_index(box_frame, n, B)
    ids = None
    if detection_id is not None:
        ids = np.asarray(detection_id).reshape(-1)
        if ids.size != n:
            raise ValueError("one detection id per box")
        if ids.size and (not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= 2 ** 24):
            raise ValueError("detection ids must be integers in [0, 2^24) (they are stored as float32)")
    capi.require_device(*features)   # (after the boxes: what is wrong with them is reported without a device)
    lib = capi.load()
    lv = capi.FpnLevels()
    with torch.cuda.device(dev):
        feats = [f.contiguous() for f in features]
        for l, f in enumerate(feats):
            lv.data[l], lv.h[l], lv.w[l], lv.scale[l] = f.data_ptr(), int(f.shape[2]), int(f.shape[3]), scales[l]
        out = torch.empty((n, channels + (0 if ids is None else 1), S, S), dtype=torch.float32, device=dev)
        bd, fd, ld = b.to(dev), _dev(idx, np.int32, dev), levels.to(torch.int32).to(dev)
        idd = None if ids is None else _dev(ids, np.int32, dev)
        check(lib.mpnhip_fpn_roi_align(C.byref(lv), B, channels, ptr(bd), ptr(fd), ptr(ld), n, S, grid, ptr(idd), ptr(out), stream_ptr()),
              "mpnhip_fpn_roi_align")
    return out


def node_ext_embeddings(features, det, image_size, original_size=None, frames=None, output_size=14, sampling_ratio=2):
    """``x_ext`` in its stored format for the detections ``det`` of the frames whose features are given: float32
    ``[n, 1 + C, S, S]``, one row per row of ``det``, the detection id in channel 0.  ``det``: a table with ``bb_left, bb_top,
    bb_right, bb_bot``, ``detection_id`` and ``frame``; ``frames``: the frame number of every entry of ``B`` (default: the sorted
    frame numbers of ``det``)."""
    frame = _col(det, "frame", np.int64)
    frames = np.unique(frame) if frames is None else np.asarray(frames, np.int64).reshape(-1)
    order = np.argsort(frames, kind="stable")
    pos = np.searchsorted(frames[order], frame)
    if frame.size and ((pos >= frames.size).any() or (frames[order][np.minimum(pos, frames.size - 1)] != frame).any()):
        raise ValueError("a detection lies in a frame whose features are not given")
    return fpn_roi_align(features, det, order[pos] if frame.size else pos, image_size, original_size, output_size, sampling_ratio,
                         _col(det, "detection_id", np.int64))


# ------------------------------------------------------------------------------------------------ the FPN backbone's input
def transform_sizes(H, W, min_size=800, max_size=1333, size_divisible=32):
    """``GeneralizedRCNNTransform``'s sizes for an ``H x W`` frame, in Python floats exactly as torchvision 0.6.0 computes them:
    ``(oh, ow, Hp, Wp)`` -- the resized image (the floor of the scaled sides: 1080 x 1920 gives 749, not 750, rows) and the batch
    padded to multiples of ``size_divisible``."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or min_size < 1 or max_size < 1 or size_divisible < 1:
        raise ValueError("sizes must be positive")
    s = float(min_size) / float(min(H, W))
    if float(max(H, W)) * s > float(max_size):
        s = float(max_size) / float(max(H, W))
    oh, ow = int(math.floor(float(H) * s)), int(math.floor(float(W) * s))
    if oh < 1 or ow < 1:
        raise ValueError("a %d x %d frame resizes to nothing" % (H, W))
    d = int(size_divisible)
    return oh, ow, int(math.ceil(float(oh) / d) * d), int(math.ceil(float(ow) / d) * d)


def rcnn_transform(frames, min_size=800, max_size=1333, mean=IMAGENET_MEAN, std=IMAGENET_STD, size_divisible=32):
    """``GeneralizedRCNNTransform.forward`` (``maskrcnn_fpn.py:81-92``) for equally sized frames in one launch
    (``mpnhip_rcnn_transform``, whose header comment states the arithmetic): ``(batch, image_size)`` -- float32
    ``[B, 3, Hp, Wp]`` on the device of ``frames``, normalised, resized to ``image_size = (oh, ow)`` and zero-padded.
    ``frames``: uint8 ``[B, H, W, 3]`` on the device, as for ``reid_crops``.  The resize takes its scale from the output size,
    as torch 1.5.0 does for a float ``scale_factor`` (``F.interpolate(size=(oh, ow))`` in later releases)."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise MpnhipError("frames must be a uint8 tensor [B, H, W, 3]")
    B, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    oh, ow, hp, wp = transform_sizes(H, W, min_size, max_size, size_divisible)
    capi.require_device(frames)
    mean_std = (C.c_float * 6)(*[float(v) for v in tuple(mean) + tuple(std)])
    with torch.cuda.device(frames.device):
        frames = frames.contiguous()
        out = torch.empty((B, 3, hp, wp), dtype=torch.float32, device=frames.device)
        check(capi.load().mpnhip_rcnn_transform(ptr(frames), B, H, W, oh, ow, hp, wp, mean_std, ptr(out), stream_ptr()),
              "mpnhip_rcnn_transform")
    return out, (oh, ow)


def fpn_features(backbone, frames, convs='stock', **transform_kw):
    """``MaskRCNN_FPN.load_image`` for a batch of frames: ``rcnn_transform`` -> ``backbone`` (a ``fpn_net.BackboneWithFPN`` in
    eval mode on the device of ``frames``) -> ``(features, image_size)``, the ordered dict ``'0' .. '3', 'pool'`` and the
    resized image's ``(oh, ow)``.  ``convs='stock'`` (the default) runs ``backbone.forward`` -- the stock modules -- under
    ``no_grad``; ``convs='native'`` runs ``backbone.forward_native`` (csrc/conv_strided.hip).  ``transform_kw``:
    ``rcnn_transform``'s keywords."""
    if convs not in ('stock', 'native'):
        raise ValueError("convs must be 'stock' or 'native', not %r" % (convs,))
    batch, image_size = rcnn_transform(frames, **transform_kw)
    if convs == 'native':
        return backbone.forward_native(batch), image_size
    with torch.no_grad():
        return backbone(batch), image_size


def node_ext_embeddings_from_frames(backbone, frames, det, convs='stock', frames_index=None, output_size=14, sampling_ratio=2,
                                    **transform_kw):
    """``load_image`` + ``get_node_embeddings`` + the id channel (``seq_processor.py:498-548``) for a batch of frames:
    ``fpn_features`` -> ``node_ext_embeddings`` with ``original_size=(H, W)``.  ``frames``: uint8 ``[B, H, W, 3]`` on the device;
    ``det``: the detections table of ``node_ext_embeddings``; ``frames_index``: the frame number of every entry of ``B``
    (default: the sorted frame numbers of ``det``).  Returns float32 ``[n, 1 + 256, S, S]``."""
    features, image_size = fpn_features(backbone, frames, convs=convs, **transform_kw)
    return node_ext_embeddings([features[k] for k in ('0', '1', '2', '3')], det, image_size,
                               original_size=(int(frames.shape[1]), int(frames.shape[2])), frames=frames_index, output_size=output_size,
                               sampling_ratio=sampling_ratio)


def store_node_ext_embeddings(seq_path, det_file_name, embeddings_dir, frame, embeddings):
    """The files of ``seq_processor.py:498-557``: ``<seq_path>/processed_data/embeddings/<det_file_name>/<embeddings_dir>/<frame>.pt``
    holding the rows of ``embeddings`` (``node_ext_embeddings``'s ``[n, 1 + C, S, S]``, the id channel included) of that frame.
    ``frame``: [n] ints.  Returns the directory relative to ``processed_data``: the ``embeddings_dir`` argument of
    ``embeddings.load_precomputed_embeddings(..., embedding_dim='3D')``."""
    import os
    rel = osp.join("embeddings", det_file_name, embeddings_dir)
    d = osp.join(seq_path, "processed_data", rel)
    os.makedirs(d, exist_ok=True)
    frame = np.asarray(frame).reshape(-1)
    emb = torch.as_tensor(embeddings).detach().float().cpu()
    if emb.dim() != 4 or emb.shape[0] != frame.size:
        raise MpnhipError("embeddings [n, 1 + C, S, S] need one row per entry of frame")
    for f in np.unique(frame):
        torch.save(emb[torch.from_numpy(np.flatnonzero(frame == f))].clone(), osp.join(d, "%d.pt" % int(f)))
    return rel
