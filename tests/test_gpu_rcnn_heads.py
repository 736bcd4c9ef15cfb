"""The RoI heads on the device: mpnhip_box_predict and mpnhip_roi_mask_finish against float64 (rcnn_heads_ref.py), the composed
routes of mpntrackseg_amd.rcnn_heads native against the float64 evaluation of the same modules, and refine_detections.

Bounds.  An operator's output is held to max(16 u, 4 x the float32 CPU evaluation's worst error / magnitude) x magnitude, u = 2^-24;
the magnitude is sum |h w| + |b| for a dot product, 1 for a score or a mask value, the box's reach (its largest |coordinate|) for
a coordinate.  A composed route is held to four times the float32 stock route's own worst error on the same inputs, and for scores
and mask values to no less than the operators' 16 u of a magnitude of 1.  Every case prints what it measured."""
import math

import numpy as np
import pytest
import torch

import embed_inputs_ref as ER
import rcnn_heads_cases as K
import rcnn_heads_ref as R
from mpntrackseg_amd import capi, embed_inputs, fpn_net, rcnn_heads as RH, synth

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
U = R.U
RATIO_H, RATIO_W = 1080.0 / 749.0, 1920.0 / 1333.0


def dev():
    return torch.device("cuda:0")


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Predictor:
    """what box_predict_native reads of a FastRCNNPredictor"""

    def __init__(self, wc, bc, wb, bb):
        lin = lambda w, b: type("L", (), dict(weight=D(w), bias=D(b)))
        self.cls_score, self.bbox_pred = lin(wc, bc), lin(wb, bb)


def box_case(seed, n, k, c, label, big_bias=False):
    h = np.maximum(synth.normal(seed, (n, k), stream=0), 0)
    wc, bc = synth.normal(seed, (c, k), stream=1, std=1 / math.sqrt(k)), synth.normal(seed, (c,), stream=2, std=0.5)
    wb, bb = synth.normal(seed, (4 * c, k), stream=3, std=1 / math.sqrt(k)), synth.normal(seed, (4 * c,), stream=4, std=0.5)
    if big_bias:
        bb[4 * label + 2] = 30.0          # every width delta of the label is far above the clip
    prop, _ = K.random_boxes(seed + 1000, n, span=1200.0, lo=20.0, hi=300.0)
    return h, wc, bc, wb, bb, prop


def check_box_outputs(got, ref, cpu32, what):
    mags = dict(logits=ref["logit_mag"], deltas=ref["delta_mag"], scores=np.ones_like(ref["scores"]), boxes=R.box_extent(ref["boxes"]))
    worst = {}
    for key, mag in mags.items():
        bound, ratio = R.case_bound(cpu32[key], ref[key], mag)
        err = np.abs(got[key].astype(F64) - ref[key])
        worst[key] = (float((err / (16 * U * mag)).max()), ratio / (16 * U))
        assert (err <= bound).all(), (what, key, worst[key])
    print(what, " ".join("%s %.3f (float32 CPU %.3f) of 16 u" % (k, v[0], v[1]) for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("k", (4, 64, 1024))
def test_box_predict_against_float64(k):
    for c in (2, 3, 91):
        for n in (1, 65, 257):
            label = 1 if c == 2 else (2 if c == 3 else 57)
            h, wc, bc, wb, bb, prop = box_case(k + c + n, n, k, c, label)
            ref = R.box_predict(h, wc, bc, wb, bb, prop, label, ratio_h=RATIO_H, ratio_w=RATIO_W)
            cpu32 = R.box_predict(h, wc, bc, wb, bb, prop, label, ratio_h=RATIO_H, ratio_w=RATIO_W, dtype=F32)
            capi.path_counters(reset=True)
            out = RH.box_predict_native(D(h), Predictor(wc, bc, wb, bb), D(prop), label, (RATIO_H, RATIO_W), return_raw=True)
            torch.cuda.synchronize()
            assert capi.path_counters()["box_predict"] == 1
            got = dict(zip(("boxes", "scores", "logits", "deltas"), (t.cpu().numpy() for t in out)))
            check_box_outputs(got, ref, cpu32, "K %d C %d n %d" % (k, c, n))


def test_box_predict_row_stride_clip_and_batch_independence():
    n, k, c, label = 65, 64, 3, 2
    h, wc, bc, wb, bb, prop = box_case(5, n, k, c, label, big_bias=True)
    pred = Predictor(wc, bc, wb, bb)
    wide = torch.full((n, k + 12), float("nan"), device=dev())
    wide[:, :k] = D(h)
    hv = wide[:, :k]
    assert hv.stride(0) == k + 12
    boxes, scores, logits, deltas = (t.cpu().numpy() for t in RH.box_predict_native(hv, pred, D(prop), label, (RATIO_H, RATIO_W), return_raw=True))
    dense = [t.cpu().numpy() for t in RH.box_predict_native(D(h), pred, D(prop), label, (RATIO_H, RATIO_W), return_raw=True)]
    for a, b in zip((boxes, scores, logits, deltas), dense):
        assert np.array_equal(a, b)
    ref = R.box_predict(h, wc, bc, wb, bb, prop, label, ratio_h=RATIO_H, ratio_w=RATIO_W)
    cpu32 = R.box_predict(h, wc, bc, wb, bb, prop, label, ratio_h=RATIO_H, ratio_w=RATIO_W, dtype=F32)
    check_box_outputs(dict(boxes=boxes, scores=scores, logits=logits, deltas=deltas), ref, cpu32, "wide rows, clipped")
    # a delta above the clip is decoded at the clip: the width is exp(clip) times the proposal's, whatever the delta
    clip = F32(R.CLIP)
    assert (deltas[:, 2] / F32(5) > clip).all()
    want_w = np.exp(F64(clip)) * (prop[:, 2].astype(F64) - prop[:, 0]) * F64(F32(RATIO_W))
    assert np.allclose(boxes[:, 2].astype(F64) - boxes[:, 0], want_w, rtol=1e-5)
    # box k alone equals box k in the batch, bit for bit
    for kk in (0, 3, 63, 64):
        alone = RH.box_predict_native(D(h[kk:kk + 1]), pred, D(prop[kk:kk + 1]), label, (RATIO_H, RATIO_W), return_raw=True)
        for a, b in zip(alone, (boxes, scores, logits, deltas)):
            assert np.array_equal(a.cpu().numpy()[0], b[kk]), kk


@pytest.mark.parametrize("S", (1, 2, 28))
def test_roi_mask_finish_against_float64(S):
    n = 5
    for C in (1, 2):
        label = C - 1
        z = synth.normal(40 + S, (n, C, S, S), stream=C, std=3.0)
        wide = torch.full((n, C * S * S + 20), float("nan"), device=dev())
        wide[:, :C * S * S] = D(z).reshape(n, -1)
        strided = torch.as_strided(wide, (n, C, S, S), (C * S * S + 20, S * S, S, 1))
        for up in (1, 2):
            ref = R.roi_mask_finish(z, label, up)
            cpu32 = R.roi_mask_finish(z, label, up, dtype=F32)
            bound, ratio = R.case_bound(cpu32, ref, np.ones_like(ref))
            capi.path_counters(reset=True)
            got = RH.roi_mask_finish_native(D(z), label, up).cpu().numpy()
            assert capi.path_counters()["roi_mask_finish"] == 1
            again = RH.roi_mask_finish_native(strided, label, up).cpu().numpy()
            assert got.shape == (n, S * up, S * up) and np.array_equal(got, again)
            err = np.abs(got.astype(F64) - ref)
            print("S %d C %d up %d: %.3f (float32 CPU %.3f) of 16 u" % (S, C, up, err.max() / (16 * U), ratio / (16 * U)))
            assert (err <= bound).all()
            if up == 2:
                # the corners are the sigmoid of the corner logits (both source indices clamped or weight 0), and the edge rows
                # interpolate along the edge only
                p = R.sigmoid(z[:, label].astype(F64))
                for (y, x), (sy, sx) in (((0, 0), (0, 0)), ((0, -1), (0, -1)), ((-1, 0), (-1, 0)), ((-1, -1), (-1, -1))):
                    assert np.abs(got[:, y, x] - p[:, sy, sx]).max() <= 16 * U
                if S > 1:
                    edge = 0.75 * p[:, 0, 0] + 0.25 * p[:, 0, 1]
                    assert np.abs(got[:, 0, 1] - edge).max() <= 16 * U and np.abs(got[:, 1, 0] - (0.75 * p[:, 0, 0] + 0.25 * p[:, 1, 0])).max() <= 16 * U
                    assert np.abs(got[:, -1, -2] - (0.75 * p[:, -1, -1] + 0.25 * p[:, -1, -2])).max() <= 16 * U


# ------------------------------------------------------------------------------------------------ composed routes
def composed_case(heads_kw, seed, n):
    heads = RH.RoIHeads(**heads_kw).eval()
    W = synth.make_roi_head_weights(heads, seed)
    feats = K.pyramid(seed + 1, heads_kw["channels"])
    boxes, frame = K.boxes_on_frames(seed + 2, n)
    return heads.to(dev()), W, feats, boxes, frame


def reference_routes(W, feats, boxes, frame):
    net = ER.resize_boxes(boxes, K.ORIGINAL_SIZE, K.IMAGE_SIZE)
    rh, rw = RH.back_ratios(K.IMAGE_SIZE, K.ORIGINAL_SIZE)
    p7, _ = ER.fpn_roi_align(feats, net, frame, K.IMAGE_SIZE, None, 7, 2, acc=F64)
    p14, _ = ER.fpn_roi_align(feats, net, frame, K.IMAGE_SIZE, None, 14, 2, acc=F64)
    box = R.box_branch(p7, W, net, 1, rh, rw)
    refined = R.box_branch(p7, W, net, 1)["boxes"]
    q14, _ = ER.fpn_roi_align(feats, refined.astype(F32), frame, K.IMAGE_SIZE, None, 14, 2, acc=F64)
    return dict(boxes=box["boxes"], scores=box["scores"], masks1=R.mask_branch(p14, W, 1, 1), masks2=R.mask_branch(p14, W, 1, 2),
                refined_masks=R.mask_branch(q14, W, 1, 1))


def hold(native, stock, ref, what, floor=0.0):
    """``floor``: 16 u of the output's magnitude where that is known beforehand (1 for a score or a mask value), so that the bound
    does not shrink with a stock route that happens to be exact"""
    e_native, e_stock = float(np.abs(native.astype(F64) - ref).max()), float(np.abs(stock.astype(F64) - ref).max())
    bound = max(floor, 4 * e_stock)
    print("%s: native %.3g, float32 stock %.3g, bound max(%.3g, 4 x stock) = %.3g" % (what, e_native, e_stock, floor, bound))
    assert native.shape == ref.shape and e_native <= bound, what
    return e_native, e_stock


NATIVE_MASK = dict(conv_affine_tile=4, conv_transpose=1, conv_small_cout=1, roi_mask_finish=1)


def counted(fn):
    capi.path_counters(reset=True)
    out = fn()
    torch.cuda.synchronize()
    return out, {k: v for k, v in capi.path_counters().items() if v}


@pytest.fixture(scope="module")
def small_case():
    heads, W, feats, boxes, frame = composed_case(dict(K.SMALL), 21, 9)
    return heads, [D(f) for f in feats], boxes, frame, reference_routes(W, feats, boxes, frame)


def test_predict_boxes_native(small_case):
    heads, tf, boxes, frame, ref = small_case
    args = (heads, tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE)
    (nb, ns), c = counted(lambda: RH.predict_boxes(*args, convs='native'))
    assert c.get("box_predict") == 1 and sum(v for k, v in c.items() if k.startswith("gemm")) == 2, c
    sb, ss = RH.predict_boxes(*args)
    hold(nb.cpu().numpy(), sb.cpu().numpy(), ref["boxes"], "predict_boxes boxes")
    hold(ns.cpu().numpy(), ss.cpu().numpy(), ref["scores"], "predict_boxes scores", 16 * U)


@pytest.mark.parametrize("up", (1, 2))
def test_predict_masks_native(small_case, up):
    heads, tf, boxes, frame, ref = small_case
    args = (heads, tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE)
    nm, c = counted(lambda: RH.predict_masks(*args, upsample=up, convs='native'))
    assert all(c.get(k) == v for k, v in NATIVE_MASK.items()) and "conv_tile" not in c and "box_predict" not in c, c
    sm, cs = counted(lambda: RH.predict_masks(*args, upsample=up))
    assert not any(k.startswith("conv") or k == "roi_mask_finish" for k in cs), cs      # the stock route ran no native convolution
    assert tuple(nm.shape) == (9, 1, 28 * up, 28 * up)
    hold(nm.cpu().numpy(), sm.cpu().numpy(), ref["masks%d" % up], "predict_masks up %d" % up, 16 * U)


def test_predict_native(small_case):
    heads, tf, boxes, frame, ref = small_case
    args = (heads, tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE)
    (nb, ns, nm), c = counted(lambda: RH.predict(*args, convs='native'))
    assert c.get("box_predict") == 1 and all(c.get(k) == v for k, v in NATIVE_MASK.items()) and "conv_tile" not in c, c
    sb, ss, sm = RH.predict(*args)
    hold(nb.cpu().numpy(), sb.cpu().numpy(), ref["boxes"], "predict boxes")
    hold(ns.cpu().numpy(), ss.cpu().numpy(), ref["scores"], "predict scores", 16 * U)
    hold(nm.cpu().numpy(), sm.cpu().numpy(), ref["refined_masks"], "predict masks on the refined boxes", 16 * U)
    heads.train()
    with pytest.raises(capi.MpnhipError):
        RH.predict(*args, convs='native')
    heads.eval()


def test_true_sizes_three_boxes():
    """256 channels, 12544 -> 1024 -> 1024, 2 classes"""
    heads, W, feats, boxes, frame = composed_case(dict(channels=256, representation_size=1024), 31, 3)
    tf, ref = [D(f) for f in feats], reference_routes(W, feats, boxes, frame)
    args = (heads, tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE)
    (nb, ns, nm), c = counted(lambda: RH.predict(*args, convs='native'))
    assert c.get("box_predict") == 1 and all(c.get(k) == v for k, v in NATIVE_MASK.items()) and "conv_tile" not in c, c
    sb, ss, sm = RH.predict(*args)
    hold(nb.cpu().numpy(), sb.cpu().numpy(), ref["boxes"], "true sizes: boxes")
    hold(ns.cpu().numpy(), ss.cpu().numpy(), ref["scores"], "true sizes: scores", 16 * U)
    hold(nm.cpu().numpy(), sm.cpu().numpy(), ref["refined_masks"], "true sizes: masks", 16 * U)


# ------------------------------------------------------------------------------------------------ refine_detections
def test_refine_detections_native():
    torch.manual_seed(0)
    backbone = fpn_net.resnet50_fpn_backbone()
    synth.make_fpn_weights(backbone, 41)
    backbone = backbone.to(dev()).eval()
    heads = RH.RoIHeads(channels=256, representation_size=64).eval()
    W = synth.make_roi_head_weights(heads, 42)
    B, H, Wd = 3, 90, 135
    frames = torch.from_numpy((synth.uniform01(43, B * H * Wd * 3) * 255).astype(np.uint8).reshape(B, H, Wd, 3)).to(dev())
    boxes, idx = K.boxes_on_frames(44, 14, frames=2)
    numbers = np.array([5, 6, 9])                       # frame 6 (the batch's second entry) has no detection
    det_frame = np.where(idx == 0, 5, 9)
    boxes = np.concatenate([boxes, boxes[:3] + F32(0.5)])   # near-duplicates: the NMS has something to remove
    det_frame = np.concatenate([det_frame, det_frame[:3]])
    det = dict(frame=det_frame, bb_left=boxes[:, 0], bb_top=boxes[:, 1], bb_right=boxes[:, 2], bb_bot=boxes[:, 3])
    kw = dict(min_size=64, max_size=96)
    nms_thr = 0.5
    # the float64 side, from the features the device computed
    features, image_size = embed_inputs.fpn_features(backbone, frames, convs='native', **kw)
    feats = [features[k].cpu().numpy() for k in RH.LEVELS]
    rows = np.argsort(np.searchsorted(numbers, det_frame), kind="stable")
    sb, sf = boxes[rows], np.searchsorted(numbers, det_frame)[rows]
    net = ER.resize_boxes(sb, (H, Wd), image_size)
    rh, rw = RH.back_ratios(image_size, (H, Wd))
    p7, _ = ER.fpn_roi_align(feats, net, sf, image_size, None, 7, 2, acc=F64)
    # the synthetic backbone's features are not of unit size: fc6 is scaled by their rms, so that the scores spread over (0, 1)
    W["box_head.fc6.weight"] = (W["box_head.fc6.weight"] / F32(np.sqrt((p7 ** 2).mean()))).astype(F32)
    heads.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    heads = heads.to(dev())
    ref = R.box_branch(p7, W, net, 1, rh, rw)
    cpu32 = R.box_branch(p7, W, net, 1, rh, rw, dtype=F32)
    # conf is the end of a composed route (the pooler and two dense layers of K = 12544 and 64 in float32 before the predictor): it
    # is held as the composed routes are, to max(16 u, 4 x the float32 stock route's own worst score error on these inputs)
    stock_scores = RH.predict_boxes(heads, features, sb, sf, image_size, (H, Wd))[1].cpu().numpy().astype(F64)
    score_bound = np.full_like(ref["scores"], max(16 * U, 4 * float(np.abs(stock_scores - ref["scores"]).max())))
    box_bound, _ = R.case_bound(cpu32["boxes"], ref["boxes"], R.box_extent(ref["boxes"]))
    thresh = float(np.sort(ref["scores"])[len(sf) // 3:len(sf) // 3 + 2].mean())      # between two scores: some detections go
    assert (np.abs(ref["scores"] - thresh) > score_bound).all(), "a score lies within its bound of the threshold"
    margin = []
    want, kept = R.det_table(ref["boxes"].astype(F32), ref["scores"].astype(F32), sf, numbers, thresh, nms_thr, F64)
    for f in np.unique(sf):
        R.nms_frame(ref["boxes"][sf == f], ref["scores"][sf == f], nms_thr, thresh, F64, margin)
    assert margin and min(margin) > 1e-4, "an IoU lies at the threshold"
    table, c = counted(lambda: RH.refine_detections(backbone, heads, frames, det, thresh, nms_thr, frames_index=numbers, convs='native', **kw))
    assert c.get("box_predict") == 1 and c.get("nms_batched") == 1, c
    print("refine_detections: %d of %d detections kept, scores %s" % (len(kept), len(sf), np.round(np.sort(ref["scores"]), 3)))
    assert table.dtype == F64 and table.shape == want.shape and 0 < len(kept) < len(sf)
    assert np.array_equal(table[:, :2], want[:, :2]) and 6 not in table[:, 0] and set(table[:, 0]) == {5.0, 9.0}
    bb = box_bound[kept]
    assert (np.abs(table[:, 2] - (ref["boxes"][kept, 0] + 1)) <= bb[:, 0] + 4 * U * (1 + np.abs(ref["boxes"][kept, 0]))).all()
    assert (np.abs(table[:, 3] - (ref["boxes"][kept, 1] + 1)) <= bb[:, 0] + 4 * U * (1 + np.abs(ref["boxes"][kept, 1]))).all()
    assert (np.abs(table[:, 4] - (ref["boxes"][kept, 2] - ref["boxes"][kept, 0])) <= 3 * bb[:, 0]).all()
    assert (np.abs(table[:, 5] - (ref["boxes"][kept, 3] - ref["boxes"][kept, 1])) <= 3 * bb[:, 0]).all()
    print("conf: native %.3g, bound %.3g" % (np.abs(table[:, 6] - ref["scores"][kept]).max(), score_bound[0]))
    assert (np.abs(table[:, 6] - ref["scores"][kept]) <= score_bound[kept]).all()
    # the stock route decides the same
    stock = RH.refine_detections(backbone, heads, frames, det, thresh, nms_thr, frames_index=numbers, **kw)
    assert np.array_equal(stock[:, :2], table[:, :2]) and np.abs(stock - table).max() < 1e-2
    # nan_roi_masks: the 56 x 56 masks of the same boxes
    m = RH.nan_roi_masks(backbone, heads, frames, sb, sf, convs='native', **kw)
    again = RH.predict_masks(heads, features, sb, sf, image_size, (H, Wd), upsample=2, convs='native')
    assert tuple(m.shape) == (len(sf), 56, 56) and bool(((m >= 0) & (m <= 1)).all()) and torch.equal(m, again[:, 0])
