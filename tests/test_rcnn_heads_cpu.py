"""The RoI heads without a GPU: the numpy references of ``rcnn_heads_ref.py`` pinned against float64 torch, the modules' key names
and checkpoint loading, the host refusals of the three entry points through the built library (everything returns before a
kernel is launched: the non-null pointers are host dummies that are never followed), the agreement of the float32 and float64
NMS references on every input the GPU test uses, and the stock route of the public functions against the references."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import embed_inputs_ref as ER
import rcnn_heads_cases as K
import rcnn_heads_ref as R
from mpntrackseg_amd import capi, rcnn_heads as RH, synth

F32, F64 = np.float32, np.float64
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))

TORCHVISION_KEYS = [
    "box_head.fc6.weight", "box_head.fc6.bias", "box_head.fc7.weight", "box_head.fc7.bias",
    "box_predictor.cls_score.weight", "box_predictor.cls_score.bias", "box_predictor.bbox_pred.weight", "box_predictor.bbox_pred.bias",
    "mask_head.mask_fcn1.weight", "mask_head.mask_fcn1.bias", "mask_head.mask_fcn2.weight", "mask_head.mask_fcn2.bias",
    "mask_head.mask_fcn3.weight", "mask_head.mask_fcn3.bias", "mask_head.mask_fcn4.weight", "mask_head.mask_fcn4.bias",
    "mask_predictor.conv5_mask.weight", "mask_predictor.conv5_mask.bias",
    "mask_predictor.mask_fcn_logits.weight", "mask_predictor.mask_fcn_logits.bias",
]


# ------------------------------------------------------------------------------------------------ the references against torch
def test_box_reference_against_float64_torch():
    n, k, c, label = 9, 24, 5, 3
    h, wc, bc = synth.normal(1, (n, k)).astype(F64), synth.normal(2, (c, k)).astype(F64), synth.normal(3, (c,)).astype(F64)
    wb, bb = synth.normal(4, (4 * c, k)).astype(F64), synth.normal(5, (4 * c,), std=0.5).astype(F64)
    wb[4 * label + 2] *= 8          # the width deltas of the label spread to both sides of the clip
    prop, _ = K.random_boxes(6, n)
    lin_c, lin_b = nn.Linear(k, c).double(), nn.Linear(k, 4 * c).double()
    with torch.no_grad():
        lin_c.weight.copy_(T(wc)), lin_c.bias.copy_(T(bc)), lin_b.weight.copy_(T(wb)), lin_b.bias.copy_(T(bb))
        logits, reg = lin_c(T(h)), lin_b(T(h))
        scores = F.softmax(logits, -1)[:, label]
        # decode_single as torchvision 0.6.0 writes it, all classes at once, then the label's column
        boxes, wx, wy, ww, wh = T(prop).double(), *R.WEIGHTS
        widths, heights = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
        ctr_x, ctr_y = boxes[:, 0] + 0.5 * widths, boxes[:, 1] + 0.5 * heights
        dx, dy, dw, dh = reg[:, 0::4] / wx, reg[:, 1::4] / wy, reg[:, 2::4] / ww, reg[:, 3::4] / wh
        clip = float(F32(R.CLIP))
        dw, dh = torch.clamp(dw, max=clip), torch.clamp(dh, max=clip)
        pcx, pcy = dx * widths[:, None] + ctr_x[:, None], dy * heights[:, None] + ctr_y[:, None]
        pw, ph = torch.exp(dw) * widths[:, None], torch.exp(dh) * heights[:, None]
        half = torch.tensor(0.5, dtype=torch.float64)
        pred = torch.stack((pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph), dim=2)[:, label]
    rh, rw = 1080.0 / 749.0, 1920.0 / 1333.0
    ref = R.box_predict(h, wc, bc, wb, bb, prop, label, ratio_h=rh, ratio_w=rw)
    assert (reg[:, 4 * label + 2] / ww).max() > clip > (reg[:, 4 * label + 2] / ww).min(), "no delta above the clip in this case"
    np.testing.assert_allclose(ref["logits"], logits.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref["deltas"], reg[:, 4 * label:4 * label + 4].numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref["scores"], scores.numpy(), rtol=1e-13)
    ratio = np.array([F32(rw), F32(rh), F32(rw), F32(rh)], F64)
    np.testing.assert_allclose(ref["boxes"], pred.numpy() * ratio, rtol=1e-12, atol=1e-10)
    # the module's own torch decode is the same expression
    np.testing.assert_allclose(RH.decode_boxes(reg[:, 4 * label:4 * label + 4], T(prop).double(), clip=clip).numpy(), pred.numpy(), rtol=1e-13)
    assert float(F32(RH.BBOX_XFORM_CLIP)) == clip and RH.BBOX_REG_WEIGHTS == R.WEIGHTS


def test_mask_reference_against_float64_torch():
    x = synth.normal(11, (3, 6, 5, 5)).astype(F64)
    conv, up, last = nn.Conv2d(6, 4, 3, padding=1).double(), nn.ConvTranspose2d(4, 5, 2, 2).double(), nn.Conv2d(5, 3, 1).double()
    with torch.no_grad():
        a = F.relu(conv(T(x)))
        b = F.relu(up(a))
        c = last(b)
        p = torch.sigmoid(c[:, 1])
        p2 = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False)(p[:, None])[:, 0]
    g = lambda t: t.detach().numpy()
    ra = R.conv3x3(x, g(conv.weight), g(conv.bias))
    rb = R.conv_transpose2x2(ra, g(up.weight), g(up.bias))
    rc = R.conv1x1(rb, g(last.weight), g(last.bias))
    for got, want in ((ra, a), (rb, b), (rc, c), (R.roi_mask_finish(rc, 1, 1), p), (R.roi_mask_finish(rc, 1, 2), p2)):
        np.testing.assert_allclose(got, g(want), rtol=1e-12, atol=1e-13)
    # sizes 1 and 2: every source index is clamped
    for s in (1, 2, 28):
        z = synth.normal(12, (2, 2, s, s)).astype(F64)
        want = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False)(torch.sigmoid(T(z)[:, 1])[:, None])[:, 0]
        np.testing.assert_allclose(R.roi_mask_finish(z, 1, 2), want.numpy(), rtol=1e-13, atol=1e-15)
    i0, i1, l0, l1 = R.up2_axis(28, F32)
    assert (i0[0], i1[0], l1[0]) == (0, 1, 0.0) and (i0[-1], i1[-1]) == (27, 27) and l1[1] == 0.25 and l1[2] == 0.75


# ------------------------------------------------------------------------------------------------ modules and checkpoints
def test_state_dict_keys_are_torchvisions():
    heads = RH.RoIHeads()
    assert list(heads.state_dict()) == TORCHVISION_KEYS
    assert list(RH.RoIHeads(mask=False).state_dict()) == TORCHVISION_KEYS[:8]
    sd = heads.state_dict()
    assert tuple(sd["box_head.fc6.weight"].shape) == (1024, 12544) and tuple(sd["box_predictor.bbox_pred.weight"].shape) == (8, 1024)
    assert tuple(sd["mask_predictor.conv5_mask.weight"].shape) == (256, 256, 2, 2)
    assert tuple(sd["mask_predictor.mask_fcn_logits.weight"].shape) == (2, 256, 1, 1)
    small = RH.RoIHeads(num_classes=3, **K.SMALL)
    assert tuple(small.state_dict()["box_head.fc6.weight"].shape) == (64, 32 * 49)
    with pytest.raises(ValueError):
        RH.RoIHeads(num_classes=92)


def test_load_maskrcnn_state_dict_round_trip():
    src = RH.RoIHeads(**K.SMALL)
    W = synth.make_roi_head_weights(src, 5)
    whole = {"roi_heads." + k: torch.from_numpy(v) for k, v in W.items()}
    whole.update({"backbone.body.conv1.weight": torch.zeros(2), "rpn.head.conv.weight": torch.zeros(3), "transform.x": torch.zeros(1)})
    dst = RH.RoIHeads(**K.SMALL)
    assert RH.load_maskrcnn_state_dict(dst, whole) == sorted(W)
    for k, v in dst.state_dict().items():
        assert np.array_equal(v.numpy(), W[k]), k
    # a Faster R-CNN checkpoint: no mask keys
    faster = {k: v for k, v in whole.items() if ".mask_" not in k}
    box_only = RH.RoIHeads(mask=False, **K.SMALL)
    assert RH.load_maskrcnn_state_dict(box_only, faster) == sorted(k for k in W if k.startswith("box_"))
    assert not box_only.has_mask
    for bad in (faster, {**whole, "roi_heads.extra.weight": torch.zeros(1)},
                {**whole, "roi_heads.box_head.fc7.bias": torch.zeros(3)}):
        with pytest.raises(capi.MpnhipError):
            RH.load_maskrcnn_state_dict(RH.RoIHeads(**K.SMALL), bad)
    with pytest.raises(capi.MpnhipError):
        RH.load_maskrcnn_state_dict(box_only, whole)        # mask tensors the heads do not have


# ------------------------------------------------------------------------------------------------ host refusals
@pytest.fixture(scope="module")
def dummy():
    buf = ctypes.create_string_buffer(512)
    return buf, (ctypes.addressof(buf) + 255) & ~255


def test_box_predict_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy
    capi.path_counters(reset=True)
    w = (ctypes.c_float * 4)(10, 10, 5, 5)

    def call(h=p, ldh=64, wc=p, bc=p, wb=p, bb=p, prop=p, n=3, k=64, c=2, label=1, weights=w, boxes=p, scores=p):
        return l.mpnhip_box_predict(h, ldh, wc, bc, wb, bb, prop, n, k, c, label, weights, 4.135, 1.0, 1.0, boxes, scores, None, None, None)

    zero_w, inf_w = (ctypes.c_float * 4)(10, 0, 5, 5), (ctypes.c_float * 4)(10, 10, float("inf"), 5)
    for bad, msg in ((dict(n=-1), b"negative n"), (dict(h=None), b"null h"), (dict(wc=None), b"null h"), (dict(bb=None), b"null h"),
                     (dict(prop=None), b"null h"), (dict(boxes=None), b"null boxes or scores"), (dict(scores=None), b"null boxes or scores"),
                     (dict(weights=None), b"null weights"), (dict(c=1), b"classes"), (dict(c=92), b"classes"), (dict(k=0), b"multiple of 4"),
                     (dict(k=62, ldh=64), b"multiple of 4"), (dict(label=2), b"label"), (dict(label=-1), b"label"), (dict(ldh=60), b"ldh"),
                     (dict(ldh=66), b"ldh"), (dict(h=p + 4), b"aligned"), (dict(wb=p + 8), b"aligned"), (dict(weights=zero_w), b"finite"),
                     (dict(weights=inf_w), b"finite"), (dict(n=2 ** 31), b"more than one launch")):
        assert call(**bad) == -1, bad
        err = l.mpnhip_last_error()
        assert err.startswith(b"mpnhip_box_predict") and msg in err, (bad, err)
    assert call(n=0) == 0 and call(n=0, h=None, boxes=None, c=0, k=3) == 0
    assert all(v == 0 for v in capi.path_counters().values())


def test_nms_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy
    capi.path_counters(reset=True)
    big = 1 << 40

    def call(boxes=p, scores=p, ptr=p, n=10, nf=2, most=64, st=-math.inf, it=0.5, keep=p, order=p, count=p, ws=p, nbytes=big):
        return l.mpnhip_nms_batched(boxes, scores, ptr, n, nf, most, st, it, keep, order, count, ws, nbytes, None)

    for bad, msg in ((dict(n=-1), b"negative"), (dict(nf=-1), b"negative"), (dict(most=4097), b"max_per_frame 4097"), (dict(most=0), b"max_per_frame"),
                     (dict(n=2 ** 30 + 1), b"row ids"), (dict(nf=0), b"without frames"), (dict(boxes=None), b"null boxes"),
                     (dict(ptr=None), b"null boxes"), (dict(keep=None), b"null keep"), (dict(count=None), b"null keep"), (dict(boxes=p + 4), b"aligned"),
                     (dict(it=float("nan")), b"NaN"), (dict(st=float("nan")), b"NaN"), (dict(most=4096, nf=2 ** 20), b"more than one launch")):
        assert call(**bad) == -1, bad
        err = l.mpnhip_last_error()
        assert err.startswith(b"mpnhip_nms_batched") and msg in err, (bad, err)
    need = l.mpnhip_nms_batched_workspace_bytes(10, 64)
    assert need >= 2 * 10 * 8 + 2 * 10 * 4 + 10 * 8
    assert call(ws=None) == -3 and call(nbytes=need - 1) == -3
    assert b"mpnhip_nms_batched: workspace" in l.mpnhip_last_error()
    assert l.mpnhip_nms_batched_workspace_bytes(10, 4097) == 0 and l.mpnhip_nms_batched_workspace_bytes(0, 64) == 0
    assert l.mpnhip_nms_batched_workspace_bytes(-1, 64) == 0
    # the suppression words are n x ceil(max_per_frame / 64) x 8 bytes
    assert l.mpnhip_nms_batched_workspace_bytes(4096, 4096) - l.mpnhip_nms_batched_workspace_bytes(4096, 64) == 4096 * 63 * 8
    assert call(n=0) == 0 and call(n=0, boxes=None, most=9999, count=None, ws=None) == 0
    assert all(v == 0 for v in capi.path_counters().values())
    assert RH.NMS_MAX_PER_FRAME == 4096
    # the wrapper refuses a descending box_frame and a frame above the cap before it touches a device
    with pytest.raises(ValueError):
        RH.frame_ptr([0, 1, 0])
    with pytest.raises(ValueError):
        RH.frame_ptr([-1, 0])
    ptr, most = RH.frame_ptr([0, 0, 2, 2, 2, 5])
    assert list(ptr) == [0, 2, 2, 5, 5, 5, 6] and most == 3


def test_roi_mask_finish_refusals_without_gpu(dummy):
    l = capi.load()
    _, p = dummy
    capi.path_counters(reset=True)

    def call(logits=p, ld=2 * 28 * 28, n=3, c=2, label=1, size=28, up=2, out=p):
        return l.mpnhip_roi_mask_finish(logits, ld, n, c, label, size, up, out, None)

    for bad, msg in ((dict(n=-1), b"negative n"), (dict(logits=None), b"null"), (dict(out=None), b"null"), (dict(size=0), b"size"),
                     (dict(size=1025), b"size"), (dict(up=0), b"up"), (dict(up=3), b"up"), (dict(c=0), b"channels"), (dict(label=2), b"label"),
                     (dict(label=-1), b"label"), (dict(ld=2 * 28 * 28 - 1), b"ld"), (dict(c=3000, size=1024, ld=1 << 40), b"channels"),
                     (dict(n=1 << 40), b"more than one launch")):
        assert call(**bad) == -1, bad
        err = l.mpnhip_last_error()
        assert err.startswith(b"mpnhip_roi_mask_finish") and msg in err, (bad, err)
    assert call(n=0) == 0 and call(n=0, logits=None, out=None, size=0, up=7) == 0
    assert all(v == 0 for v in capi.path_counters().values())


def test_counter_names_and_places():
    names = list(capi.path_counters())
    assert names.index("conv_affine_up") < names.index("box_predict") < names.index("nms_batched") < names.index("roi_mask_finish") \
        < names.index("conv_transpose_bwd")


# ------------------------------------------------------------------------------------------------ NMS references
def test_nms_references_agree_on_every_gpu_case():
    """float32 and float64 give the same keep set and order on every input ``test_gpu_nms.py`` uses: no case is left out for
    closeness to the threshold"""
    for name, boxes, scores, ptr, iou_thr, score_thr in K.nms_cases():
        st = -math.inf if score_thr is None else score_thr
        if name == "frame_of_4096":
            a, b = R.nms_frame_fast(boxes, scores, iou_thr, st, F32), R.nms_frame_fast(boxes, scores, iou_thr, st, F64)
            assert a == b and 500 < len(a) < 4096, (name, len(a))
            continue
        margin = []
        r32, r64 = R.nms_batched(boxes, scores, ptr, iou_thr, st, F32), R.nms_batched(boxes, scores, ptr, iou_thr, st, F64, margin)
        for x, y in zip(r32, r64):
            assert np.array_equal(x, y), name
        print(name, "kept", int(r32[2].sum()), "of", len(scores), "smallest |iou - threshold| %.3g" % min(margin))
    (b, s, p), (bb, ss, pp, f) = K.embedded_frame()
    alone, inside = R.nms_batched(b, s, p, 0.5), R.nms_batched(bb, ss, pp, 0.5)
    assert np.array_equal(alone[0], inside[0][pp[f]:pp[f + 1]]) and alone[2][0] == inside[2][f]


def test_nms_reference_semantics_and_fast_form():
    for name, boxes, scores, want in K.edge_frames():
        for dt in (F32, F64):
            assert R.nms_frame(boxes, scores, 0.5, 0.25, dt) == want, (name, dt)
    b, s = K.random_boxes(31, 300)
    for thr, st in ((0.5, -math.inf), (0.3, 0.4)):
        assert R.nms_frame_fast(b, s, thr, st, F32) == R.nms_frame(b, s, thr, st, F32)
    # the same rule in torch: the IoU matrix, then the greedy loop
    tb = T(b).double()
    area = (tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])
    lt, rb = torch.max(tb[:, None, :2], tb[None, :, :2]), torch.min(tb[:, None, 2:], tb[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    iou = (inter / (area[:, None] + area[None, :] - inter)).numpy()
    kept = []
    for i in np.argsort(-s.astype(F64), kind="stable"):
        if all(iou[j, i] <= 0.5 for j in kept):
            kept.append(int(i))
    assert kept == R.nms_frame(b, s, 0.5, -math.inf, F64)


# ------------------------------------------------------------------------------------------------ the stock route
@pytest.fixture(scope="module")
def small():
    heads = RH.RoIHeads(**K.SMALL).eval()
    W = synth.make_roi_head_weights(heads, 21)
    feats = K.pyramid(22, K.SMALL["channels"])
    boxes, frame = K.boxes_on_frames(23, 9)
    return heads, W, feats, boxes, frame


def _cpu_pooler(monkeypatch):
    """the pooler is the one operator without a torch form: on the CPU its numpy restatement stands in"""
    def pool(features, boxes, frame_idx, image_size, output_size):
        out, _ = ER.fpn_roi_align([f.numpy() for f in features], boxes.numpy(), frame_idx.numpy(), image_size, None, output_size, 2)
        return torch.from_numpy(out)
    monkeypatch.setattr(RH, "fpn_roi_align", pool)


def test_stock_route_equals_the_reference(small, monkeypatch):
    heads, W, feats, boxes, frame = small
    _cpu_pooler(monkeypatch)
    tf = [T(f) for f in feats]
    net = ER.resize_boxes(boxes, K.ORIGINAL_SIZE, K.IMAGE_SIZE)
    rh, rw = RH.back_ratios(K.IMAGE_SIZE, K.ORIGINAL_SIZE)
    p7, _ = ER.fpn_roi_align(feats, net, frame, K.IMAGE_SIZE, None, 7, 2, acc=F64)
    p14, _ = ER.fpn_roi_align(feats, net, frame, K.IMAGE_SIZE, None, 14, 2, acc=F64)
    ref = R.box_branch(p7, W, net, 1, rh, rw)
    got_b, got_s = RH.predict_boxes(heads, tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE)
    assert got_b.dtype == torch.float32 and tuple(got_b.shape) == (9, 4) and tuple(got_s.shape) == (9,)
    np.testing.assert_allclose(got_s.numpy(), ref["scores"], rtol=0, atol=2e-6)
    assert (np.abs(got_b.numpy() - ref["boxes"]) <= 2e-5 * R.box_extent(ref["boxes"])).all()
    for up in (1, 2):
        m = RH.predict_masks(heads, tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE, upsample=up)
        assert tuple(m.shape) == (9, 1, 28 * up, 28 * up)
        np.testing.assert_allclose(m.numpy(), R.mask_branch(p14, W, 1, up), rtol=0, atol=5e-6)
    # predict: the masks on the refined boxes, in the network's image
    refined = R.box_branch(p7, W, net, 1)
    q14, _ = ER.fpn_roi_align(feats, refined["boxes"].astype(F32), frame, K.IMAGE_SIZE, None, 14, 2, acc=F64)
    pb, ps, pm = RH.predict(heads, tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE)
    assert (np.abs(pb.numpy() - ref["boxes"]) <= 2e-5 * R.box_extent(ref["boxes"])).all()
    np.testing.assert_allclose(ps.numpy(), ref["scores"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(pm.numpy(), R.mask_branch(q14, W, 1, 1), rtol=0, atol=2e-4)
    # the routes are named, the native one is inference only, heads without a mask branch say so
    with pytest.raises(ValueError):
        RH.predict_boxes(heads, tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE, convs='fast')
    heads.train()
    with pytest.raises(capi.MpnhipError):
        RH.predict_boxes(heads, tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE, convs='native')
    heads.eval()
    with pytest.raises(capi.MpnhipError):
        RH.predict_masks(RH.RoIHeads(mask=False, **K.SMALL).eval(), tf, boxes, frame, K.IMAGE_SIZE, K.ORIGINAL_SIZE)
    with pytest.raises(ValueError):
        RH.predict_boxes(heads, tf, np.array([[5, 5, 3, 9]], F32), [0], K.IMAGE_SIZE, K.ORIGINAL_SIZE)


def test_det_table_and_file(tmp_path):
    boxes = np.array([[10.5, 20.25, 30.5, 60.25], [11, 20, 31, 60], [100, 100, 120, 140], [5, 5, 9, 9]], F32)
    scores = np.array([0.9, 0.8, 0.3, 0.95], F32)
    table, kept = R.det_table(boxes, scores, np.array([0, 0, 0, 1]), [7, 9], 0.5, 0.5)
    assert kept == [0, 3]
    assert np.array_equal(table, np.array([[7, -1, 11.5, 21.25, 20, 40, F32(0.9)], [9, -1, 6, 6, 4, 4, F32(0.95)]], F64))
    path = tmp_path / "det.txt"
    RH.write_det_file(str(path), table)
    assert path.read_text() == "7,-1,11.5,21.25,20.0,40.0,0.9\n9,-1,6.0,6.0,4.0,4.0,0.95\n"
