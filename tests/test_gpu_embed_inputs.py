"""The embedding inputs on the device (``csrc/embed_inputs.hip`` through ``mpntrackseg_amd.embed_inputs``): ReID patches equal what
numpy's ``pad`` and Pillow's ``resize`` returned (tests/golden/g23_reid_crops.npz) byte for byte and the restatement's float32
bit for bit; the FPN RoIAlign equals the float32 restatement of tests/embed_inputs_ref.py bit for bit; the stored node_ext files
come back through ``embeddings.load_precomputed_embeddings``."""
import numpy as np
import pytest
import torch

import embed_inputs_ref as R
from mpntrackseg_amd import embed_inputs as E, embeddings as EM

pytestmark = pytest.mark.gpu

GROUPS = (("small_128x64", "small_frames", (128, 64)), ("small_16x8", "small_frames", (16, 8)), ("small_5x3", "small_frames", (5, 3)),
          ("big_128x64", "big_frames", (128, 64)))


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("g23_reid_crops.npz")


@pytest.fixture(scope="module")
def frames(fixture):
    return {k: torch.from_numpy(fixture[k]).to(dev()) for k in ("small_frames", "big_frames")}


# ------------------------------------------------------------------------------------------------ patches
@pytest.mark.parametrize("group,which,size", GROUPS)
def test_crops_equal_pad_and_pillow_byte_for_byte(fixture, frames, group, which, size):
    boxes, box_frame, want = fixture[group + "_boxes"], fixture[group + "_frame"], fixture[group + "_crops"]
    out, u8 = E.reid_crops(frames[which], boxes, box_frame, size, return_uint8=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(boxes), 3) + size and out.is_cuda
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == want.shape
    u8 = u8.cpu().numpy()
    names = fixture["big_names" if which == "big_frames" else "small_names"]
    for k in range(len(boxes)):
        assert np.array_equal(u8[k], want[k]), "box %d of %s (%s): %d bytes differ" % (k, group, names[k] if len(names) == len(boxes) else "", int((u8[k] != want[k]).sum()))
    assert np.array_equal(out.cpu().numpy(), R.normalise(want))          # the normalised floats, bit for bit
    assert torch.equal(E.reid_crops(frames[which], boxes, box_frame, size), out)


def test_crop_rows_do_not_depend_on_their_neighbours_or_the_launch_grouping(fixture, frames):
    boxes, box_frame = fixture["small_16x8_boxes"], fixture["small_16x8_frame"]
    whole, whole_u8 = E.reid_crops(frames["small_frames"], boxes, box_frame, (16, 8), return_uint8=True)
    perm = np.random.default_rng(2).permutation(len(boxes))
    assert len(set(box_frame[perm][:4].tolist())) == 2                    # both frames, out of order
    shuffled = E.reid_crops(frames["small_frames"], boxes[perm], box_frame[perm], (16, 8))
    assert torch.equal(shuffled, whole[torch.from_numpy(perm).to(dev())])
    for k in (0, 7, 12, 17):
        assert torch.equal(E.reid_crops(frames["small_frames"], boxes[k:k + 1], box_frame[k:k + 1], (16, 8))[0], whole[k]), k
    grouped, grouped_u8 = E.reid_crops(frames["small_frames"], boxes, box_frame, (16, 8), return_uint8=True, boxes_per_launch=5)
    assert torch.equal(grouped, whole) and torch.equal(grouped_u8, whole_u8)


def test_crops_without_pad_and_with_other_statistics_equal_the_restatement(fixture, frames):
    boxes, box_frame = fixture["small_16x8_boxes"], fixture["small_16x8_frame"]
    mean, std = (0.4, 0.5, 0.6), (0.2, 0.25, 0.3)
    want_u8, want = R.reid_crops(fixture["small_frames"], boxes, box_frame, (16, 8), pad=False, mean=mean, std=std)
    out, u8 = E.reid_crops(frames["small_frames"], boxes, box_frame, (16, 8), pad=False, mean=mean, std=std, return_uint8=True)
    assert np.array_equal(u8.cpu().numpy(), want_u8) and np.array_equal(out.cpu().numpy(), want)
    table = {k: v for k, v in zip(("bb_left", "bb_top", "bb_right", "bb_bot"), boxes.T)}         # the DataFrame's columns
    assert torch.equal(E.reid_crops(frames["small_frames"], table, box_frame, (16, 8), pad=False, mean=mean, std=std), out)


def test_no_boxes_give_an_empty_batch(frames):
    out = E.reid_crops(frames["small_frames"], np.zeros((0, 4)), np.zeros(0, np.int64))
    assert tuple(out.shape) == (0, 3, 128, 64) and out.is_cuda


# ------------------------------------------------------------------------------------------------ RoIAlign
IMAGE, ORIGINAL = (500, 640), (375, 480)
SHAPES = ((128, 160), (64, 80), (32, 40), (16, 20))       # the levels of the image padded to a multiple of 32: 512 x 640
# (name, box in the frame's own coordinates: left, top, right, bottom; the level it must get)
BOXES = (
    ("level 0", (100.0, 50.0, 145.5, 92.25), 0), ("level 0, again", (300.0, 200.0, 330.0, 270.0), 0),
    ("level 1", (50.5, 60.0, 170.0, 190.0), 1), ("level 1, again", (200.0, 100.0, 330.25, 215.5), 1),
    ("level 2", (20.0, 30.0, 250.0, 280.0), 2), ("level 2, again", (150.0, 20.0, 420.0, 300.5), 2),
    ("level 3", (10.0, 5.0, 370.0, 365.0), 3), ("level 3, again", (60.0, 3.0, 459.0, 372.0), 3),
    ("canonical 112", (30.0, 12.0, 114.0, 96.0), 1), ("canonical 224", (30.0, 12.0, 198.0, 180.0), 2), ("canonical 448", (30.0, 12.0, 366.0, 348.0), 3),
    ("under one cell wide", (200.0, 20.0, 202.0, 320.0), 0),
    ("past the right and bottom edges", (400.0, 300.0, 520.0, 420.0), 1),
    ("from negative coordinates", (-40.0, -30.0, 60.0, 50.0), 1),
)
BOX_FRAME = np.asarray([1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0])


def features(channels, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(2, channels) + s).astype(np.float32) for s in SHAPES]


@pytest.fixture(scope="module")
def pyramid():
    host = features(5, 11)
    return host, [torch.from_numpy(f).to(dev()) for f in host]


def boxes_array():
    return np.asarray([b[1] for b in BOXES], np.float64)


def test_the_boxes_are_the_cases_they_are_named_for():
    b = R.resize_boxes(boxes_array(), ORIGINAL, IMAGE)
    scales = R.level_scales(SHAPES, IMAGE)
    assert scales == [1 / 4, 1 / 8, 1 / 16, 1 / 32]                       # (128 / 500 and 16 / 500 round to them)
    assert R.box_levels(b).tolist() == [c[2] for c in BOXES]
    side = np.sqrt((b[:, 2] - b[:, 0]).astype(np.float64) * (b[:, 3] - b[:, 1]))
    assert side[8:11].tolist() == [112.0, 224.0, 448.0]
    assert (np.abs(np.log2(np.delete(side, (8, 9, 10)) / 224) % 1 - 0.5) < 0.49).all()     # the others: 0.01 octaves or more from a boundary
    k = 11
    assert (b[k, 2] - b[k, 0]) * scales[0] < 1                            # the extent clamps to 1
    k = 12
    for axis, size in ((0, SHAPES[1][1]), (1, SHAPES[1][0])):
        low, high, l, h, inside = R.roi_axis(b[k, axis], b[k, 2 + axis], scales[1], 14, 2, size, np.float32)
        assert (~inside).any() and (inside & (low == high) & (low == size - 1)).any(), axis    # beyond size; between size - 1 and size
    k = 13
    for axis, size in ((0, SHAPES[1][1]), (1, SHAPES[1][0])):
        low, high, l, h, inside = R.roi_axis(b[k, axis], b[k, 2 + axis], scales[1], 14, 2, size, np.float32)
        assert (~inside[0]).any() and (inside & (low == 0) & (l == 0)).any(), axis             # below -1; between -1 and 0
    assert len(set(BOX_FRAME.tolist())) == 2 and (np.diff(BOX_FRAME) < 0).any()


@pytest.mark.parametrize("S", (14, 7, 3))
def test_fpn_roi_align_has_the_bits_of_the_float32_restatement(pyramid, S):
    host, device = pyramid
    want, levels = R.fpn_roi_align(host, boxes_array(), BOX_FRAME, IMAGE, ORIGINAL, S, 2)
    got = E.fpn_roi_align(device, boxes_array(), BOX_FRAME, IMAGE, ORIGINAL, S, 2)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(BOXES), 5, S, S) and got.is_cuda
    got = got.cpu().numpy()
    for k, (name, _, _) in enumerate(BOXES):
        assert np.array_equal(got[k], want[k]), "%s: max |device - restatement| = %.3e" % (name, np.abs(got[k] - want[k]).max())
    assert np.abs(want).max() > 0.1 and (want[12] == 0).any() and (want[13] == 0).any()
    assert torch.equal(E.fpn_roi_align(device, boxes_array(), BOX_FRAME, IMAGE, ORIGINAL, S, 2).cpu(), torch.from_numpy(got))


def test_fpn_roi_align_without_the_box_mapping_and_with_three_samples(pyramid):
    host, device = pyramid
    b = R.resize_boxes(boxes_array(), ORIGINAL, IMAGE)
    want, _ = R.fpn_roi_align(host, b, BOX_FRAME, IMAGE, None, 5, 3)
    got = E.fpn_roi_align(device, b, BOX_FRAME, IMAGE, None, 5, 3)
    assert np.array_equal(got.cpu().numpy(), want)


def test_the_other_paths_of_the_kernel(pyramid):
    """S = 17: more positions than the 256 threads of a block, so a thread takes a second one.  And boxes pooled from a level
    where their footprint is far larger than the level mapper would allow, which only the C entry point permits (the levels are
    the caller's there): of the two below, both at level 0 (128 x 160 cells), the first touches 120 x 153 cells, the second
    79 x 99."""
    import ctypes
    from mpntrackseg_amd import capi
    host, device = pyramid
    want, _ = R.fpn_roi_align(host, boxes_array(), BOX_FRAME, IMAGE, ORIGINAL, 17, 2)
    assert np.array_equal(E.fpn_roi_align(device, boxes_array(), BOX_FRAME, IMAGE, ORIGINAL, 17, 2).cpu().numpy(), want)
    boxes = np.asarray([[2.5, 3.25, 630.0, 490.0], [100.0, 80.0, 500.0, 400.0]], np.float32)
    frame, ids = [1, 0], [5, 6]
    for k, cells in ((0, (120, 153)), (1, (79, 99))):
        spans = [R.roi_axis(boxes[k, a], boxes[k, 2 + a], 0.25, 14, 2, SHAPES[0][1 - a], np.float32) for a in (1, 0)]
        assert tuple(int(hi.max() - lo.min() + 1) for lo, hi, _, _, _ in spans) == cells
    lv = capi.FpnLevels()
    for l, f in enumerate(device):
        lv.data[l], lv.h[l], lv.w[l], lv.scale[l] = f.data_ptr(), f.shape[2], f.shape[3], 0.25 / 2 ** l
    to = lambda a, t: torch.tensor(a, dtype=t, device=dev())
    b, fr, lvl, idd = to(boxes, torch.float32), to(frame, torch.int32), to([0, 0], torch.int32), to(ids, torch.int32)
    out = torch.empty((2, 6, 14, 14), dtype=torch.float32, device=dev())
    capi.check(capi.load().mpnhip_fpn_roi_align(ctypes.byref(lv), 2, 5, capi.ptr(b), capi.ptr(fr), capi.ptr(lvl), 2, 14, 2, capi.ptr(idd),
                                                capi.ptr(out), capi.stream_ptr()), "mpnhip_fpn_roi_align")
    out = out.cpu().numpy()
    for k in range(2):
        assert np.array_equal(out[k, 1:], R.roi_align(host[0][frame[k]], boxes[k], 0.25, 14, 2, np.float32)), k
        assert (out[k, 0] == ids[k]).all()


def test_256_channels_and_the_detection_id_channel(pyramid):
    host = features(256, 12)
    device = [torch.from_numpy(f).to(dev()) for f in host]
    pick = [2, 7, 12]
    boxes, box_frame, ids = boxes_array()[pick], BOX_FRAME[pick], np.asarray([70001, 3, (1 << 24) - 1])
    want, _ = R.fpn_roi_align(host, boxes, box_frame, IMAGE, ORIGINAL, 14, 2)
    plain = E.fpn_roi_align(device, boxes, box_frame, IMAGE, ORIGINAL)
    assert tuple(plain.shape) == (3, 256, 14, 14) and np.array_equal(plain.cpu().numpy(), want)
    with_id = E.fpn_roi_align(device, boxes, box_frame, IMAGE, ORIGINAL, detection_id=ids)
    assert tuple(with_id.shape) == (3, 257, 14, 14)
    assert torch.equal(with_id[:, 1:], plain)
    assert torch.equal(with_id[:, 0].cpu(), torch.from_numpy(ids.astype(np.float32)).view(3, 1, 1).expand(3, 14, 14))
    # five channels with ids: the id channel shifts every block's range of outputs
    host5, device5 = pyramid
    ids = np.arange(len(BOXES)) * 1000 + 7
    for S in (14, 3):
        with_id = E.fpn_roi_align(device5, boxes_array(), BOX_FRAME, IMAGE, ORIGINAL, S, 2, detection_id=ids)
        want5, _ = R.fpn_roi_align(host5, boxes_array(), BOX_FRAME, IMAGE, ORIGINAL, S, 2, detection_id=ids)
        assert np.array_equal(with_id.cpu().numpy(), want5)


def test_stored_node_ext_embeddings_come_back_through_load_precomputed_embeddings(pyramid, tmp_path):
    host, device = pyramid
    b = boxes_array()
    frame = np.where(BOX_FRAME == 0, 3, 8)                               # the features of frames 3 and 8, in that order
    order = np.argsort(frame, kind="stable")                             # the det table: sorted by frame, ids ascending
    det = {"frame": frame[order], "detection_id": np.arange(len(BOXES)) + 40, "bb_left": b[order, 0], "bb_top": b[order, 1],
           "bb_right": b[order, 2], "bb_bot": b[order, 3]}
    emb = E.node_ext_embeddings(device, det, IMAGE, ORIGINAL)
    want, _ = R.fpn_roi_align(host, b[order], BOX_FRAME[order], IMAGE, ORIGINAL, 14, 2, detection_id=det["detection_id"])
    assert tuple(emb.shape) == (len(BOXES), 6, 14, 14) and np.array_equal(emb.cpu().numpy(), want)
    rel = E.store_node_ext_embeddings(str(tmp_path), "dets_file", "node_ext", det["frame"], emb)
    stored = torch.load(str(tmp_path / "processed_data" / "embeddings" / "dets_file" / "node_ext" / "3.pt"))
    assert tuple(stored.shape) == (int((frame == 3).sum()), 6, 14, 14) and stored[:, 0, 0, 0].tolist() == det["detection_id"][det["frame"] == 3].tolist()
    keep = np.ones(len(BOXES), bool)
    keep[[1, 9]] = False                                                 # a det table that drops two detections
    kept = {k: v[keep] for k, v in det.items()}
    back = EM.load_precomputed_embeddings(kept, {"seq_path": str(tmp_path)}, rel, embedding_dim='3D')
    assert back.is_cuda and torch.equal(back, emb[torch.from_numpy(keep).to(dev())][:, 1:])


def test_no_boxes_give_an_empty_result(pyramid):
    _, device = pyramid
    out = E.fpn_roi_align(device, np.zeros((0, 4)), np.zeros(0, np.int64), IMAGE, ORIGINAL)
    assert tuple(out.shape) == (0, 5, 14, 14) and out.is_cuda
    out = E.fpn_roi_align(device, np.zeros((0, 4)), np.zeros(0, np.int64), IMAGE, ORIGINAL, detection_id=np.zeros(0, np.int64))
    assert tuple(out.shape) == (0, 6, 14, 14)
