"""Full-frame MOTS masks without a device: the run-length codec of ``mpntrackseg_amd.masks`` against COCO's (restated statement
by statement in tests/full_masks_ref.py) and the sample line of the MOTS evaluation kit, the float32 restatement of the paste
against the literal pipeline (torch's CPU resize) and the reference's own ``ensure_unique_masks``
(tests/golden/g20_full_masks.npz; tools/make_golden.py gen_g20), the argument checks of the new C-ABI entry points, and
``tracker.save_results_to_file``."""
import ctypes

import numpy as np
import pytest

from mpntrackseg_amd import capi, masks as M, tracker
import full_masks_ref as R

MPNHIP_ERR_WORKSPACE = -3   # include/mpnhip.h


# ------------------------------------------------------------------------------------------------ codec
def test_sample_line_of_the_evaluation_kit_round_trips(golden):
    z = golden("g20_full_masks.npz")
    s, (h, w) = str(z["sample_rle"]), z["sample_shape"].tolist()
    assert (h, w) == (375, 1242)
    counts = M.rle_counts(s)
    assert counts.tolist() == R.np_rle_from_string(s)
    assert counts.size == 83 and int(counts.sum()) == h * w and counts.min() >= 0
    assert M.rle_string(counts) == s and R.np_rle_string(counts.tolist()) == s
    mask = M.rle_to_mask(s, h, w)
    assert mask.shape == (h, w) and mask.dtype == np.uint8 and int(mask.sum()) == int(counts[1::2].sum())
    assert R.np_rle_counts(mask) == counts.tolist()


def _round_trip(mask):
    h, w = mask.shape
    counts = R.np_rle_counts(mask)
    assert sum(counts) == h * w and (len(counts) == 1 or counts[-1] > 0)   # no trailing zero-length run
    s = M.rle_string(counts)
    assert s == R.np_rle_string(counts)
    assert M.rle_counts(s).tolist() == counts
    assert np.array_equal(M.rle_to_mask(s, h, w), mask)
    # the boundaries the device hands over give the same counts
    pos, n = R.np_events(np.where(mask, 0, -1), 1)
    assert n.tolist() == [len(counts) - 1] and M.rle_counts_from_events(pos, h * w).tolist() == counts
    return s, counts


def test_random_masks_round_trip():
    rng = np.random.default_rng(1)
    for h, w, p in ((1, 1, 0.5), (7, 5, 0.5), (37, 53, 0.1), (37, 53, 0.9), (64, 48, 0.5), (375, 300, 0.02)):
        for _ in range(3):
            _round_trip((rng.random((h, w)) < p).astype(np.uint8))
    # long runs: counts that need several 5-bit groups, and negative differences
    m = np.zeros((300, 500), np.uint8)
    m[:, 100:350] = 1
    m[10:20, 400] = 1
    _, counts = _round_trip(m)
    assert max(counts) > 32 ** 3


def test_edge_masks_round_trip():
    h, w = 6, 4
    empty, full = np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)
    assert _round_trip(empty)[1] == [24]
    assert _round_trip(full)[1] == [0, 24]
    first = empty.copy()
    first[0, 0] = 1
    assert _round_trip(first)[1] == [0, 1, 23]
    last = empty.copy()
    last[-1, -1] = 1
    assert _round_trip(last)[1] == [23, 1]
    across = empty.copy()          # the run goes on from the foot of column 1 to the head of column 2
    across[4:, 1] = 1
    across[:3, 2] = 1
    assert _round_trip(across)[1] == [10, 5, 9]
    with pytest.raises(ValueError):
        M.rle_to_mask(M.rle_string([10, 5, 9]), h, w + 1)
    with pytest.raises(ValueError):
        M.rle_counts("o")              # a group that announces another one and is the last
    assert M.rle_string([]) == "" and M.rle_counts("").size == 0


# ------------------------------------------------------------------------------------------------ restatement
EXCLUDE = 1e-5   # five times the largest difference seen between the float32 restatement and torch's CPU interpolate (1.9e-6)


def _excluded(images, threshold):
    """Pixels the literal pipeline decides within EXCLUDE: the winner's value against the threshold, or the two largest values
    against each other.  A tie is counted only where it can show in a binary mask, i.e. where the winner comes within EXCLUDE of
    reaching the threshold: below that every mask is 0 at the pixel whoever wins (the zeros outside the boxes tie everywhere).
    That leaves out fewer pixels than the plain rule, never more."""
    top = np.sort(images, axis=0)
    near_thr = np.abs(top[-1] - np.float32(threshold)) <= EXCLUDE
    near_tie = (top[-1] - top[-2] <= EXCLUDE) if images.shape[0] > 1 else np.zeros_like(near_thr)
    return near_thr | (near_tie & (top[-1] >= np.float32(threshold) - EXCLUDE))


def _covered(boxes, mw, H, W):
    cov = np.zeros((H, W), bool)
    for x0, y0, x1, y1, _, _ in R.np_expand_boxes(boxes, mw).tolist():
        if x1 >= x0 and y1 >= y0:
            cov[max(y0, 0):max(min(y1 + 1, H), 0), max(x0, 0):max(min(x1 + 1, W), 0)] = True
    return cov


def test_restatement_against_the_literal_pipeline():
    """40 frames of 6 sigmoid blobs with +-0.05 noise, boxes of 3 - 90 px, partly off the image: the binary masks of the float32
    restatement equal those of the literal pipeline (torch's CPU resize, np.argmax, >= 0.5) except where the literal pipeline
    decides within 1e-5, and such pixels are at most 0.1 % of the pixels a box covers."""
    rng = np.random.default_rng(2020)
    H, W, thr = 96, 128, 0.5
    excluded = covered = differing = 0
    for case in range(40):
        masks = R.blob_masks(rng, 6)
        boxes = R.random_boxes(rng, 6, H, W)
        lit = R.literal_paste(masks, boxes, H, W)
        want, _ = R.np_frame(masks, boxes, H, W, thr, paste=lambda *a: lit)
        got, _ = R.np_frame(masks, boxes, H, W, thr)
        ex = _excluded(lit, thr)
        cov = _covered(boxes, 56, H, W)
        assert not ((lit != 0).any(axis=0) & ~cov).any()
        excluded += int((ex & cov).sum())
        covered += int(cov.sum())
        differing += int((got != want).sum())
        assert np.array_equal(got[~ex], want[~ex]), case
    print("literal pipeline: %d of %d box-covered pixels excluded, %d pixels differ" % (excluded, covered, differing))
    assert covered > 100000
    assert excluded <= 0.001 * covered


def test_restatement_against_the_reference_fixture(golden):
    z = golden("g20_full_masks.npz")
    (H, W), thr, fp = z["img_shape"].tolist(), float(z["mask_threshold"]), z["frame_ptr"]
    assert z["masks"].shape == (11, 56, 56) and fp.tolist() == [0, 6, 7, 11] and (H, W) == (96, 128)
    ref = np.unpackbits(z["binary_bits"])[:11 * H * W].reshape(11, H, W)
    strings = [str(s) for s in z["rle"]]
    excluded = covered = 0
    for f in range(3):
        a, b = int(fp[f]), int(fp[f + 1])
        masks, boxes = z["masks"][a:b], z["boxes"][a:b]
        labels, _ = R.np_frame(masks, boxes, H, W, thr)
        ex = _excluded(R.literal_paste(masks, boxes, H, W), thr)
        cov = _covered(boxes, 56, H, W)
        excluded += int((ex & cov).sum())
        covered += int(cov.sum())
        got = R.binary_masks(labels, b - a)
        assert np.array_equal(got[:, ~ex], ref[a:b][:, ~ex])
        assert ref[a:b].sum(axis=0).max() <= 1
        for i in range(a, b):   # the stored strings are the stored masks
            assert np.array_equal(M.rle_to_mask(strings[i], H, W), ref[i])
            assert M.rle_string(R.np_rle_counts(ref[i])) == strings[i]
        if not ex.any():
            assert R.np_strings(labels, b - a) == strings[a:b]
    assert excluded <= 0.001 * covered
    assert ref.sum() > 2000


def test_restatement_on_hand_made_frames():
    """The rules of the arg-max, stated on values: first maximum, NaN as the maximum, the threshold on the winner."""
    imgs = np.zeros((3, 1, 5), np.float32)
    imgs[0, 0] = [0.6, 0.2, np.nan, 0.5, 0.0]
    imgs[1, 0] = [0.6, 0.7, 0.9, 0.4, 0.0]
    imgs[2, 0] = [0.9, 0.7, np.nan, 0.1, 0.0]
    winner, value = R.np_unique(imgs)
    assert winner[0].tolist() == [2, 1, 0, 0, 0]
    labels = R.np_labels(winner, value, 0.5)
    assert labels[0].tolist() == [2, 1, -1, 0, -1]
    # truncation toward zero of the expanded box: -0.4 -> 0, and the scale comes from the mask WIDTH
    b = R.np_expand_boxes([[0.0, 0.0, 11.2, 11.2], [5.0, 5.0, 3.0, 3.0], [np.nan, 0, 1, 1]], 28)
    assert b[0].tolist() == [0, 0, 11, 11, 12, 12]
    assert b[1].tolist() == [5, 5, 2, 2, 1, 1]      # r < l: the corners cross, nothing is pasted, the resize would be 1 x 1
    assert b[2].tolist() == [0, 0, -1, -1, 1, 1]
    # a 2 x 2 mask of ones resized to its own padded size is the padded mask
    assert np.array_equal(R.np_resize(np.ones((2, 2), np.float32), 4, 4), np.pad(np.ones((2, 2), np.float32), 1))


# ------------------------------------------------------------------------------------------------ C ABI
def test_full_masks_entry_points_argument_checks_without_gpu():
    """Size queries and argument checks run on the host: empty inputs are successful no-ops, null pointers with work to do and
    bad sizes are refused before any launch with the function's name in mpnhip_last_error(), a short workspace is
    MPNHIP_ERR_WORKSPACE."""
    l = capi.load()
    one = ctypes.c_void_p(256)   # a non-null address that no call below may reach a launch with
    big = 1 << 30
    thr = ctypes.c_float(0.5)
    q = l.mpnhip_full_masks_workspace_bytes
    assert q(0, 0, 0, 0) == 0
    assert q(240, 8, 1080 * 1920, 0) >= 240 * 24
    assert q(240, 8, 1080 * 1920, 100000) >= q(240, 8, 1080 * 1920, 0) + 3 * 4 * 100000
    assert q(10, 1, 1 << 31, 0) == 0 and q(-1, 1, 100, 0) == 0
    paste = l.mpnhip_paste_unique_masks
    # nothing to do
    assert paste(None, 0, 56, 56, None, None, 0, None, 0, 1080, 1920, thr, None, None, None, 0, None) == 0
    assert paste(None, 0, 56, 56, None, None, 0, one, 3, 0, 1920, thr, None, None, None, 0, None) == 0
    # refusals
    assert paste(one, 5, 56, 56, one, None, 5, one, 2, 37, 53, ctypes.c_float(0.0), one, None, one, big, None) != 0
    assert b"paste_unique_masks" in l.mpnhip_last_error() and b"mask_threshold" in l.mpnhip_last_error()
    assert paste(one, 5, 56, 56, one, None, 5, one, 2, 37, 53, ctypes.c_float(-1.0), one, None, one, big, None) != 0
    assert paste(one, 5, 56, 56, one, None, 5, one, 2, 37, 53, ctypes.c_float(float("nan")), one, None, one, big, None) != 0
    assert paste(one, 5, 0, 56, one, None, 5, one, 2, 37, 53, thr, one, None, one, big, None) != 0
    assert b"mh, mw" in l.mpnhip_last_error()
    assert paste(one, 5, 56, 0, one, None, 5, one, 2, 37, 53, thr, one, None, one, big, None) != 0
    assert paste(one, 5, 56, 56, one, None, 5, one, 2, 1 << 16, 1 << 15, thr, one, None, one, big, None) != 0   # H * W = 2^31
    assert b"paste_unique_masks" in l.mpnhip_last_error()
    assert paste(one, 5, 56, 56, one, None, 5, one, 2, -37, 53, thr, one, None, one, big, None) != 0
    assert paste(one, 5, 56, 56, one, None, 5, one, 70000, 37, 53, thr, one, None, one, big, None) != 0
    assert paste(None, 5, 56, 56, one, None, 5, one, 2, 37, 53, thr, one, None, one, big, None) != 0
    assert paste(one, 5, 56, 56, None, None, 5, one, 2, 37, 53, thr, one, None, one, big, None) != 0
    assert paste(one, 5, 56, 56, one, None, 5, None, 2, 37, 53, thr, one, None, one, big, None) != 0
    assert paste(one, 5, 56, 56, one, None, 5, one, 2, 37, 53, thr, None, None, one, big, None) != 0
    assert b"paste_unique_masks" in l.mpnhip_last_error()
    assert paste(one, 5, 56, 56, one, None, 5, one, 2, 37, 53, thr, one, None, one, 16, None) == MPNHIP_ERR_WORKSPACE
    assert paste(one, 5, 56, 56, one, None, 5, one, 2, 37, 53, thr, one, None, None, 0, None) == MPNHIP_ERR_WORKSPACE
    assert b"paste_unique_masks" in l.mpnhip_last_error()
    count = l.mpnhip_mask_run_events_count
    assert count(None, 0, 0, 0, None, None, None, 0, None) == 0
    assert count(None, 2, 37 * 53, 5, one, one, one, big, None) != 0
    assert b"mask_run_events_count" in l.mpnhip_last_error()
    assert count(one, 2, 37 * 53, 5, None, one, one, big, None) != 0
    assert count(one, 2, 37 * 53, 5, one, None, one, big, None) != 0
    assert count(one, 2, 1 << 31, 5, one, one, one, big, None) != 0
    assert count(one, -2, 37 * 53, 5, one, one, one, big, None) != 0
    assert count(one, 2, 37 * 53, 5, one, one, one, 16, None) == MPNHIP_ERR_WORKSPACE
    assert count(one, 2, 37 * 53, 5, one, one, None, 0, None) == MPNHIP_ERR_WORKSPACE
    assert b"mask_run_events_count" in l.mpnhip_last_error()
    fill = l.mpnhip_mask_run_events
    assert fill(None, 0, 0, 0, 0, None, None, 0, None) == 0
    assert fill(None, 2, 37 * 53, 5, 0, None, None, 0, None) == 0          # no event: nothing to write
    assert fill(None, 2, 37 * 53, 5, 10, one, one, big, None) != 0
    assert b"mask_run_events" in l.mpnhip_last_error()
    assert fill(one, 2, 37 * 53, 5, 10, None, one, big, None) != 0
    assert fill(one, 2, 37 * 53, 5, -1, one, one, big, None) != 0
    assert fill(one, 2, 37 * 53, 5, 1 << 31, one, one, big, None) != 0
    assert fill(one, 2, 1 << 31, 5, 10, one, one, big, None) != 0
    assert fill(one, 2, 37 * 53, 5, 10, one, one, 16, None) == MPNHIP_ERR_WORKSPACE
    assert fill(one, 2, 37 * 53, 5, 10, one, None, 0, None) == MPNHIP_ERR_WORKSPACE
    assert b"mask_run_events" in l.mpnhip_last_error()


def test_python_entry_points_refuse_host_tensors_and_bad_thresholds():
    import torch
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        M.paste_unique_masks(torch.zeros(1, 1, 4, 4), np.zeros((1, 4)), [0, 1], (8, 8), 0.5)
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        M.mask_run_events(torch.zeros((1, 8, 8), dtype=torch.int32), 1)
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        tracker.to_full_masks(torch.zeros(1, 1, 4, 4), np.zeros((1, 4)), [0], [True], (8, 8))


# ------------------------------------------------------------------------------------------------ text output
def test_save_results_to_file(tmp_path):
    frame = np.array([3, 1, 1, 2, 3, 1])
    ped = np.array([7, 4, 0, 4, 2, 9])
    keep = np.array([True, True, True, True, True, False])
    rles = np.array(["a", "b", "c", "d", "e", None], dtype=object)
    path = tmp_path / "seq.txt"
    rows = tracker.save_results_to_file(str(path), frame, ped, 2, (375, 1242), rles, keep)
    text = path.read_text()
    assert text == "".join(r + "\n" for r in rows)
    # id = ped_id + label * 1000 + 1; rows by (frame, id); frame id label height width rle; the dropped detection is absent
    assert rows == ["1 2001 2 375 1242 c", "1 2005 2 375 1242 b", "2 2005 2 375 1242 d", "3 2003 2 375 1242 e", "3 2008 2 375 1242 a"]
    assert all(len(r.split(" ")) == 6 for r in rows) and "2010" not in text
    assert list(tmp_path.iterdir()) == [path]            # no date-stamped second copy
    # a label per detection, tensors as inputs
    import torch
    rows = tracker.save_results_to_file(str(path), torch.from_numpy(frame), torch.from_numpy(ped), np.array([2, 2, 1, 2, 2, 2]),
                                        (375, 1242), rles, torch.from_numpy(keep))
    assert rows[0] == "1 1001 1 375 1242 c" and rows[1] == "1 2005 2 375 1242 b" and len(rows) == 5
    with pytest.raises(capi.MpnhipError, match="no mask"):
        tracker.save_results_to_file(str(path), frame, ped, 2, (375, 1242), rles, np.ones(6, bool))
    with pytest.raises(capi.MpnhipError):
        tracker.save_results_to_file(str(path), frame[:3], ped, 2, (375, 1242), rles, keep)
