"""The batched COCO run-length codec (``csrc/rle_codec.hip``) without a device: the size queries and argument checks of its C
entry points, ``masks.rle_strings``, and the host logic of the device paths of ``mots_eval.load_mots_txt`` -- which row of a file
is refused, and why, from hand-made status words.  What the kernels compute is tests/test_gpu_rle_codec.py's."""
import ctypes

import numpy as np
import pytest

from mpntrackseg_amd import capi, gt_assign, masks as M, mots_eval as ME, tracker

MPNHIP_ERR_ARG, MPNHIP_ERR_WORKSPACE = -1, -3   # include/mpnhip.h


def test_workspace_queries_grow_with_their_sizes():
    l = capi.load()
    enc, dec = l.mpnhip_rle_encode_workspace_bytes, l.mpnhip_rle_decode_workspace_bytes
    assert enc(0, 0) == 0 and dec(0) == 0
    # per entry two offsets, per count (one per event and one per entry) a length and an offset, int64 each
    assert enc(240, 0) >= 2 * 8 * 241 + 2 * 8 * 241
    assert enc(240, 100000) >= enc(240, 0) + 2 * 8 * 100000
    assert enc(4000, 100000) > enc(240, 100000)
    assert dec(10) >= 8 * 11 and dec(100000) >= dec(10) + 8 * 99990
    for bad in ((-1, 5), (5, -1), (1 << 30, 5), (5, 1 << 31)):
        assert enc(*bad) == 0, bad
    assert dec(-1) == 0 and dec(1 << 30) == 0


def test_entry_points_argument_checks_without_gpu():
    """Empty inputs are successful no-ops; null pointers, bad sizes, an undersized capacity and a short workspace are refused
    before any launch, with the entry's name in mpnhip_last_error()."""
    l = capi.load()
    one = ctypes.c_void_p(256)   # a non-null address that no call below may reach a launch with
    big = 1 << 30
    hw = 1080 * 1920
    enc = l.mpnhip_rle_encode
    assert enc(None, None, 0, 0, hw, None, 0, None, None, 0, None) == 0
    assert enc(None, None, 0, 0, 0, None, 0, None, None, 0, None) == 0
    # the capacity that always suffices is 7 * (n_events + n_dets): one less is refused, whatever else is right
    assert enc(one, one, 5, 100, hw, one, 7 * 105 - 1, one, one, big, None) == MPNHIP_ERR_ARG
    assert b"rle_encode" in l.mpnhip_last_error() and b"bytes_capacity" in l.mpnhip_last_error()
    assert enc(one, one, 5, 0, hw, one, 34, one, one, big, None) == MPNHIP_ERR_ARG
    assert enc(one, one, 5, 100, hw, one, -1, one, one, big, None) == MPNHIP_ERR_ARG
    for bad in (dict(n_dets=-1), dict(n_events=-1), dict(hw=-1), dict(hw=1 << 31), dict(n_events=1 << 31), dict(n_dets=1 << 30)):
        a = dict(n_dets=5, n_events=100, hw=hw)
        a.update(bad)
        assert enc(one, one, a["n_dets"], a["n_events"], a["hw"], one, 1 << 40, one, one, big, None) == MPNHIP_ERR_ARG, bad
        assert b"rle_encode" in l.mpnhip_last_error()
    assert enc(None, one, 5, 100, hw, one, 7 * 105, one, one, big, None) == MPNHIP_ERR_ARG     # events without positions
    assert enc(one, None, 5, 100, hw, one, 7 * 105, one, one, big, None) == MPNHIP_ERR_ARG
    assert enc(one, one, 5, 100, hw, None, 7 * 105, one, one, big, None) == MPNHIP_ERR_ARG
    assert enc(one, one, 5, 100, hw, one, 7 * 105, None, one, big, None) == MPNHIP_ERR_ARG
    assert b"rle_encode" in l.mpnhip_last_error()
    assert enc(one, one, 5, 100, hw, one, 7 * 105, one, one, 16, None) == MPNHIP_ERR_WORKSPACE
    assert enc(one, one, 5, 100, hw, one, 7 * 105, one, None, 0, None) == MPNHIP_ERR_WORKSPACE
    assert enc(None, one, 5, 0, hw, one, 35, one, None, 0, None) == MPNHIP_ERR_WORKSPACE       # no event: positions not needed
    assert b"rle_encode" in l.mpnhip_last_error()

    scan = l.mpnhip_rle_decode_scan
    assert scan(None, 0, None, None, 0, None, None, None, None, None) == 0
    assert scan(one, -1, one, one, 3, one, one, one, one, None) == MPNHIP_ERR_ARG
    assert b"rle_decode_scan" in l.mpnhip_last_error()
    assert scan(one, 1 << 31, one, one, 3, one, one, one, one, None) == MPNHIP_ERR_ARG
    assert scan(one, 10, one, one, -1, one, one, one, one, None) == MPNHIP_ERR_ARG
    for k in (0, 2, 3, 5, 6, 7, 8):   # every pointer is needed
        args = [one, 10, one, one, 3, one, one, one, one]
        args[k] = None
        assert scan(*args, None) == MPNHIP_ERR_ARG, k
        assert b"rle_decode_scan" in l.mpnhip_last_error()

    runs = l.mpnhip_rle_decode_runs
    assert runs(None, 0, None, None, 0, None, None, 0, None, None, None, None, None, 0, None) == 0
    ok = [one, 10, one, one, 3, one, one, 4, one, one, one, one, one, big]
    for pos, value in ((1, -1), (1, 1 << 31), (4, -1), (4, 1 << 30), (7, -1), (7, 1 << 31)):
        args = list(ok)
        args[pos] = value
        assert runs(*args, None) == MPNHIP_ERR_ARG, (pos, value)
        assert b"rle_decode_runs" in l.mpnhip_last_error()
    for pos in (0, 2, 3, 5, 6, 8, 9, 10, 11):
        args = list(ok)
        args[pos] = None
        assert runs(*args, None) == MPNHIP_ERR_ARG, pos
        assert b"rle_decode_runs" in l.mpnhip_last_error()
    args = list(ok)
    args[13] = 16
    assert runs(*args, None) == MPNHIP_ERR_WORKSPACE
    args[12], args[13] = None, 0
    assert runs(*args, None) == MPNHIP_ERR_WORKSPACE
    assert b"rle_decode_runs" in l.mpnhip_last_error()
    args = list(ok)             # no run to write: the run arrays are not needed -- reaches the workspace check
    args[7], args[9], args[10], args[11], args[13] = 0, None, None, None, 16
    assert runs(*args, None) == MPNHIP_ERR_WORKSPACE


def test_rle_strings_slices():
    strings = ["", M.rle_string([5, 3, 2]), "", "", M.rle_string([0, 2073600]), M.rle_string([100, 40000, 5, 39000, 7]), ""]
    data = np.frombuffer("".join(strings).encode("ascii"), np.uint8)
    ptr = np.concatenate(([0], np.cumsum([len(s) for s in strings])))
    got = M.rle_strings(data, ptr)
    assert got == strings and all(type(s) is str for s in got)
    assert M.rle_strings(np.zeros(0, np.uint8), [0]) == []
    assert M.rle_strings(np.zeros(0, np.uint8), [0, 0, 0]) == ["", ""]
    assert M.rle_strings(list(data), ptr.astype(np.int32)) == strings


def test_status_words_name_the_host_codecs_refusals():
    assert M.rle_status_error(0) is None and M.rle_status_error(M.RLE_NEGATIVE | M.RLE_BAD_SUM) is None
    for string, bit in (("/", M.RLE_BAD_CHAR), ("p", M.RLE_BAD_CHAR), ("o", M.RLE_TRUNCATED), ("o" * 12 + "1", M.RLE_TOO_LONG)):
        with pytest.raises(ValueError) as e:
            M.rle_counts(string)
        assert str(e.value) == M.rle_status_error(bit)
    # the host looks at the characters first, then at the end, then at the lengths
    assert M.rle_status_error(7) == M.rle_status_error(1) and M.rle_status_error(6) == M.rle_status_error(2)
    assert (M.RLE_BAD_CHAR, M.RLE_TRUNCATED, M.RLE_TOO_LONG, M.RLE_NEGATIVE, M.RLE_BAD_SUM) == (1, 2, 4, 8, 16)
    assert M.RLE_UNREADABLE == 7


def test_first_refused_row():
    """``mots_eval.first_refused_row``: the first bad row in file order decides, and inside a row the loader's order -- a string
    that does not parse, a duplicate id, an unknown class, counts that do not describe the image."""
    f = ME.first_refused_row
    frame, tid, cls = [0, 0, 1, 1, 2], [2001, 2002, 2001, 10000, 2002], [2, 2, 2, 10, 2]
    h, w, ok = [5] * 5, [4] * 5, [0] * 5
    assert f(frame, tid, cls, h, w, ok) is None
    assert f([], [], [], [], [], []) is None
    for bit in (1, 2, 4, 3, 7):
        assert f(frame, tid, cls, h, w, [0, 0, bit, 0, 0]) == (2, "parse")
    for bit in (8, 16, 24):
        assert f(frame, tid, cls, h, w, [0, 0, 0, bit, 0]) == (3, "counts")
    assert f(frame, tid, cls, [5, 5, 5, 5, -5], w, ok) == (4, "counts")
    assert f(frame, tid, cls, h, [4, -4, 4, 4, 4], ok) == (1, "counts")
    assert f(frame, tid, [2, 2, 3, 10, 2], h, w, ok) == (2, "class")
    assert f(frame, tid, [2, 2, 2, 10, 0], h, w, ok) == (4, "class")
    # a duplicate is the LATER row of the pair; the same id in another frame is none
    assert f([0, 0, 1, 1, 0], [2001, 2002, 2001, 10000, 2001], cls, h, w, ok) == (4, "duplicate")
    assert f([0, 0, 0, 1, 2], [2001, 2002, 2001, 10000, 2002], cls, h, w, ok) == (2, "duplicate")
    # several bad rows: the first one in file order, whatever its kind
    assert f(frame, tid, [2, 2, 2, 10, 7], h, w, [0, 16, 0, 0, 1]) == (1, "counts")
    assert f(frame, tid, [2, 7, 2, 10, 2], h, w, [0, 0, 0, 0, 1]) == (1, "class")
    assert f([0, 0, 0, 1, 2], [2001, 2001, 2001, 10000, 2002], [2, 2, 9, 10, 2], h, w, [0, 0, 2, 16, 0]) == (1, "duplicate")
    # several reasons in one row: parse, then duplicate, then class, then counts
    both = ([0, 0], [2001, 2001], [2, 5], [5, -5], [4, 4])
    assert f(*both, [0, 1 | 16]) == (1, "parse")
    assert f(*both, [0, 16]) == (1, "duplicate")
    assert f([0, 0], [2001, 2002], [2, 5], [5, -5], [4, 4], [0, 16]) == (1, "class")
    assert f([0, 0], [2001, 2002], [2, 2], [5, -5], [4, 4], [0, 0]) == (1, "counts")
    # a third row of an id is a duplicate as well (of either earlier one)
    assert f([3, 3, 3], [7, 7, 7], [2, 2, 2], [1] * 3, [1] * 3, [0, 0, 0]) == (1, "duplicate")


def test_python_entry_points_refuse_host_tensors_and_bad_switches(tmp_path):
    import torch
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        M.mask_run_strings(torch.zeros((1, 8, 8), dtype=torch.int32), 1)
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        M.rle_encode_events(torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 64)
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        M.rle_decode_batch(["0"], 1, 1, "cpu")
    path = tmp_path / "rows.txt"
    path.write_text("0 2001 2 1 1 01\n")
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        ME.load_mots_txt(str(path), device="cpu")
    assert ME.load_mots_txt(str(path))["area"].tolist() == [1]       # the default is the host path
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        gt_assign.mask_rows({"frame": [0], "img_height": [1], "img_width": [1], "rle": np.array(["01"], object)}, device="cpu")
    with pytest.raises(capi.MpnhipError, match="strings must be"):
        tracker.to_full_masks(torch.zeros(1, 1, 4, 4), np.zeros((1, 4)), [0], [True], (8, 8), strings="gpu")
    with pytest.raises(capi.MpnhipError, match="strings must be"):
        gt_assign._strings_device("gpu", None)
