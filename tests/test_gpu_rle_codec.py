"""The batched COCO run-length codec on the device (``csrc/rle_codec.hip`` through ``mpntrackseg_amd.masks``) against the host codec
-- ``masks.rle_string``, ``rle_counts_from_events``, ``rle_counts`` and ``mots_eval.counts_to_runs``, which
tests/test_full_masks_cpu.py pins to the evaluation kit's sample line and to the reference's strings -- and its three consumers
against their host paths.  Bytes and integers: every comparison is for equality."""
import numpy as np
import pytest
import torch

import gt_assign_ref as GR
import hota_ref as HR
import mots_metrics_ref as R
from mpntrackseg_amd import capi, gt_assign, masks as M, mots_eval as ME, tracker

pytestmark = pytest.mark.gpu

H, W = 37, 53
FULL_HD, INT_MAX = 1080 * 1920, 2 ** 31 - 1


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ helpers
def counts_of_stored(stored):
    """the counts whose stored values (rleToString's: count i >= 3 minus count i - 2) are ``stored``"""
    c = [int(v) for v in stored]
    for i in range(3, len(c)):
        c[i] += c[i - 2]
    return c


def stored_of_counts(counts):
    c = np.asarray(counts, np.int64)
    x = c.copy()
    x[3:] -= c[1:-2]
    return x.tolist()


def closed(counts, hw):
    """``counts`` with the one more count that makes them sum to ``hw``"""
    rest = hw - sum(counts)
    assert rest > 0
    return list(counts) + [rest]


def device_strings(entries, hw):
    """encode on the device the entries given as lists of counts summing to hw (their boundaries: the running sums but the last)"""
    for c in entries:
        assert sum(c) == hw and len(c) >= 1
    pos = [np.cumsum(c)[:-1] for c in entries]
    cnt = np.asarray([p.size for p in pos], np.int32)
    flat = np.concatenate(pos).astype(np.int32) if pos else np.zeros(0, np.int32)
    data, sp = M.rle_encode_events(torch.from_numpy(flat).to(dev()), torch.from_numpy(cnt).to(dev()), hw)
    sp = sp.cpu().numpy()
    assert sp.dtype == np.int64 and sp.shape == (len(entries) + 1,) and sp[0] == 0 and (np.diff(sp) >= 0).all()
    assert data.dtype == torch.uint8 and data.numel() >= 7 * (flat.size + cnt.size) and int(sp[-1]) <= 7 * (flat.size + cnt.size)
    return M.rle_strings(data[:int(sp[-1])].cpu().numpy(), sp)


def check_encode(entries, hw):
    got = device_strings(entries, hw)
    want = [M.rle_string(M.rle_counts_from_events(np.cumsum(c)[:-1], hw)) for c in entries]
    assert got == want
    for s, c in zip(got, entries):       # ... and they are the strings of these counts
        assert M.rle_counts(s).tolist() == list(c)
    return got


STATUS_OF = {"not a COCO run-length string": M.RLE_BAD_CHAR, "truncated COCO run-length string": M.RLE_TRUNCATED,
             "count too long": M.RLE_TOO_LONG}


def host_decode(s, hw):
    """(n_counts or None, begin, end, area, status) of one string by the host codec"""
    none = np.zeros(0, np.int64)
    try:
        c = M.rle_counts(s)
    except ValueError as e:
        return None, none, none, 0, STATUS_OF[str(e)]
    status = (M.RLE_NEGATIVE if c.size and c.min() < 0 else 0) | (M.RLE_BAD_SUM if int(c.sum()) != hw else 0)
    if status:
        return c.size, none, none, 0, status
    b, e = ME.counts_to_runs(c)
    return c.size, b, e, int((e - b).sum()), 0


def check_decode(strings, hw):
    """decode on the device against the host codec, string by string; returns the device's dict with the runs on the host"""
    hw = np.broadcast_to(np.asarray(hw, np.int64), (len(strings),))
    d = M.rle_decode_batch(strings, hw, np.ones(len(strings), np.int64), dev())
    assert list(d) == ["n_counts", "n_runs", "area", "status", "run_ptr", "run_row", "run_begin", "run_end"]
    for k in ("run_row", "run_begin", "run_end"):
        assert d[k].dtype == torch.int32 and d[k].is_cuda
        d[k] = d[k].cpu().numpy()
    for k in ("n_counts", "n_runs", "area", "status", "run_ptr"):
        assert d[k].dtype == np.int64
    assert d["run_ptr"].tolist() == np.concatenate(([0], np.cumsum(d["n_runs"]))).tolist()
    assert d["run_row"].size == d["run_begin"].size == d["run_end"].size == int(d["run_ptr"][-1])
    for i, s in enumerate(strings):
        n, b, e, area, status = host_decode(s, int(hw[i]))
        a, z = int(d["run_ptr"][i]), int(d["run_ptr"][i + 1])
        got = int(d["status"][i])
        if got & M.RLE_UNREADABLE:       # the device names every reason a string cannot be read, the host the first it meets
            assert got & ~M.RLE_UNREADABLE == 0
            got &= -got
        assert got == status, (i, s)
        assert n is None or int(d["n_counts"][i]) == n, (i, s)
        assert d["run_begin"][a:z].tolist() == b.tolist() and d["run_end"][a:z].tolist() == e.tolist(), (i, s)
        assert (d["run_row"][a:z] == i).all() and int(d["area"][i]) == area and int(d["n_runs"][i]) == b.size
    return d


# ------------------------------------------------------------------------------------------------ encoder
def test_encoder_value_boundaries():
    """the stored values at which the number of characters changes, as raw counts (index < 3) and as differences (index >= 3)"""
    hw = FULL_HD
    entries = [
        closed([15, 16, 15, 16 + 15, 15 + 16], hw),          # raw 15 / 16 / 15, differences 15 and 16
        closed([16, 20, 17, 4, 1, 3], hw),                   # differences -16, -16, -1 ... and -17:
        closed([1, 20, 1, 3, 1, 3], hw),                     # -17, 0, 0
        closed([0, 7, 0, 7, 0, 7], hw),                      # a leading 0, differences of 0
        closed([31, 32, 511, 512, 513, 16383, 16384], hw),   # 2 / 3 characters
        closed([524287, 524288, 5, 1000000], hw),            # 4 and 5 characters (hw is 5 itself), a difference of 5 characters
        closed([5, 600000, 5, 7, 5], hw),                    # a negative difference of 5 characters
    ]
    stored = [stored_of_counts(c) for c in entries]
    assert stored[0][:5] == [15, 16, 15, 15, 16] and stored[1][3] == -16 and stored[2][3] == -17 and 0 in stored[2][3:]
    assert stored[3][0] == 0 and stored[3][3:6] == [0, 0, 0] and stored[6][3] == 7 - 600000
    check_encode(entries, hw)
    one = lambda v: len(M.rle_string([v]))
    assert [one(v) for v in (15, 16, -16, -17, 0, 524287, 524288, hw)] == [1, 2, 1, 2, 1, 4, 5, 5]
    # 7 characters: counts and differences of 2^29 and more, both signs, in an image of 2^31 - 1 pixels
    big = INT_MAX
    entries = [[big], [0, big], closed([1, 2 ** 30, 1, 5, 2 ** 29, 5, 3], big), closed([2 ** 29 - 1, 2 ** 29, 7], big),
               closed([big - 3, 1], big)]
    stored = stored_of_counts(entries[2])
    assert stored[3] == 5 - 2 ** 30 and one(big) == 7 and one(5 - 2 ** 30) == 7 and one(2 ** 29 - 1) == 6 and one(2 ** 29) == 7
    check_encode(entries, big)


def test_encoder_structure():
    hw = H * W
    rng = np.random.default_rng(11)
    long_entry = np.diff(np.concatenate(([0], np.sort(rng.choice(np.arange(1, hw), 700, replace=False)), [hw]))).tolist()
    entries = [
        [hw],                                 # no event: the one count hw
        [100, hw - 100],                      # one event: the mask runs to the end of the image
        [0, 9, hw - 9],                       # a first event at position 0
        [0, hw],                              # ... the full image
        [5, 6, hw - 11],                      # three counts: no difference is stored
        [5, 6, 7, hw - 18],                   # four: the first one
        [hw], [hw], [hw],                     # empty entries side by side
        long_entry,                           # 701 counts: several blocks of the scan
        [hw - 1, 1],                          # the last pixel alone
        [hw],
    ]
    assert len(long_entry) == 701 and min(long_entry) >= 1
    n_counts = sum(len(c) for c in entries)
    assert n_counts > 2 * 256 and n_counts % 256 != 0        # the last block is partial
    got = check_encode(entries, hw)
    assert got[0] == got[6] == got[-1] == M.rle_string([hw]) and got[3] == M.rle_string([0, hw])
    # many entries, most of them short
    many = []
    for _ in range(333):
        k = int(rng.choice([0, 0, 1, 2, 3, 4, 9, 40]))
        cuts = np.sort(rng.choice(np.arange(0, hw), k, replace=False))
        many.append(np.diff(np.concatenate(([0], cuts, [hw]))).tolist())
    check_encode(many, hw)
    # no entry at all: one offset
    assert device_strings([], hw) == []
    data, sp = M.rle_encode_events(torch.zeros(0, dtype=torch.int32, device=dev()), torch.zeros(0, dtype=torch.int32, device=dev()), hw)
    assert sp.cpu().tolist() == [0]


def test_encoder_refuses_an_undersized_capacity():
    lib = capi.load()
    d = dev()
    pos, cnt = torch.tensor([3, 9, 20], dtype=torch.int32, device=d), torch.tensor([2, 0, 1], dtype=torch.int32, device=d)
    need = 7 * (3 + 3)
    data = torch.full((need,), 0x55, dtype=torch.uint8, device=d)
    sp = torch.full((4,), -7, dtype=torch.int64, device=d)
    ws = torch.empty(lib.mpnhip_rle_encode_workspace_bytes(3, 3), dtype=torch.uint8, device=d)
    args = lambda cap: (capi.ptr(pos), capi.ptr(cnt), 3, 3, 100, capi.ptr(data), cap, capi.ptr(sp), capi.ptr(ws), ws.numel(), capi.stream_ptr())
    assert lib.mpnhip_rle_encode(*args(need - 1)) == -1
    assert b"rle_encode" in lib.mpnhip_last_error() and b"bytes_capacity" in lib.mpnhip_last_error()
    torch.cuda.synchronize()
    assert (data == 0x55).all() and (sp == -7).all()          # refused before any launch
    assert lib.mpnhip_rle_encode(*args(need)) == 0
    sp_h = sp.cpu().numpy()
    want = [M.rle_string([3, 6, 91]), M.rle_string([100]), M.rle_string([20, 80])]
    assert M.rle_strings(data[:int(sp_h[-1])].cpu().numpy(), sp_h) == want
    assert (data[int(sp_h[-1]):] == 0x55).all()


# ------------------------------------------------------------------------------------------------ decoder
def chunk_strings():
    """strings of 64, 65 and 129 characters: one-character counts, and a longer one across characters 63 | 64 and 127 | 128"""
    singles = lambda n: [int(v) for v in np.random.default_rng(n).integers(0, 4, n)]
    s64 = counts_of_stored([4, 5, 6] + singles(59) + [100])                                        # 62 + 2 characters
    s65 = counts_of_stored([4, 5, 6] + singles(59) + [1000])                                       # 62 + 3
    s129 = counts_of_stored([4, 5, 6] + singles(59) + [1000] + singles(61) + [-900])               # 62 + 3 + 61 + 3
    s129b = counts_of_stored([4, 5, 6] + singles(60) + [40000, 100] + singles(58) + [300000])      # 63 + 4 + 2 + 58 + 4, an even number
    return [s64, s65, s129, s129b]


def test_decoder_chunks():
    counts = chunk_strings()
    strings = [M.rle_string(c) for c in counts]
    assert [len(s) for s in strings] == [64, 65, 129, 131] and [len(c) % 2 for c in counts] == [1, 1, 1, 0]
    more = lambda s, i: (ord(s[i]) - 48) & 0x20 != 0
    assert more(strings[0], 62) and not more(strings[0], 63)
    assert more(strings[1], 63) and more(strings[2], 63) and more(strings[2], 127) and more(strings[3], 63) and more(strings[3], 127)
    assert all(min(c) >= 0 for c in counts)
    d = check_decode(strings, [sum(c) for c in counts])
    assert (d["status"] == 0).all() and d["n_counts"].tolist() == [len(c) for c in counts]
    # the same strings in another order, between short ones: a wavefront's string does not depend on its neighbours
    mixed = ["", strings[2], "5", strings[0], strings[3], M.rle_string([0, 4]), strings[1]]
    check_decode(mixed, [0, sum(counts[2]), 5, sum(counts[0]), sum(counts[3]), 4, sum(counts[1])])


def test_decoder_small_strings():
    strings = ["", "", "5", M.rle_string([3, 2, 0, 4]), M.rle_string([9]), M.rle_string([5, 0, 4]), M.rle_string([0, 9]),
               M.rle_string([0, 0, 9]), M.rle_string([2, 3, 4]), M.rle_string([2, 3, 1, 3]), M.rle_string([1] * 9)]
    hw = [0, 9, 5, 9, 9, 9, 9, 9, 9, 9, 9]
    d = check_decode(strings, hw)
    assert d["status"].tolist() == [0, M.RLE_BAD_SUM] + [0] * 9
    assert d["n_counts"].tolist() == [0, 0, 1, 4, 1, 3, 2, 3, 3, 4, 9]
    a = int(d["run_ptr"][3])
    assert d["run_begin"][a:a + 2].tolist() == [3, 5] and d["run_end"][a:a + 2].tolist() == [5, 9]      # adjacent runs stay two
    assert d["area"].tolist() == [0, 0, 0, 6, 0, 0, 9, 0, 3, 6, 4] and d["n_runs"].tolist() == [0, 0, 0, 2, 0, 0, 1, 0, 1, 2, 4]
    assert M.rle_decode_batch([], 5, 5, dev())["run_ptr"].tolist() == [0]


def test_decoder_refusals():
    """one string per status bit, a good string before and behind each; then the bits in the strings of the chunk test"""
    good = M.rle_string([3, 2, 4])
    bad = [("3/4", 9, M.RLE_BAD_CHAR), ("3p4", 9, M.RLE_BAD_CHAR), (good + "o", 9, M.RLE_TRUNCATED), ("o" * 12 + "1", 9, M.RLE_TOO_LONG),
           (M.rle_string([10, -3, 5]), 12, M.RLE_NEGATIVE), (good, 10, M.RLE_BAD_SUM), (good, 8, M.RLE_BAD_SUM),
           (M.rle_string([3, 7, -1]), 9, M.RLE_NEGATIVE), (M.rle_string([3, -5, 4]), 9, M.RLE_NEGATIVE | M.RLE_BAD_SUM),
           ("o" * 11 + "1", 9, M.RLE_BAD_SUM), ("o" * 11 + "O", 9, M.RLE_NEGATIVE | M.RLE_BAD_SUM), (good, -1, M.RLE_BAD_SUM)]
    strings, hw, want = [good], [9], [0]
    for s, n, status in bad:
        strings += [s, good]
        hw += [n, 9]
        want += [status, 0]
    d = check_decode(strings, hw)
    assert d["status"].tolist() == want
    assert d["n_runs"].tolist() == [1 - (s != 0) for s in want] and d["area"].tolist() == [2 * (s == 0) for s in want]
    # a bad character, a cut and a count of 13 groups at every place of the long strings, the chunk borders among them
    base = M.rle_string(chunk_strings()[2])
    total = sum(chunk_strings()[2])
    variants, sizes = [], []
    for i in (0, 1, 62, 63, 64, 65, 126, 127, 128):
        variants += [base[:i] + "/" + base[i + 1:], base[:i] + "p" + base[i + 1:], base[:i + 1] if (ord(base[i]) - 48) & 0x20 else base[:i] + "o",
                     base[:i] + "o" * 13 + base[i:], base]
        sizes += [total] * 5
    d = check_decode(variants, sizes)
    assert (d["status"].reshape(-1, 5)[:, :4] != 0).all() and (d["status"].reshape(-1, 5)[:, 4] == 0).all()


# ------------------------------------------------------------------------------------------------ round trips
def test_random_masks_round_trip():
    rng = np.random.default_rng(12)
    n = 200
    dens = np.concatenate(([0.0, 1.0], rng.choice([0.01, 0.1, 0.5, 0.9, 0.99], n - 2)))
    masks = rng.random((n, H, W)) < dens[:, None, None]
    masks[5, 0, 0], masks[6, -1, -1], masks[7, 0, 0], masks[8, -1, -1] = True, True, False, False
    assert not masks[0].any() and masks[1].all()
    want = [GR.rle_of(m) for m in masks]
    # one mask per frame: frame f holds detection f
    labels = torch.from_numpy(np.where(masks.transpose(0, 2, 1), np.arange(n, dtype=np.int32)[:, None, None], np.int32(-1)).astype(np.int32)).to(dev())
    data, sp = M.mask_run_strings(labels, n)
    assert data.dtype == np.uint8 and sp.dtype == np.int64 and data.size == sp[-1]
    got = M.rle_strings(data, sp)
    assert got == want
    # the host's runs, and the boundaries the strings came from
    d = check_decode(got, H * W)
    assert (d["status"] == 0).all() and d["area"].tolist() == masks.reshape(n, -1).sum(axis=1).tolist()
    pos, counts = M.mask_run_events(labels, n)
    ends = np.cumsum(counts)
    for i in range(n):
        a, z = int(d["run_ptr"][i]), int(d["run_ptr"][i + 1])
        ev = np.stack((d["run_begin"][a:z], d["run_end"][a:z]), axis=1).reshape(-1)
        assert ev[ev < H * W].tolist() == pos[ends[i] - counts[i]:ends[i]].tolist()
    # the runs paint the masks back
    frame_ptr = np.arange(n + 1)
    back = ME.paint_label_runs(torch.from_numpy(d["run_row"]).to(dev()), torch.from_numpy(d["run_begin"]).to(dev()),
                               torch.from_numpy(d["run_end"]).to(dev()), frame_ptr, n, H * W, dev())
    assert torch.equal(back.view(n, W, H), labels)


# ------------------------------------------------------------------------------------------------ consumers
@pytest.mark.parametrize("frames_per_launch", (1, 4))
def test_to_full_masks_with_device_strings(golden, frames_per_launch):
    z = golden("g20_full_masks.npz")
    (h, w), thr = z["img_shape"].tolist(), float(z["mask_threshold"])
    frame = np.array([1] * 6 + [2] + [4] * 4)
    node_preds = torch.from_numpy(z["masks"]).view(11, 1, 56, 56).to(dev())
    for keep in (np.ones(11, bool), np.array([1, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1], bool), np.zeros(11, bool)):
        want = tracker.to_full_masks(node_preds, z["boxes"], frame, keep, (h, w), thr, frames_per_launch=frames_per_launch)
        got = tracker.to_full_masks(node_preds, z["boxes"], frame, keep, (h, w), thr, frames_per_launch=frames_per_launch, strings='device')
        assert got.dtype == object and got.shape == (11,) and got.tolist() == want.tolist()
        assert all(s is None or type(s) is str for s in got)


def same_dict(got, want):
    assert list(got) == list(want)
    for k in want:
        assert isinstance(got[k], np.ndarray) and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def test_load_mots_txt_on_the_device(tmp_path):
    g22, g23 = dict(np.load(R.GOLDEN)), dict(np.load(HR.GOLDEN))
    n_rows = 0
    for scene in HR.SCENES:
        gt, pred, _ = HR.scene_images(g23, g22, scene)
        for side, ids in (("gt", gt), ("pred", pred)):
            path = R.write_txt(str(tmp_path / ("%s_%s.txt" % (scene, side))), R.id_image_rows(ids))
            want = ME.load_mots_txt(path)
            same_dict(ME.load_mots_txt(path, device=dev()), want)
            n_rows += want["frame"].size
            assert (want["area"] > 0).all() and want["run_row"].size >= want["frame"].size
    assert n_rows > 50
    empty = R.write_txt(str(tmp_path / "empty.txt"), [])
    same_dict(ME.load_mots_txt(empty, device=dev()), ME.load_mots_txt(empty))
    blank = R.write_txt(str(tmp_path / "blank.txt"), ["", "0 2001 2 3 3 " + M.rle_string([2, 3, 4]), "  "])
    same_dict(ME.load_mots_txt(blank, device=dev()), ME.load_mots_txt(blank))


def test_load_mots_txt_on_the_device_refuses_what_the_host_path_refuses(tmp_path):
    g22 = dict(np.load(R.GOLDEN))
    rows = R.id_image_rows(g22["cases:gt"])
    first = rows[0].split(" ")
    cut = " ".join(first[:5] + [first[5] + "o"])
    wrong = " ".join(first[:3] + [str(int(first[3]) + 1)] + first[4:])
    files = {
        "duplicate": rows + [rows[0]],
        "class": rows + [" ".join([first[0], "3999", "3"] + first[3:])],
        "overlap": rows + [" ".join([first[0], "2999"] + first[2:])],
        "fields": ["x 1 2 3"],
        # two bad rows: the first one in file order decides, whichever path finds it
        "class_then_string": rows[:3] + [" ".join([first[0], "3999", "3"] + first[3:])] + rows[3:] + [cut],
        "string_then_class": rows[:3] + [" ".join([first[0], "4999"] + first[2:5] + [first[5] + "o"])] + rows[3:] + [" ".join([first[0], "3999", "3"] + first[3:])],
        "counts_then_fields": rows[:5] + [" ".join([first[0], "5999"] + first[2:3] + wrong.split(" ")[3:])] + ["7 8"] + rows[5:],
        "fields_then_counts": rows[:5] + ["7 8 2 x 5 11"] + [wrong],
        "one_row_many_reasons": rows + [" ".join(first[:2] + ["3"] + first[3:5] + [first[5] + "/"])],
        "duplicate_of_unknown_class": rows + [" ".join(first[:2] + ["3"] + first[3:])],
        "short_row": rows + ["1 2 2 5 5"],
        "negative_size": rows + ["0 4999 2 -5 4 " + M.rle_string([20])],
    }
    messages = {}
    for name, lines in files.items():
        path = R.write_txt(str(tmp_path / "bad.txt"), lines)
        with pytest.raises(ValueError) as host:
            ME.load_mots_txt(path)
        with pytest.raises(ValueError) as device:
            ME.load_mots_txt(path, device=dev())
        assert type(device.value) is ValueError and str(device.value) == str(host.value), name
        messages[name] = str(host.value)
    assert "Multiple objects" in messages["duplicate"] and "Unknown object class" in messages["class"]
    assert "overlapping masks" in messages["overlap"] and "Error in bad.txt" in messages["fields"]
    assert "Unknown object class" in messages["class_then_string"] and "Error in bad.txt" in messages["string_then_class"]
    assert "do not describe" in messages["counts_then_fields"] and "Error in bad.txt in line: 7 8 2 x" in messages["fields_then_counts"]
    assert "Error in bad.txt" in messages["one_row_many_reasons"] and "Multiple objects" in messages["duplicate_of_unknown_class"]
    assert "do not describe a -5 x 4" in messages["negative_size"]


def test_mask_rows_on_the_device():
    det, gt, _ = GR.mask_scene()
    for rows in (det, gt):
        want = gt_assign.mask_rows(rows)
        same_dict(gt_assign.mask_rows(rows, device=dev()), want)
        assert want["run_row"].size > want["frame"].size
    # strings as bytes, and the refusals with the host path's words
    as_bytes = dict(gt, rle=np.array([s.encode("ascii") for s in gt["rle"]], dtype=object))
    same_dict(gt_assign.mask_rows(as_bytes, device=dev()), gt_assign.mask_rows(gt))
    for k, change in ((2, lambda s: s + "o"), (1, lambda s: "/" + s), (3, lambda s: M.rle_string([5])), (0, lambda s: "o" * 13 + s)):
        bad = dict(gt, rle=gt["rle"].copy())
        bad["rle"][k] = change(bad["rle"][k])
        with pytest.raises(ValueError) as host:
            gt_assign.mask_rows(bad)
        with pytest.raises(ValueError) as device:
            gt_assign.mask_rows(bad, device=dev())
        assert type(device.value) is ValueError and str(device.value) == str(host.value)
    # the two steps that read mask rows give the same with either decoder
    want = gt_assign.assign_gt(det, gt, 0.2, mask_priority=True, device=dev())
    got = gt_assign.assign_gt(det, gt, 0.2, mask_priority=True, device=dev(), strings="device")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and (want[0] >= 0).any()
    m_want, v_want = gt_assign.gt_roi_masks(det, gt, want[1], size=(14, 14))
    m_got, v_got = gt_assign.gt_roi_masks(det, gt, want[1], size=(14, 14), strings="device")
    assert torch.equal(m_got, m_want) and torch.equal(v_got, v_want) and bool(v_want.any())
