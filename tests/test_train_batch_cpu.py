"""The host side of the training sampler (``mpntrackseg_amd/dataset.py``) and the numpy restatement of the device operators
(``tests/train_batch_ref.py``) against the reference's own ``MOTGraphDataset`` / ``MOTGraph`` / ``MOTGraphAugmentor``, recorded in
tests/golden/g25_train_samples.npz by tools/make_golden_train_batch.py; and the host-side argument checks of the new entry
points.  No GPU.

Tolerances: integers, the float64 boxes and their float32 casts are exact.  ``edge_attr`` is compared within rtol = atol = 2e-6,
the bound tests/test_gpu_tracker.py uses for g14: ``log`` and the division differ between libraries by an ulp of float32
(6e-8 relative), and the embedding distance is summed in another order."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_ref as R  # noqa: E402
from mpntrackseg_amd import capi, dataset  # noqa: E402


@pytest.fixture(scope="module")
def g25(golden):
    z = golden("g25_train_samples.npz")
    return (z,) + R.fixture(z)


def test_seq_step_size_matches_the_reference(g25):
    z, params, tables, _ = g25
    for fps, mov, step in z["step_sizes"]:
        assert dataset.seq_step_size(int(fps), bool(mov), params["target_fps_dict"]) == step, (fps, mov)
    assert any(fps / params["target_fps_dict"]["moving" if mov else "static"] % 1 == 0.5 for fps, mov, _ in z["step_sizes"])   # a tie
    for t in tables:
        assert dataset.seq_step_size(t["fps"], t["mov_camera"], params["target_fps_dict"]) == t["step_size"]


def test_index_dataset_matches_the_reference(g25):
    z, _, tables, _ = g25
    keys = [k for k in z.files if k.startswith("index:")]
    assert len(keys) >= 6
    for k in keys:
        _, name, cfg = k.split(":")
        step, fpg, mind = (int(v) for v in cfg.split("_"))
        got = dataset.index_dataset(tables[R.SEQS.index(name)]["frame"], step, fpg, mind)
        assert got.dtype == np.int64 and np.array_equal(got, z[k]), k
    assert z["index:B:2_15_25"].size == 0 and z["index:A:1_5_4"].size > 20


def test_window_rows_match_the_reference(g25):
    z, _, tables, _ = g25
    tags = sorted(k.split(":")[1] for k in z.files if k.startswith("rows:") and k.endswith(":args"))
    assert {"fpg_cut", "max_detects_cut", "end", "end_ensure", "tail_one_frame", "tail_empty"} <= set(tags)
    for tag in tags:
        seq, start, step, fpg, maxd, end, ensure = (int(v) for v in z[f"rows:{tag}:args"])
        t = tables[seq]
        rows = dataset.window_rows(t["frame"], t["detection_id"], start, step, "max" if fpg < 0 else fpg, None if maxd < 0 else maxd,
                                   None if end < 0 else end, bool(ensure))
        assert np.array_equal(t["detection_id"][rows], z[f"rows:{tag}:detection_id"]), tag


def test_draw_augmentation_reproduces_the_reference_draws(g25):
    z, params, tables, samples = g25
    kinds = set()
    for k, s in enumerate(samples):
        t = tables[s["seq"]]
        mode = "train" if s["train"] else "val"
        rng = np.random.RandomState(s["seed"])
        window = lambda step: dataset.window_rows(t["frame"], t["detection_id"], s["start"], step, params["frames_per_graph"], params["max_detects"])
        step, kept, eps = dataset.draw_augmentation(rng, lambda step: t["id"][window(step)], t["step_size"], params, mode)
        rows = window(step)[kept]
        assert step == s["step_size"] and np.array_equal(rows, s["rows"]), k
        if s["train"]:
            assert eps.dtype == np.float64 and np.array_equal(eps, s["eps"]), k
            kinds |= {"step"} if step != t["step_size"] else set()
            kinds |= {"untracked"} if set(t["id"][window(step)].tolist()) == {-1} else set()
        else:
            assert eps is None and kept.size == window(step).size
        assert rng.rand() == z[f"s{k}:next_rand"], k      # the stream was consumed as the reference consumed it
        # the two-call form gives the same
        rng = np.random.RandomState(s["seed"])
        step2 = dataset.draw_step_size(rng, t["step_size"], params, mode)
        _, kept2, eps2 = dataset.draw_augmentation(rng, t["id"][window(step2)], step2, params, mode, draw_step=False)
        assert step2 == step and np.array_equal(kept2, kept) and (eps2 is None) == (eps is None)
    assert kinds == {"step", "untracked"}


def test_numpy_restatement_matches_the_reference_samples(g25):
    z, params, tables, samples = g25
    pruned = 0
    for k, s in enumerate(samples):
        got = R.build_batch(tables, [(s["seq"], s["rows"], s["eps"])], params)
        want_boxes = np.stack([z[f"s{k}:{c}"] for c in R.BOX_COLUMNS], axis=1)
        assert got["boxes"].tobytes() == want_boxes.tobytes(), k                      # float64, bit for bit
        assert got["cols"].tobytes() == want_boxes[:, [R.H, R.W, R.FX, R.FY]].astype(np.float32).tobytes(), k
        assert np.array_equal(got["frame"], z[f"s{k}:frame"]) and np.array_equal(got["id"], z[f"s{k}:id"])
        assert np.array_equal(got["edge_index"], z[f"s{k}:edge_index"]), k
        assert np.array_equal(got["edge_labels"], z[f"s{k}:edge_labels"]), k
        assert np.allclose(got["edge_attr"], z[f"s{k}:edge_attr"], rtol=2e-6, atol=2e-6), k
        if s["train"]:
            assert got["min_iou"] == z[f"s{k}:min_iou"] >= params["min_iou_bb_wiggling"]
        pruned += R.batch_pairs(got["frame"], got["graph_ptr"], params["max_frame_dist"]).shape[1] * 2 > got["edge_index"].shape[1]
    assert pruned >= 4      # top_k_nns removes edges at this size


def test_numpy_batch_is_the_concatenation_of_its_graphs(g25):
    _, params, tables, samples = g25
    batch = [(s["seq"], s["rows"], s["eps"]) for s in samples[:R.N_TRAIN]]
    whole = R.build_batch(tables, batch, params)
    off_n, off_e = 0, 0
    for g, one in enumerate(batch):
        part = R.build_batch(tables, [one], params)
        n, e = len(part["frame"]), part["edge_index"].shape[1]
        assert np.array_equal(whole["edge_index"][:, off_e:off_e + e], part["edge_index"] + off_n)
        assert np.array_equal(whole["edge_attr"][off_e:off_e + e], part["edge_attr"])
        assert np.array_equal(whole["edge_labels"][off_e:off_e + e], part["edge_labels"])
        assert (whole["edge_graph"][off_e:off_e + e] == g).all() and (whole["node_graph"][off_n:off_n + n] == g).all()
        off_n, off_e = off_n + n, off_e + e
    assert off_e == whole["edge_index"].shape[1]


def test_train_batch_entry_points_argument_checks_without_gpu():
    """Everything below returns before a kernel is launched or a byte is copied (the non-null pointers are host dummies that are
    never dereferenced, except graph_ptr, which IS a host array)."""
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    big = 1 << 30
    gp = lambda *v: (ctypes.c_int32 * len(v))(*v)
    f = ctypes.c_float(1e-6)
    # ---- augment_boxes
    need = l.mpnhip_augment_boxes_workspace_bytes()
    assert need > 0
    aug = lambda ptr_host=gp(0, 2, 5), b=2, n=5, ws=p, nbytes=big, boxes=p, src=p, out=p, dev_ptr=p, miniou=p: l.mpnhip_augment_boxes(
        boxes, p, p, 9, src, ptr_host, b, None, n, out, p, p, p, p, dev_ptr, miniou, p, ws, nbytes, None)
    assert aug(ptr_host=None, b=0, n=0) == 0                                   # no graphs: a successful no-op
    assert aug(b=0, n=5) == -1 and b"augment_boxes" in l.mpnhip_last_error()  # nodes without a graph
    assert aug(n=-1) == -1 and aug(b=-1) == -1
    assert aug(ptr_host=None) == -1 and aug(dev_ptr=None) == -1
    for bad in (gp(0, 3, 2), gp(1, 2, 5), gp(0, 2, 4), gp(0, 6, 5), gp(0, -1, 5)):
        assert aug(ptr_host=bad) == -1, list(bad)
        assert b"graph_ptr" in l.mpnhip_last_error()
    assert aug(ptr_host=gp(0, 6, 5)) == -1 and b"not ascending" in l.mpnhip_last_error()
    assert aug(boxes=None) == -1 and aug(src=None) == -1 and aug(out=None) == -1 and aug(miniou=None) == -1
    assert aug(ws=None) == -3 and aug(nbytes=need - 1) == -3 and b"augment_boxes: workspace" in l.mpnhip_last_error()
    # ---- batch_pairs
    assert 0 < l.mpnhip_batch_pairs_workspace_bytes(10) < l.mpnhip_batch_pairs_workspace_bytes(100000)
    assert l.mpnhip_batch_pairs_workspace_bytes(-1) == 0
    need = l.mpnhip_batch_pairs_workspace_bytes(5)
    cnt = lambda n=5, b=2, fr=p, ng=p, dp=p, offs=p, ws=p, nbytes=big: l.mpnhip_batch_pairs_count(fr, ng, dp, b, n, 4, offs, ws, nbytes, None)
    fill = lambda n=5, b=2, npairs=7, fr=p, ng=p, dp=p, offs=p, out=p: l.mpnhip_batch_pairs_fill(fr, ng, dp, b, n, 4, offs, npairs, out, None)
    assert cnt(n=0, b=0, fr=None, ng=None, dp=None, offs=None, ws=None, nbytes=0) == 0 and fill(n=0, b=0, npairs=0, fr=None, out=None) == 0
    assert fill(npairs=0, out=None) == 0
    assert cnt(n=-1) == -1 and cnt(b=0) == -1 and b"batch_pairs" in l.mpnhip_last_error()
    assert cnt(fr=None) == -1 and cnt(ng=None) == -1 and cnt(dp=None) == -1 and cnt(offs=None) == -1
    assert cnt(ws=None) == -3 and cnt(nbytes=need - 1) == -3
    assert fill(npairs=-1) == -1 and fill(fr=None) == -1 and fill(out=None) == -1 and fill(offs=None) == -1 and fill(b=0) == -1
    # ---- batch_edge_features
    ef = lambda e=3, n=5, b=2, ei=p, fps=p, emb=p, ld=8, dim=8, out=p: l.mpnhip_batch_edge_features(ei, e, n, p, p, fps, b, p, emb, ld, dim, f,
                                                                                                      out, p, None)
    assert ef(e=0, n=0, b=0, ei=None, fps=None, emb=None, out=None) == 0
    assert ef(e=-1) == -1 and ef(n=0) == -1 and ef(b=0) == -1 and ef(ld=4) == -1 and b"batch_edge_features" in l.mpnhip_last_error()
    assert ef(ei=None) == -1 and ef(fps=None) == -1 and ef(emb=None) == -1 and ef(out=None) == -1
    # ---- batch_edge_layout
    need = l.mpnhip_batch_edge_layout_workspace_bytes(2)
    assert need > 0 and l.mpnhip_batch_edge_layout_workspace_bytes(-1) == 0
    cols = (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 5)
    lay = lambda npairs=7, k=4, n=5, b=2, pairs=p, kept=p, ac=cols, nc=6, ei=p, ea=p, ws=p, nbytes=big: l.mpnhip_batch_edge_layout(
        pairs, npairs, kept, k, p, n, b, p, p, ac, nc, ei, ea, p, ws, nbytes, None)
    assert lay(npairs=0, k=0, n=0, b=0, pairs=None, kept=None, ei=None, ea=None, ws=None, nbytes=0) == 0
    assert lay(k=0, ws=None) == 0
    assert lay(k=8) == -1 and b"batch_edge_layout" in l.mpnhip_last_error()          # more kept than pairs
    assert lay(k=-1) == -1 and lay(n=0) == -1 and lay(b=0) == -1 and lay(nc=7) == -1 and lay(nc=-1) == -1 and lay(ac=None) == -1
    assert lay(ac=(ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 6)) == -1 and lay(ac=(ctypes.c_int32 * 6)(-1, 1, 2, 3, 4, 5)) == -1
    assert lay(pairs=None) == -1 and lay(ei=None) == -1 and lay(ea=None) == -1
    assert lay(kept=None, ws=None) == -3                                                # (kept = NULL is "all": valid)
    assert lay(ws=None) == -3 and lay(nbytes=need - 1) == -3 and b"batch_edge_layout: workspace" in l.mpnhip_last_error()
