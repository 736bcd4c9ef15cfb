"""Training batches on the device (``mpntrackseg_amd/train_batch.py``, ``csrc/train_batch.hip``) against
(a) the reference's own samples (tests/golden/g25_train_samples.npz, tools/make_golden_train_batch.py): float64 boxes and their
    float32 casts bit for bit, integers exact, ``edge_attr`` within rtol = atol = 2e-6 (the bound of g14 in test_gpu_tracker.py:
    ``log`` and the division differ between libraries by an ulp, the embedding norm is summed in another order);
(b) the package's existing per-sample path -- ``graph.construct_graph(..., inference_mode=False)``, ``assign_edge_labels``,
    ``gather_rows`` -- concatenated with node offsets in PyG-``Batch`` order: bit for bit, for B = 1, 3 and 6;
(c) properties: the graph ids are consistent, the result does not depend on how the batch is cut, a bad ``eps`` row raises;
(d) one training step from ``TrainingBatches`` into ``TrainStep``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_ref as R  # noqa: E402
from mpntrackseg_amd import dataset, graph as G, synth, train_batch as TB  # noqa: E402
from mpntrackseg_amd.mpn import MOTMPNet  # noqa: E402
from mpntrackseg_amd.train import TrainStep  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def g25(golden):
    z = golden("g25_train_samples.npz")
    params, tables, samples = R.fixture(z)
    stores = []
    for i, t in enumerate(tables):
        n = len(t["frame"])
        det = dict(frame=t["frame"], id=t["id"], detection_id=t["detection_id"], **{c: t["boxes"][:, j] for j, c in enumerate(R.BOX_COLUMNS)})
        stores.append(TB.SequenceStore(det, t["fps"], t["step_size"], t["reid"], t["x"].reshape(n, 64, 1, 1),
                                       x_ext=synth.normal(70 + i, (n, 3, 2, 2)), mask_labels=(synth.uniform01(72 + i, n * 16) < 0.5).reshape(n, 1, 4, 4),
                                       mask_gt_ixs=synth.uniform01(74 + i, n) < 0.6, device=DEV))
    return z, params, tables, samples, stores


def _tuples(samples):
    return [(s["seq"], s["rows"], s["eps"]) for s in samples]


def _per_sample(store, rows, eps, params):
    """One graph through the functions the package had before: ``construct_graph(inference_mode=False)``, ``assign_edge_labels``,
    ``gather_rows``; the wiggled float32 columns are numpy's (bit-exact float64 arithmetic, tests/train_batch_ref.py)."""
    dev = store.device
    ids = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
    _, cols, _ = R.augment_boxes(store.boxes.cpu().numpy(), rows, eps)
    det = dict(frame=store.frame[rows], bb_height=cols[:, 0], bb_width=cols[:, 1], feet_x=cols[:, 2], feet_y=cols[:, 3])
    emb = G.gather_rows(store.reid, ids)
    g = G.construct_graph(det, emb, store.fps, params["max_frame_dist"], params["edge_feats_to_use"], top_k_nns=params["top_k_nns"],
                          reciprocal_k_nns=params["reciprocal_k_nns"], inference_mode=False)
    labels = G.assign_edge_labels(g["edge_index"], store.id[rows], params["true_edge_labels"])
    gather = lambda t: G.gather_rows(t, ids).view((len(rows),) + tuple(t.shape[1:]))
    return dict(edge_index=g["edge_index"], edge_attr=g["edge_attr"], edge_labels=labels, x=gather(store.x), x_ext=gather(store.x_ext),
                mask_labels=gather(store.mask_labels), mask_gt_ixs=gather(store.mask_gt_ixs) != 0)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _assert_is_concatenation(batch, parts):
    off_n, off_e = 0, 0
    ptr = batch["graph_ptr"].cpu().numpy()
    for g, part in enumerate(parts):
        n, e = part["x"].shape[0], part["edge_index"].shape[1]
        assert ptr[g] == off_n and ptr[g + 1] == off_n + n
        assert _same_bits(batch["edge_index"][:, off_e:off_e + e], part["edge_index"] + off_n), g
        for k in ("edge_attr", "edge_labels"):
            assert _same_bits(batch[k][off_e:off_e + e], part[k]), (g, k)
        for k in ("x", "x_ext", "mask_labels", "mask_gt_ixs"):
            assert _same_bits(batch[k][off_n:off_n + n], part[k]), (g, k)
        assert (batch["edge_graph"][off_e:off_e + e] == g).all() and (batch["node_graph"][off_n:off_n + n] == g).all()
        off_n, off_e = off_n + n, off_e + e
    assert off_e == batch["edge_index"].shape[1] and off_n == batch["x"].shape[0]


def test_augment_boxes_matches_the_reference_bits(g25):
    z, params, tables, samples, stores = g25
    train = samples[:R.N_TRAIN]
    ss = TB.StoreSet(stores)
    node_src = np.concatenate([s["rows"] + ss.offsets[s["seq"]] for s in train])
    ptr = np.concatenate(([0], np.cumsum([len(s["rows"]) for s in train])))
    eps = np.concatenate([s["eps"] for s in train])
    out = TB.augment_boxes(ss, node_src, ptr, eps)
    want = np.concatenate([np.stack([z[f"s{k}:{c}"] for c in R.BOX_COLUMNS], axis=1) for k in range(R.N_TRAIN)])
    assert out["boxes"].cpu().numpy().tobytes() == want.tobytes()
    assert out["cols"].cpu().numpy().tobytes() == want[:, [R.H, R.W, R.FX, R.FY]].astype(np.float32).tobytes()
    assert np.array_equal(out["frame"].cpu().numpy(), np.concatenate([z[f"s{k}:frame"] for k in range(R.N_TRAIN)]))
    assert np.array_equal(out["id"].cpu().numpy(), np.concatenate([z[f"s{k}:id"] for k in range(R.N_TRAIN)]))
    assert np.array_equal(out["node_graph"].cpu().numpy(), np.repeat(np.arange(R.N_TRAIN), np.diff(ptr)))
    assert np.array_equal(out["graph_ptr"].cpu().numpy(), ptr) and int(out["bad_rows"].item()) == 0
    all_boxes = np.concatenate([t["boxes"] for t in tables])
    assert float(out["min_iou"].item()) == R.iou_pairs(want[:, :4], all_boxes[node_src][:, :4]).min() == min(z[f"s{k}:min_iou"] for k in range(R.N_TRAIN))
    # without eps: the rows as they are, no minimum
    plain = TB.augment_boxes(ss, node_src, ptr, None)
    assert plain["boxes"].cpu().numpy().tobytes() == all_boxes[node_src].tobytes() and float(plain["min_iou"].item()) == np.inf
    # a NaN shift gives numpy's NaN minimum; more than one block of nodes
    many = np.tile(node_src, 12)
    eps_many = np.tile(eps, (12, 1))
    eps_many[300, 1] = np.nan
    got = TB.augment_boxes(ss, many, np.array([0, 7, 7, many.size]), eps_many)
    assert many.size > 512 and np.isnan(float(got["min_iou"].item()))
    eps_many[300, 1] = 0.2
    got = TB.augment_boxes(ss, many, np.array([0, 7, 7, many.size]), eps_many)
    assert float(got["min_iou"].item()) == R.augment_boxes(all_boxes, many, eps_many)[2] < params["min_iou_bb_wiggling"]
    assert np.array_equal(got["node_graph"].cpu().numpy(), np.repeat([0, 1, 2], [7, 0, many.size - 7]))


def test_build_batch_refuses_a_shift_past_the_bound(g25):
    _, params, _, samples, stores = g25
    batch = _tuples(samples[:3])
    eps = batch[1][2].copy()
    # one row of one graph, scaled to eight times the bound of augmentation.py:62-65 (one side moved by 0.31 of the box: IoU < 0.8)
    eps[2] = np.where(eps[2] < 0, -8.0, 8.0) * dataset.wiggle_max_eps(params["min_iou_bb_wiggling"])
    batch[1] = (batch[1][0], batch[1][1], eps)
    with pytest.raises(AssertionError, match="min_iou_bb_wiggling"):
        TB.build_batch(stores, batch, params)
    TB.build_batch(stores, _tuples(samples[:3]), params)   # the unscaled batch passes; nothing faulted in between


@pytest.mark.parametrize("b", [1, 3, 6])
def test_build_batch_is_the_concatenation_of_the_per_sample_path(g25, b):
    _, params, tables, samples, stores = g25
    # B = 6: an augmented graph of each sequence (different fps), a window of one populated frame (no edges), a graph without
    # nodes (built by hand: the fixture's draws keep at least five detections), and two more samples
    one_frame = dataset.window_rows(tables[0]["frame"], tables[0]["detection_id"], 39, 3, params["frames_per_graph"], params["max_detects"])
    assert len(np.unique(tables[0]["frame"][one_frame])) == 1 and one_frame.size > 1
    tr = _tuples(samples)
    picks = {1: [tr[0]], 3: [tr[4], (0, one_frame, np.zeros((one_frame.size, 4))), tr[1]],
             6: [tr[0], (0, one_frame, np.zeros((one_frame.size, 4))), tr[4], (1, np.zeros(0, np.int64), np.zeros((0, 4))), tr[2], tr[5]]}[b]
    assert b < 3 or {stores[p[0]].fps for p in picks} == {20.0, 6.0}
    batch = TB.build_batch(stores, picks, params)
    parts = [_per_sample(stores[si], rows, eps, params) for si, rows, eps in picks]
    assert b < 3 or parts[1]["edge_index"].shape[1] == 0
    _assert_is_concatenation(batch, parts)
    assert batch["n_graphs"] == b and batch["edge_graph"].dtype == torch.int32 and batch["mask_gt_ixs"].dtype == torch.bool


def test_build_batch_matches_the_reference_samples(g25):
    z, params, _, samples, stores = g25
    for group in (range(R.N_TRAIN), range(R.N_TRAIN, R.N_SAMPLES)):      # the augmented samples as one batch, then the 'val' pair
        batch = TB.build_batch(stores, _tuples([samples[k] for k in group]), params)
        ei, ea, lab = batch["edge_index"].cpu().numpy(), batch["edge_attr"].cpu().numpy(), batch["edge_labels"].cpu().numpy()
        ptr = batch["graph_ptr"].cpu().numpy()
        boxes = batch["boxes"].cpu().numpy()
        off_e = 0
        for g, k in enumerate(group):
            e = z[f"s{k}:edge_index"].shape[1]
            assert np.array_equal(ei[:, off_e:off_e + e], z[f"s{k}:edge_index"] + ptr[g]), k
            assert np.array_equal(lab[off_e:off_e + e], z[f"s{k}:edge_labels"]), k
            assert np.allclose(ea[off_e:off_e + e], z[f"s{k}:edge_attr"], rtol=2e-6, atol=2e-6), k
            want = np.stack([z[f"s{k}:{c}"] for c in R.BOX_COLUMNS], axis=1)
            assert boxes[ptr[g]:ptr[g + 1]].tobytes() == want.tobytes(), k
            off_e += e
        assert off_e == ei.shape[1]


def test_graph_ids_are_consistent(g25):
    _, params, _, samples, stores = g25
    batch = TB.build_batch(stores, _tuples(samples[:R.N_TRAIN]), params)
    ptr = batch["graph_ptr"].cpu().numpy().astype(np.int64)
    ei, eg, ng = batch["edge_index"].cpu().numpy(), batch["edge_graph"].cpu().numpy(), batch["node_graph"].cpu().numpy()
    assert np.array_equal(ng, np.repeat(np.arange(R.N_TRAIN), np.diff(ptr))) and (np.diff(eg) >= 0).all()
    for side in ei:
        assert (side >= ptr[eg]).all() and (side < ptr[eg + 1]).all()
    e = ei.shape[1]
    for g in range(R.N_TRAIN):      # inside a graph: the pairs (row < col), then the same pairs flipped
        sel = np.nonzero(eg == g)[0]
        half = sel.size // 2
        fwd, bwd = ei[:, sel[:half]], ei[:, sel[half:]]
        assert sel.size % 2 == 0 and (fwd[0] < fwd[1]).all() and np.array_equal(fwd[::-1], bwd)
    assert e == eg.size


def test_result_does_not_depend_on_how_the_batch_is_cut(g25):
    _, params, _, samples, stores = g25
    tr = _tuples(samples[:R.N_TRAIN])
    whole = TB.build_batch(stores, tr, params)
    halves = [TB.build_batch(stores, tr[:3], params), TB.build_batch(stores, tr[3:], params)]
    parts = []
    for h in halves:
        ptr, eg = h["graph_ptr"].cpu().numpy(), h["edge_graph"].cpu().numpy()
        for g in range(3):
            es = np.nonzero(eg == g)[0]
            e0, e1 = (es[0], es[-1] + 1) if es.size else (0, 0)
            part = {k: h[k][e0:e1] for k in ("edge_attr", "edge_labels")}
            part["edge_index"] = h["edge_index"][:, e0:e1] - int(ptr[g])
            part.update({k: h[k][ptr[g]:ptr[g + 1]] for k in ("x", "x_ext", "mask_labels", "mask_gt_ixs")})
            parts.append(part)
    _assert_is_concatenation(whole, parts)


def test_training_batches_feed_a_training_step(g25):
    _, params, tables, _, stores = g25
    tb = TB.TrainingBatches(stores, params, batch_size=3, mode="train", rng=np.random.RandomState(5), shuffle=True)
    n_ref = sum(dataset.index_dataset(t["frame"], t["step_size"], params["frames_per_graph"], params["min_detects"]).size for t in tables)
    assert tb.n_samples == n_ref > 20 and len(tb) == -(-n_ref // 3)
    one = tb[4]
    assert one["n_graphs"] == 1 and one["edge_index"].shape[1] > 0
    mp = synth.model_params(32, 4, "sum", num_class_steps=2, node_in_dim=64, edge_in_dim=6)
    W = synth.make_weights(mp, seed=7, gain=0.5)
    model = MOTMPNet(mp)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
    model = model.to(DEV).train()
    step = TrainStep(model)
    before = step.bucket.flat_params.clone()
    batch = next(iter(tb))
    assert batch["n_graphs"] == 3 and batch["edge_index"].shape[1] > 0
    step(batch["x"].view(batch["x"].shape[0], -1), batch["edge_index"], batch["edge_attr"], labels=batch["edge_labels"],
         edge_graph=batch["edge_graph"], n_graphs=batch["n_graphs"])
    torch.cuda.synchronize()
    loss = torch.as_tensor(step.last_loss).float()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(step.bucket.flat_params).all())
    assert not torch.equal(before, step.bucket.flat_params)     # the optimizer moved the parameters
