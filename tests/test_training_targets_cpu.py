"""Training targets without a GPU: the numpy restatement of tests/training_targets_ref.py against what the REFERENCE functions
themselves produced (tests/golden/g21_training_targets.npz: MOTGraph.assign_edge_labels and MOTNeuralSolver._compute_loss with
autograd), and the host-side argument checks of the four C-ABI entries of csrc/train_targets.hip."""
import ctypes

import numpy as np
import pytest
import torch

import training_targets_ref as R
from mpntrackseg_amd import capi, graph, loss
from oracle import loss_oracle as LO

F1 = ctypes.c_float(1.0)


@pytest.fixture(scope="module")
def z(golden):
    return golden("g21_training_targets.npz")


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("tag", R.LABEL_CASES)
def test_restated_labels_equal_the_reference(z, tag, mode):
    want = z[f"lab:{tag}:{mode}"]
    got = R.edge_labels(z[f"lab:{tag}:edge_index"], z[f"lab:{tag}:ids"], mode)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_label_cases_cover_what_they_are_for(z):
    ei, ids = z["lab:base:edge_index"], z["lab:base:ids"]
    assert ei.shape == (2, 400) and ids.shape == (48,) and (ids == -1).any()
    assert 0 < z["lab:base:closest"].sum() < z["lab:base:all"].sum()
    # the stored duplicates of active edges are all active; self loops on real ids: 'all' only
    assert z["lab:dups:edge_index"].shape == (2, 410)
    assert z["lab:dups:closest"][400:403].tolist() == [1, 1, 1] and z["lab:dups:closest"][403:406].tolist() == [0, 0, 0]
    assert z["lab:dups:all"][406:].tolist() == [1] * 4 and z["lab:dups:closest"][406:].tolist() == [0] * 4
    assert z["lab:unique:all"].sum() == 0 and z["lab:one:closest"].tolist() == [1] and z["lab:none:all"].shape == (0,)
    assert z["lab:big:edge_index"].shape == (2, 3000)
    with pytest.raises(IndexError):
        R.edge_labels(np.array([[0], [2]]), np.array([1, 1]), "closest")


def check_loss_case(z, tag, logits, labels, preds, mlab, valid, node_graph=None, edge_graph=None, n_graphs=1):
    w = R.LOSS_WEIGHTS
    lv, grads = R.mask_loss(list(preds), mlab, valid, w["segmentation"], node_graph, n_graphs)
    # tracking term: the oracle's restatement (pinned to the reference by g9 / g16), per graph where there are several
    lg = torch.from_numpy(logits).double().requires_grad_(True)
    track = 0
    for g in range(n_graphs):
        sel = torch.from_numpy(np.ones(logits.shape[1], bool) if edge_graph is None else edge_graph == g)
        track = track + LO.tracking_loss([lg[s][sel].view(-1, 1) for s in range(logits.shape[0])], torch.from_numpy(labels).double()[sel],
                                         weight=w["tracking"]) / n_graphs
    track.backward()
    ref = float(z[f"{tag}:loss"])
    assert abs(float(track.detach()) + lv[0] - ref) <= 1e-6 * abs(ref)
    assert np.abs(lg.grad.numpy() - z[f"{tag}:glogits"]).max() <= 1e-6 * np.abs(z[f"{tag}:glogits"]).max()
    rows = R.sample_rows(valid)
    for s, g in enumerate(grads):
        want = z[f"{tag}:gmask_rows"][s]
        scale = max(float(np.abs(want).max()), 1e-30)
        assert np.abs(g[rows] - want).max() <= 1e-6 * scale
        assert abs(np.sqrt((g ** 2).sum()) - z[f"{tag}:gmask_norm"][s]) <= 1e-6 * max(float(z[f"{tag}:gmask_norm"][s]), 1e-30)
        rs = np.abs(g).reshape(g.shape[0], -1).sum(axis=1)
        assert np.abs(rs - z[f"{tag}:gmask_row_abssum"][s]).max() <= 1e-6 * max(float(z[f"{tag}:gmask_row_abssum"][s].max()), 1e-30)
        assert not g[~np.asarray(valid, bool)].any() and not z[f"{tag}:gmask_row_abssum"][s][~np.asarray(valid, bool)].any()


@pytest.mark.parametrize("tag", sorted(R.LOSS_CASES))
def test_restated_loss_matches_the_reference(z, tag):
    check_loss_case(z, tag, *R.loss_inputs(tag))


def test_restated_graph_batched_loss_matches_the_reference(z):
    logits, labels, preds, mlab, valid, node_graph, edge_graph = R.graph_inputs()
    assert [int(valid[node_graph == g].sum()) for g in range(3)] == list(R.GRAPH_CASE["valid"])
    check_loss_case(z, "graphs", logits, labels, preds, mlab, valid, node_graph, edge_graph, 3)


def test_loss_inputs_are_the_cases_the_fixture_names():
    for tag, (n, k, hw, nv, _) in R.LOSS_CASES.items():
        logits, labels, preds, mlab, valid = R.loss_inputs(tag)
        assert preds.shape == (k, n, 1) + hw and mlab.shape == (n, 1) + hw and int(valid.sum()) == nv and logits.shape[0] == k
    assert float(np.abs(R.loss_inputs("extreme")[2]).max()) >= 80.0
    m = R.loss_inputs("scalar")[3]
    assert ((m > 0) & (m < 1)).all()   # non-binary labels


def test_edge_labels_argument_checks_without_gpu():
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    assert l.mpnhip_edge_labels_workspace_bytes(1000) >= 8000 > l.mpnhip_edge_labels_workspace_bytes(10) > 0
    # no edges: a successful no-op whatever else is null
    for mode in (0, 1):
        assert l.mpnhip_edge_labels(None, 0, None, 0, mode, None, None, None, 0, None) == 0
        assert l.mpnhip_edge_labels(None, 0, None, 48, mode, None, None, None, 0, None) == 0
    # refused before any launch: unknown mode, negative sizes, null tensors, an undersized workspace
    assert l.mpnhip_edge_labels(p, 5, p, 3, 2, p, p, p, 256, None) == -1
    assert b"edge_labels: unknown mode 2" in l.mpnhip_last_error()
    assert l.mpnhip_edge_labels(p, -1, p, 3, 0, p, p, p, 256, None) == -1
    assert b"edge_labels: bad sizes" in l.mpnhip_last_error()
    assert l.mpnhip_edge_labels(p, 5, p, 2 ** 31, 0, p, p, p, 256, None) == -1
    for args in ((None, 5, p, 3, 1, p, p), (p, 5, None, 3, 1, p, p), (p, 5, p, 3, 1, None, p), (p, 5, p, 3, 1, p, None)):
        assert l.mpnhip_edge_labels(*args, p, 256, None) == -1
        assert b"edge_labels: null" in l.mpnhip_last_error()
    assert l.mpnhip_edge_labels(p, 5, p, 3, 1, p, p, None, 0, None) == -3
    assert l.mpnhip_edge_labels(p, 5, p, 1000, 1, p, p, p, 256, None) == -3
    assert b"edge_labels: workspace 256 <" in l.mpnhip_last_error()


def test_mask_loss_argument_checks_without_gpu():
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    ptrs = (ctypes.c_void_p * 16)(*[p.value] * 16)
    many = (ctypes.c_void_p * 17)(*[p.value] * 17)
    assert l.mpnhip_mask_loss_workspace_bytes(3, 500, 3136, 1) > l.mpnhip_mask_loss_workspace_bytes(1, 500, 3136, 1) > 0
    assert l.mpnhip_mask_loss_workspace_bytes(1, 500, 3136, 8) >= l.mpnhip_mask_loss_workspace_bytes(1, 500, 3136, 1)
    # nothing to do: no steps, no rows or empty rows (no loss_out: nothing is touched)
    assert l.mpnhip_mask_loss(None, 0, None, None, None, 1, 40, 3136, F1, None, None, None, 0, None) == 0
    assert l.mpnhip_mask_loss(None, 2, None, None, None, 1, 0, 3136, F1, None, None, None, 0, None) == 0
    assert l.mpnhip_mask_loss(None, 2, None, None, None, 1, 40, 0, F1, None, None, None, 0, None) == 0
    # refusals
    assert l.mpnhip_mask_loss(many, 17, p, p, None, 1, 4, 16, F1, p, many, p, 256, None) == -1
    assert b"mask_loss: 17 steps in one call (at most 16" in l.mpnhip_last_error()
    assert l.mpnhip_mask_loss(ptrs, -1, p, p, None, 1, 4, 16, F1, p, ptrs, p, 256, None) == -1
    assert b"mask_loss: bad sizes" in l.mpnhip_last_error()
    for ng in (0, 1025):
        assert l.mpnhip_mask_loss(ptrs, 2, p, p, p, ng, 4, 16, F1, p, ptrs, p, 256, None) == -1
        assert b"graphs" in l.mpnhip_last_error()
    assert l.mpnhip_mask_loss(ptrs, 2, p, p, None, 3, 4, 16, F1, p, ptrs, p, 256, None) == -1
    assert b"without node_graph" in l.mpnhip_last_error()
    for args in ((None, 2, p, p, None, 1, 4, 16, F1, p, ptrs), (ptrs, 2, None, p, None, 1, 4, 16, F1, p, ptrs),
                 (ptrs, 2, p, None, None, 1, 4, 16, F1, p, ptrs), (ptrs, 2, p, p, None, 1, 4, 16, F1, None, ptrs),
                 (ptrs, 2, p, p, None, 1, 4, 16, F1, p, None)):
        assert l.mpnhip_mask_loss(*args, p, 1 << 20, None) == -1
        assert b"mask_loss: null tensor" in l.mpnhip_last_error()
    holes = (ctypes.c_void_p * 2)(p.value, None)
    assert l.mpnhip_mask_loss(holes, 2, p, p, None, 1, 4, 16, F1, p, ptrs, p, 1 << 20, None) == -1
    assert b"null tensor of step 1" in l.mpnhip_last_error()
    assert l.mpnhip_mask_loss(ptrs, 2, p, p, None, 1, 4, 16, F1, p, ptrs, None, 0, None) == -3
    assert l.mpnhip_mask_loss(ptrs, 2, p, p, None, 1, 4000, 3136, F1, p, ptrs, p, 256, None) == -3
    assert b"mask_loss: workspace 256 <" in l.mpnhip_last_error()


def test_host_mirrors_refuse_cpu_tensors():
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        graph.assign_edge_labels(ei, torch.tensor([3, 3]))
    with pytest.raises(capi.MpnhipError, match="unknown mode"):
        graph.assign_edge_labels(ei, torch.tensor([3, 3]), mode="nearest")
    m = torch.zeros(2, 1, 3, 5)
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        loss.mask_loss_and_grad([m], m, torch.ones(2, dtype=torch.bool), 1.5)
    batch = type("B", (), dict(edge_labels=torch.zeros(2), mask_labels=m, mask_gt_ixs=torch.ones(2, dtype=torch.bool)))()
    with pytest.raises(capi.MpnhipError, match="HIP device only"):
        loss.compute_loss({"classified_edges": [torch.zeros(2, 1)], "mask_predictions": [m]}, batch, R.LOSS_WEIGHTS)
    with pytest.raises(capi.MpnhipError, match="need edge_graph"):
        loss.compute_loss({"classified_edges": [torch.zeros(2, 1)], "mask_predictions": [m]}, batch, R.LOSS_WEIGHTS, n_graphs=2)
    with pytest.raises(capi.MpnhipError, match="need edge_graph"):
        loss.compute_loss({"classified_edges": [torch.zeros(2, 1)], "mask_predictions": [m]}, batch, R.LOSS_WEIGHTS,
                          edge_graph=torch.zeros(2, dtype=torch.int32), n_graphs=2)
