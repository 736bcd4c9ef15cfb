"""The tail of the sliding-window inference without a device: the argument checks and size queries of its C-ABI entry points, and
the consistency of tests/golden/g17_window_tail.npz (the reference's MPNTracker._evaluate_graph_in_batches run to its end) with an
independent numpy restatement of the undirected merge and the pruning -- ``np_merge`` / ``np_prune`` below, which
tests/test_gpu_tracker_tail.py uses as the expectation for random inputs."""
import ctypes

import numpy as np
import pytest

from mpntrackseg_amd import capi, synth

MPNHIP_ERR_WORKSPACE = -3   # include/mpnhip.h

SEQ_CASES = ["s1", "s2", "l1", "l2"]


def np_merge(edge_index, attrs=()):
    """One entry per unordered pair {r, c}: ``(edge_index_u [2, U] with row < col in lexicographic order, [mean of attr over the
    pair's directed copies ...], inverse [E])``.  Sums run over the copies in ascending edge id in float32 (np.add.at is
    unbuffered and walks its indices in order), then one float32 division by the number of copies."""
    ei = np.asarray(edge_index, dtype=np.int64)
    keys = (np.minimum(ei[0], ei[1]).astype(np.uint64) << np.uint64(32)) | np.maximum(ei[0], ei[1]).astype(np.uint64)
    uniq, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    ei_u = np.stack((uniq >> np.uint64(32), uniq & np.uint64(0xFFFFFFFF))).astype(np.int64)
    means = []
    for a in attrs:
        s = np.zeros(uniq.size, np.float32)
        np.add.at(s, inverse, np.asarray(a, np.float32))
        means.append(s / counts.astype(np.float32))
    return ei_u, means, inverse.reshape(-1).astype(np.int64)


def np_prune(edge_index, preds, threshold=0.5):
    with np.errstate(invalid="ignore"):
        keep = np.asarray(preds) >= np.float32(threshold)
    return np.asarray(edge_index)[:, keep], np.asarray(preds)[keep], np.nonzero(keep)[0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_tail_entry_points_argument_checks_without_gpu():
    """Size queries and argument checks of the new entry points run on the host: empty inputs are successful no-ops, null pointers
    and bad sizes are refused with the function's name in mpnhip_last_error(), a short workspace is MPNHIP_ERR_WORKSPACE."""
    l = capi.load()
    one = ctypes.c_void_p(256)   # a non-null address that no call below may reach a launch with
    f = ctypes.c_float
    # undirected merge
    assert l.mpnhip_undirected_merge_workspace_bytes(0) == 0
    small, big = l.mpnhip_undirected_merge_workspace_bytes(1000), l.mpnhip_undirected_merge_workspace_bytes(100000)
    assert 0 < small < big and small >= 1000 * (8 + 4 + 4)
    assert l.mpnhip_undirected_merge_sort(None, 0, 0, None, None, None, 0, None) != 0       # the count is always written
    assert b"undirected_merge_sort" in l.mpnhip_last_error()
    assert l.mpnhip_undirected_merge_sort(None, 10, 0, None, one, None, 0, None) != 0
    assert b"undirected_merge_sort" in l.mpnhip_last_error()
    assert l.mpnhip_undirected_merge_sort(one, -1, 0, one, one, one, 1 << 20, None) != 0
    assert l.mpnhip_undirected_merge_sort(one, 10, 0, one, one, one, 16, None) == MPNHIP_ERR_WORKSPACE
    assert b"undirected_merge_sort" in l.mpnhip_last_error()
    assert l.mpnhip_undirected_merge_fill(0, 0, None, 0, None, None, None, None) == 0
    assert l.mpnhip_undirected_merge_fill(10, 0, None, 0, None, None, None, None) == 0
    assert l.mpnhip_undirected_merge_fill(10, 11, one, 1 << 20, one, None, None, None) != 0   # more pairs than edges
    assert b"undirected_merge_fill" in l.mpnhip_last_error()
    assert l.mpnhip_undirected_merge_fill(10, 5, one, 1 << 20, one, one, None, None) != 0     # attr without attr_u
    assert l.mpnhip_undirected_merge_fill(10, 5, one, 16, one, None, None, None) == MPNHIP_ERR_WORKSPACE
    assert l.mpnhip_undirected_merge_fill(10, 5, None, 0, one, None, None, None) == MPNHIP_ERR_WORKSPACE
    # threshold
    assert l.mpnhip_threshold_flags(None, 0, f(0.5), None, None) == 0
    assert l.mpnhip_threshold_flags(None, 4, f(0.5), None, None) != 0
    assert b"threshold_flags" in l.mpnhip_last_error()
    assert l.mpnhip_threshold_flags(one, -1, f(0.5), one, None) != 0
    # node masks
    assert l.mpnhip_node_mask_accumulate(None, 0, 3136, 0, 10, None, None, None) == 0
    assert l.mpnhip_node_mask_accumulate(None, 3, 3136, 0, 10, None, None, None) != 0
    assert b"node_mask_accumulate" in l.mpnhip_last_error()
    assert l.mpnhip_node_mask_accumulate(one, 3, 3136, 8, 10, one, one, None) != 0            # rows 8..10 of 10 nodes
    assert b"node_mask_accumulate" in l.mpnhip_last_error()
    assert l.mpnhip_node_mask_accumulate(one, 3, 3136, -1, 10, one, one, None) != 0
    assert l.mpnhip_node_mask_accumulate(one, 3, -1, 0, 10, one, one, None) != 0
    assert l.mpnhip_node_mask_average(None, None, 0, 3136, None, None) == 0
    assert l.mpnhip_node_mask_average(None, None, 5, 0, None, None) == 0
    assert l.mpnhip_node_mask_average(None, None, 5, 3136, None, None) != 0
    assert b"node_mask_average" in l.mpnhip_last_error()
    # directed time-valid pairs: the workspace query is the undirected one's
    assert l.mpnhip_time_valid_conn_directed_count(None, 0, -1, None, None, 0, None) != 0     # the offsets are always written
    assert b"time_valid_conn" in l.mpnhip_last_error()
    assert l.mpnhip_time_valid_conn_directed_count(None, 5, -1, one, None, 0, None) != 0
    assert l.mpnhip_time_valid_conn_directed_count(one, 5, -1, one, one, 8, None) == MPNHIP_ERR_WORKSPACE
    assert l.mpnhip_time_valid_conn_directed_fill(None, 0, -1, None, 0, None, None) == 0
    assert l.mpnhip_time_valid_conn_directed_fill(None, 5, -1, None, 0, None, None) == 0
    assert l.mpnhip_time_valid_conn_directed_fill(None, 5, -1, None, 7, None, None) != 0
    assert b"time_valid_conn" in l.mpnhip_last_error()


def test_restatement_on_a_hand_made_list():
    ei = np.array([[3, 0, 1, 0, 1, 3], [1, 1, 0, 3, 3, 0]])   # pairs {1,3} {0,1} {0,1} {0,3} {1,3} {0,3}
    a = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0], np.float32)
    ei_u, (m,), inv = np_merge(ei, [a])
    assert ei_u.tolist() == [[0, 0, 1], [1, 3, 3]]
    assert m.tolist() == [3.0, 20.0, 8.5] and inv.tolist() == [2, 0, 0, 1, 2, 1]
    ek, pk, ids = np_prune(ei_u, np.array([0.5, np.nan, 0.49999997], np.float32))
    assert ek.tolist() == [[0], [1]] and pk.tolist() == [0.5] and ids.tolist() == [0]


@pytest.mark.parametrize("tag", SEQ_CASES)
def test_fixture_is_consistent_with_the_restatement(golden, tag):
    """Merging the fixture's directed scores reproduces its undirected list bit for bit, and pruning that at 0.5 its survivors."""
    z = golden("g17_window_tail.npz")
    ei = z[f"{tag[0]}:edge_index"]
    final = z[f"{tag}:final_edge_preds"]
    assert final.dtype == np.float32 and final.shape == (ei.shape[1],)
    ei_u, (pu,), inv = np_merge(ei, [final])
    assert ei.shape[1] == 2 * ei_u.shape[1]
    assert np.array_equal(ei_u, z[f"{tag}:edge_index_u"])
    assert same_bits(pu, z[f"{tag}:edge_preds_u"])
    assert np.array_equal(inv, z[f"{tag}:orig_indices"])
    ek, pk, _ = np_prune(ei_u, pu)
    assert np.array_equal(ek, z[f"{tag}:edge_index"]) and same_bits(pk, z[f"{tag}:edge_preds"])
    assert 0 < ek.shape[1] < ei_u.shape[1]   # the pruning is not vacuous
    # the rule of the end-to-end test: pairs this close to the threshold may flip; at most 1 % of a case's pairs are
    assert int((np.abs(z[f"{tag}:edge_preds_u"] - 0.5) <= 2e-5).sum()) <= 0.01 * ei_u.shape[1]


def test_fixture_sequences_and_masks(golden):
    z = golden("g17_window_tail.npz")
    for sq in ("s", "l"):
        frames, lo, hi, seed = [int(v) for v in z[f"{sq}:seq"]]
        det = synth.make_detections(frames=frames, dets_lo=lo, dets_hi=hi, seed=seed, emb_dim=32, node_in_dim=64, frame_stride=2)
        assert np.array_equal(det["frame"], z[f"{sq}:frame"]) and np.array_equal(det["x"], z[f"{sq}:x"])
    n = z["l:frame"].shape[0]
    assert (n, z["l:edge_index"].shape[1]) == (104, 10088)
    g10 = golden("g10_windows.npz")
    assert np.array_equal(g10["w1:edge_index"], z["s:edge_index"]) and same_bits(g10["w1:edge_attr"], z["s:edge_attr"])
    for tag in ("s1", "s2"):
        assert same_bits(g10[f"w{tag[1]}:final_edge_preds"], z[f"{tag}:final_edge_preds"])
        m = golden("g17_window_tail_masks.npz")[f"{tag}:node_preds"]
        assert m.shape == (z["s:frame"].shape[0], 1, 56, 56) and not np.isnan(m).any()
        assert 0.0 < m.min() and m.max() < 1.0
    for tag in ("l1", "l2"):
        assert z[f"{tag}:node_preds_head"].shape == (16, 1, 56, 56) and z[f"{tag}:node_preds_sum"].shape == (n,)
        assert np.allclose(z[f"{tag}:node_preds_head"].astype(np.float64).sum(axis=(1, 2, 3)), z[f"{tag}:node_preds_sum"][:16], rtol=0, atol=0)
    for tag in SEQ_CASES:
        assert 0.0 < float(z[f"{tag}:max_abs_mask_logit"]) < 50.0


def test_fixture_directed_pairs_match_the_dense_formulation(golden):
    z = golden("g17_window_tail.npz")
    f = z["l:frame"].astype(np.int64)
    for name in ("tv_max", "tv_3"):
        mfd = int(z[f"{name}:max_frame_dist"])
        d = np.abs(f[:, None] - f[None, :])
        cond = (d > 0) if mfd < 0 else ((d > 0) & (d <= mfd))
        row, col = np.nonzero(cond)
        assert np.array_equal(row, z[f"{name}:row"]) and np.array_equal(col, z[f"{name}:col"])
        assert row.size > 0
