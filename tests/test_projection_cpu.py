"""From edge scores to track ids, without a device: the numpy restatement of tests/projection_ref.py against the reference's own
outputs (tests/golden/g19_projection.npz: GreedyProjector.project, MPNTracker._assign_ped_ids, Postprocessor.drop_short_trajectories;
tools/make_golden.py gen_g19), the argument checks of the new C-ABI entry points, and the default LP solver of ``ExactProjector``."""
import ctypes

import numpy as np
import pytest

from mpntrackseg_amd import capi
from projection_ref import component_graphs, np_flows, np_greedy, np_keep, np_labels, np_rate, np_violated
from test_tracker_tail_cpu import same_bits

MPNHIP_ERR_WORKSPACE = -3   # include/mpnhip.h

SYNTHETIC = ["a", "b", "t", "hub"]
G19_CASES = SYNTHETIC + ["g17_s1", "g17_s2", "g17_l1", "g17_l2"]


def g19_case(z, tag):
    return z[f"{tag}:edge_index"], z[f"{tag}:edge_preds"], int(z[f"{tag}:num_nodes"])


def test_fixture_lists_the_cases(golden):
    z = golden("g19_projection.npz")
    assert [str(c) for c in z["cases"]] == G19_CASES
    for tag in G19_CASES:
        ei, p, n = g19_case(z, tag)
        assert ei.dtype == np.int64 and p.dtype == np.float32 and ei.shape == (2, p.size)
        assert (ei[0] < ei[1]).all() and 0 <= ei.min() and ei.max() < n


@pytest.mark.parametrize("tag", G19_CASES)
def test_restatement_reproduces_the_reference(golden, tag):
    z = golden("g19_projection.npz")
    ei, p, n = g19_case(z, tag)
    rp, rate, info = np_greedy(ei, p, n)
    assert same_bits(rp, z[f"{tag}:round_preds"])
    assert z[f"{tag}:constr_satisf_rate"].dtype == np.float32 and same_bits(rate, z[f"{tag}:constr_satisf_rate"])
    assert [info["violated_out"], info["violated_in"], info["cleared_by_a"], info["ties"]] == z[f"{tag}:stats"].tolist()
    # the result satisfies every constraint, and only zeroes edges
    assert np.bincount(ei[0][rp == 1], minlength=n).max() <= 1 and np.bincount(ei[1][rp == 1], minlength=n).max() <= 1
    assert not (rp > (p > 0.5)).any()
    labels = np_labels(ei, rp, n)
    assert np.array_equal(labels, z[f"{tag}:ped_ids"])
    for mtl in (2, 5):
        assert np.array_equal(np_keep(labels, mtl), z[f"{tag}:keep{mtl}"])


def test_fixture_cases_exercise_what_they_are_for(golden):
    z = golden("g19_projection.npz")
    for tag in SYNTHETIC:
        v_out, v_in, cleared, ties = z[f"{tag}:stats"].tolist()
        assert min(v_out, v_in, cleared) >= 10, tag       # ... and cleared < v_in: pass B has work left
        assert cleared < v_in
    assert z["t:stats"][3] >= 1 and (z["t:edge_preds"] == 0.5).any()
    ei, p, n = g19_case(z, "hub")
    hub = 65 * 5 + 2
    assert n == 650 and int(((p > 0.5) & (ei[0] == hub)).sum()) > 256 and int(((p > 0.5) & (ei[1] == hub)).sum()) > 256
    assert z["hub:keep5"].any() and not z["hub:keep5"].all()
    for tag in G19_CASES:
        assert z[f"{tag}:keep2"].any() and not z[f"{tag}:keep2"].all()


def test_restatement_on_hand_made_graphs():
    # node 0 has three active outgoing edges (ids 0, 1, 2: scores .9 .9 .7): the tie keeps id 0.  Node 3 then has the incoming
    # edges 0 (kept) and 3: the better-scored 3 wins pass B and edge 0 goes as well.
    ei = np.array([[0, 0, 0, 1, 2], [3, 4, 5, 3, 4]])
    p = np.array([0.9, 0.9, 0.7, 0.95, 0.5], np.float32)
    rp, flow_out, flow_in, v_out, v_in, nc = np_flows(ei, p, 6)
    assert rp.tolist() == [1, 1, 1, 1, 0] and flow_out.tolist() == [3, 1, 0, 0, 0, 0] and flow_in.tolist() == [0, 0, 0, 2, 1, 1]
    assert (v_out, v_in, nc) == (1, 1, 6)
    out, rate, info = np_greedy(ei, p, 6)
    assert out.tolist() == [0, 0, 0, 1, 0] and info["ties"] == 1 and info["cleared_by_a"] == 0
    assert rate == np.float32(1) - np.float32(2) / np.float32(6)
    assert np.isnan(np_rate(0, 0))
    nodes, edges, ids = np_violated(ei, p, 6)
    assert nodes.tolist() == [True, False, False, True, False, False] and ids.tolist() == [0, 1, 2, 3]
    g = component_graphs()
    assert np_labels(*g["chain_descending"]).tolist() == [0] * 200
    assert np_labels(*g["star_300"]).tolist() == [0] * 301
    assert np_labels(*g["duplicate_edge"]).tolist() == [0, 0, 1, 2, 3, 1, 4]
    assert np_labels(*g["isolated_nodes"]).tolist() == [0, 1, 2, 3, 1, 4, 5, 5, 6, 7]
    assert np_labels(*g["joined_by_last_edge"]).tolist() == [0, 0, 0, 1, 1, 0, 0, 0]
    assert np_labels(*g["inactive_only"]).tolist() == [0, 1, 2]
    assert np_labels(*g["single_node"]).tolist() == [0] and np_labels(*g["no_edges"]).tolist() == [0, 1, 2, 3, 4]
    assert np_keep(np.array([0, 0, 1, 2, 0, 2]), 2).tolist() == [True, True, False, True, True, True]
    assert np_keep(np.array([0, 0, 1, 2, 0, 2]), 3).tolist() == [True, True, False, False, True, False]


def test_restatement_labels_match_scipy():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for name, (ei, p, n) in component_graphs().items():
        act = p == 1
        m = sp.csr_matrix((np.ones(int(act.sum()), int), (ei[0][act], ei[1][act])), shape=(n, n))
        _, want = connected_components(csgraph=m, directed=False, return_labels=True)
        assert np.array_equal(np_labels(ei, p, n), want), name


def test_projection_entry_points_argument_checks_without_gpu():
    """Size queries and argument checks run on the host: empty inputs are successful no-ops, null pointers with a non-zero size
    and bad sizes are refused before any launch with the function's name in mpnhip_last_error(), a short workspace is
    MPNHIP_ERR_WORKSPACE."""
    l = capi.load()
    one = ctypes.c_void_p(256)   # a non-null address that no call below may reach a launch with
    big = 1 << 20
    # round and count
    assert l.mpnhip_project_round_count_workspace_bytes(0) == 0
    assert l.mpnhip_project_round_count_workspace_bytes(1000) >= 2000
    assert l.mpnhip_project_round_count(None, 0, 0, None, None, None, None, None, None, 0, None) == 0
    assert l.mpnhip_project_round_count(None, 5, 4, None, None, one, one, one, one, big, None) != 0
    assert b"project_round_count" in l.mpnhip_last_error()
    assert l.mpnhip_project_round_count(one, 5, 4, one, one, None, None, one, one, big, None) != 0
    assert b"project_round_count" in l.mpnhip_last_error()
    assert l.mpnhip_project_round_count(one, 5, 4, one, one, one, one, None, one, big, None) != 0   # the counters are always written
    assert l.mpnhip_project_round_count(one, -1, 4, one, one, one, one, one, one, big, None) != 0
    assert l.mpnhip_project_round_count(one, 5, 1 << 31, one, one, one, one, one, one, big, None) != 0
    assert l.mpnhip_project_round_count(one, 5, 400, one, one, one, one, one, one, 16, None) == MPNHIP_ERR_WORKSPACE
    assert l.mpnhip_project_round_count(one, 5, 400, one, one, one, one, one, None, big, None) == MPNHIP_ERR_WORKSPACE
    assert b"project_round_count" in l.mpnhip_last_error()
    # greedy passes
    assert l.mpnhip_project_greedy_workspace_bytes(0) == 0 and l.mpnhip_project_greedy_workspace_bytes(1000) >= 12000
    assert l.mpnhip_project_greedy(None, 0, 0, None, None, None, None, None, 0, None) == 0
    assert l.mpnhip_project_greedy(None, 0, 7, None, None, None, None, None, 0, None) == 0
    assert l.mpnhip_project_greedy(None, 5, 4, None, None, None, None, one, big, None) != 0
    assert b"project_greedy" in l.mpnhip_last_error()
    assert l.mpnhip_project_greedy(one, 5, 4, one, None, one, one, one, big, None) != 0
    assert l.mpnhip_project_greedy(one, 5, -4, one, one, one, one, one, big, None) != 0
    assert l.mpnhip_project_greedy(one, 5, 400, one, one, one, one, one, 16, None) == MPNHIP_ERR_WORKSPACE
    assert b"project_greedy" in l.mpnhip_last_error()
    # violated sub-problem
    assert l.mpnhip_project_violated_masks(None, 0, 0, None, None, None, None, None) == 0
    assert l.mpnhip_project_violated_masks(None, 5, 4, one, one, one, None, None) != 0
    assert b"project_violated_masks" in l.mpnhip_last_error()
    assert l.mpnhip_project_violated_masks(one, 5, 4, None, None, None, one, None) != 0
    assert b"project_violated_masks" in l.mpnhip_last_error()
    assert l.mpnhip_project_violated_masks(one, -5, 4, one, one, one, one, None) != 0
    # connected components
    assert l.mpnhip_connected_components_workspace_bytes(0) == 0
    small, large = l.mpnhip_connected_components_workspace_bytes(1000), l.mpnhip_connected_components_workspace_bytes(100000)
    assert 16000 <= small < large
    assert l.mpnhip_connected_components(None, 0, 0, None, None, None, None, 0, None) == 0
    assert l.mpnhip_connected_components(None, 0, 4, None, None, None, one, big, None) != 0          # labels of 4 nodes
    assert b"connected_components" in l.mpnhip_last_error()
    assert l.mpnhip_connected_components(None, 5, 4, None, one, None, one, big, None) != 0
    assert b"connected_components" in l.mpnhip_last_error()
    assert l.mpnhip_connected_components(one, 5, 400, one, one, None, one, 16, None) == MPNHIP_ERR_WORKSPACE
    assert l.mpnhip_connected_components(one, 5, 400, one, one, None, None, 0, None) == MPNHIP_ERR_WORKSPACE
    assert b"connected_components" in l.mpnhip_last_error()
    assert l.mpnhip_connected_components(one, 1 << 30, 4, one, one, None, one, big, None) != 0
    # track lengths
    assert l.mpnhip_track_lengths(None, 0, 2, None, None, None) == 0
    assert l.mpnhip_track_lengths(None, 4, 2, None, None, None) != 0
    assert b"track_lengths" in l.mpnhip_last_error()
    assert l.mpnhip_track_lengths(one, 4, 2, one, None, None) != 0
    assert l.mpnhip_track_lengths(one, -4, 2, one, one, None) != 0
    assert b"track_lengths" in l.mpnhip_last_error()


def _objective(p, x):
    return float(((1.0 - 2.0 * p.astype(np.float64)) * x).sum())


@pytest.mark.parametrize("tag", ["a", "b", "t"])
def test_default_lp_solver_on_the_violated_subproblems(golden, tag):
    """The scipy form of the reference's LP on the sub-problem ExactProjector would hand it: integral after snapping, every in- and
    out-constraint satisfied, and no worse than the greedy rounding of the same sub-problem plus M * 1e-6 (HiGHS's feasibility
    tolerance is 1e-7; the margin allows ten times that per edge)."""
    pytest.importorskip("scipy")
    from mpntrackseg_amd import projectors
    z = golden("g19_projection.npz")
    ei, p, n = g19_case(z, tag)
    _, _, ids = np_violated(ei, p, n)
    sub_ei, sub_p = ei[:, ids], p[ids]
    M = ids.size
    assert M >= 100
    x = projectors.snap(projectors.solve_with_scipy(sub_ei, sub_p))
    assert x.shape == (M,) and np.isin(x, (0.0, 1.0)).all()
    assert np.bincount(sub_ei[0], weights=x, minlength=n).max() <= 1 and np.bincount(sub_ei[1], weights=x, minlength=n).max() <= 1
    greedy, _, _ = np_greedy(sub_ei, sub_p, n)
    print("LP objective %.6f, greedy %.6f on %d edges" % (_objective(sub_p, x), _objective(sub_p, greedy), M))
    assert _objective(sub_p, x) <= _objective(sub_p, greedy) + M * 1e-6
    if tag == "a":   # without pulp, this is what default_solver() picks
        try:
            import pulp  # noqa: F401
        except ImportError:
            assert projectors.default_solver() is projectors.solve_with_scipy


def test_snap_and_solver_protocol():
    from mpntrackseg_amd import projectors
    v = projectors.snap([1e-7, 1 - 5e-7, 0.5, -1e-9, 1.0000005, 0.1])
    assert v.tolist() == [0.0, 1.0, 0.5, 0.0, 1.0, 0.1]
    assert projectors.solve_with_scipy(np.zeros((2, 0), np.int64), np.zeros(0, np.float32)).shape == (0,)
