"""tests/graph_feats_ref.py is right, its bounds bind, and mpnhip_pairwise_distance / mpnhip_edge_features check their arguments.
No GPU.

(a) The float64 references equal torch in float64 (F.pairwise_distance; the reference's feature expression) to 1e-12 of the
    magnitudes, on the inputs of tests/test_gpu_graph_feats.py.
(b) The float32 comparators (the same two with torch in float32 on the CPU) against the references: printed per case.
(c) Wrong formulas leave max(floor, 4 x comparator): eps omitted from the distance, eps added once per row; mean_h not halved, row
    and column swapped in one feature, log(h_r / h_c).
(d) Argument checks of the two entry points before any launch."""
import ctypes

import numpy as np
import pytest

import graph_feats_ref as G
from mpntrackseg_amd import capi, synth

U = G.U
PIN = 1e-12
DIMS = (1, 3, 4, 64, 252, 255, 256, 257, 260, 512, 2048)
FPS = (29.97, 10.0, 1.0 / 3.0)


def detections():
    d = synth.make_detections(frames=10, seed=11)
    n = d["frame"].shape[0]
    r, c = np.divmod(np.arange(n * n, dtype=np.int64), n)
    return d, np.stack([r, c])   # all ordered pairs, the self edges among them


@pytest.mark.parametrize("dim", DIMS)
def test_distance_reference_and_comparator(dim):
    import torch
    emb, ei = G.dist_inputs(dim)
    ref, mag = G.pairwise_distance(emb, ei)
    assert G.worst_ratio(G.pairwise_distance_f32(emb, ei, dtype=torch.float64), ref, mag) <= PIN
    assert (mag >= ref * (1 - 1e-15)).all() and (mag > 0).all()
    eps = float(np.float32(G.EPS))
    assert abs(ref[-3] - np.sqrt(dim) * eps) <= 1e-15 and abs(ref[-2] - np.sqrt(dim) * eps) <= 1e-15   # self edge, identical rows
    c = G.worst_ratio(G.pairwise_distance_f32(emb, ei), ref, mag)
    print("dim %4d: float32 torch CPU %.2f u (floor %.1f u, bound %.1f u)" % (dim, c / U, G.dist_floor(dim) / U, G.bound(G.dist_floor(dim), c) / U))
    assert np.isfinite(c)


@pytest.mark.parametrize("mutant", G.DIST_MUTANTS)
def test_distance_mutants_leave_the_bound(mutant):
    hit = []
    for dim in DIMS:
        emb, ei = G.dist_inputs(dim)
        ref, mag = G.pairwise_distance(emb, ei)
        bnd = G.bound(G.dist_floor(dim), G.worst_ratio(G.pairwise_distance_f32(emb, ei), ref, mag))
        r = G.worst_ratio(G.pairwise_distance(emb, ei, mutant=mutant)[0], ref, mag)
        print(mutant, dim, "%.3g u against %.1f u" % (r / U, bnd / U))
        if r > bnd:
            hit.append(dim)
    assert set(hit) == set(DIMS) if mutant == "no_eps" else {256, 2048} <= set(hit)   # (dim 1: eps once IS eps per element)


@pytest.mark.parametrize("fps", FPS)
def test_feature_reference_and_comparator(fps):
    import torch
    for label, (cols, ei) in (("detections", detections()), ("hand table", G.hand_table())):
        ref, mag = G.edge_features(ei, fps, *G.feat_args(cols))
        assert G.worst_ratio(G.edge_features_f32(ei, fps, *G.feat_args(cols), dtype=torch.float64), ref, mag) <= PIN
        cmp = G.edge_features_f32(ei, fps, *G.feat_args(cols))
        for i, name in enumerate(G.FEAT_NAMES):
            c = G.worst_ratio(cmp[:, i], ref[:, i], mag[:, i])
            print("%s fps %.4g %-18s float32 torch CPU %.2f u (bound %.1f u)" % (label, fps, name, c / U, G.bound(G.FEAT_FLOOR, c) / U))
            assert np.isfinite(c)
        self_edges = ei[0] == ei[1]
        assert self_edges.sum() >= 3 and not ref[self_edges].any() and not cmp[self_edges].any()
    cols, ei = G.hand_table()
    ref, _ = G.edge_features(ei, fps, *G.feat_args(cols))
    assert not ref[3:5, 3:].any() and ref[3:5, :3].all()          # equal heights and widths at different nodes: both logs exactly 0
    assert abs(ref[5, 3] - np.log(1e4 / float(np.float32(1e-3)))) < 1e-12 and ref[6, 3] == -ref[5, 3]
    assert ref[7, 0] == 0 and ref[8, 0] == 0                      # frames 2^24 and 2^24 + 1 are one float32
    assert abs(ref[9, 0] - (3 - 2.0 ** 24) / float(np.float32(fps))) < 1e-6


@pytest.mark.parametrize("mutant", G.FEAT_MUTANTS)
def test_feature_mutants_leave_the_bound(mutant):
    col = dict(mean_h_not_halved=(1, 2), feet_x_swapped=(1,), log_inverted=(3,))[mutant]
    for cols, ei in (detections(), G.hand_table()):
        ref, mag = G.edge_features(ei, FPS[0], *G.feat_args(cols))
        cmp = G.edge_features_f32(ei, FPS[0], *G.feat_args(cols))
        got, _ = G.edge_features(ei, FPS[0], *G.feat_args(cols), mutant=mutant)
        for i in range(5):
            r = G.worst_ratio(got[:, i], ref[:, i], mag[:, i])
            bnd = G.bound(G.FEAT_FLOOR, G.worst_ratio(cmp[:, i], ref[:, i], mag[:, i]))
            assert (r > bnd) == (i in col), (mutant, i, r / U)


def test_entry_points_argument_checks_without_gpu():
    """Everything below returns before a kernel is launched (the non-null pointers are host dummies that are never dereferenced)."""
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    f = ctypes.c_float

    def dist(emb=p, ld=8, dim=8, ei=p, e=3, out=p):
        return l.mpnhip_pairwise_distance(emb, ld, dim, ei, e, f(1e-6), out, None)

    def feats(ei=p, e=3, n=5, frame=p, fps=29.97, h=p, w=p, fx=p, fy=p, out=p):
        return l.mpnhip_edge_features(ei, e, n, frame, f(fps), h, w, fx, fy, out, None)

    assert dist(e=0) == 0 and dist(e=0, emb=None, ei=None, out=None) == 0
    for bad in (dict(e=-1), dict(dim=-1), dict(ld=7), dict(ld=-8, dim=-8), dict(emb=None), dict(ei=None), dict(out=None)):
        assert dist(**bad) != 0, bad
        assert b"pairwise_distance" in l.mpnhip_last_error(), bad
    assert feats(e=0) == 0 and feats(e=0, ei=None, frame=None, h=None, w=None, fx=None, fy=None, out=None) == 0
    for bad in (dict(e=-1), dict(n=-1), dict(fps=0.0), dict(fps=-29.97), dict(fps=float("nan"))) \
            + tuple({k: None} for k in ("ei", "frame", "h", "w", "fx", "fy", "out")):
        assert feats(**bad) != 0, bad
        assert b"edge_features" in l.mpnhip_last_error(), bad
    assert feats(fps=0.0) != 0 and b"fps" in l.mpnhip_last_error()
