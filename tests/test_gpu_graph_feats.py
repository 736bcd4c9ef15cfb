"""mpnhip_pairwise_distance and mpnhip_edge_features (csrc/graph_build.hip) through the C ABI -- so that the leading dimension
and the base pointer are the test's -- against tests/graph_feats_ref.py: numpy float64 on the same float32 inputs.
tests/test_graph_feats_ref_cpu.py pins that reference against float64 torch and shows that the bounds bind.

Bounds, u = 2^-24, per element against the magnitudes of graph_feats_ref (distance: sqrt(sum (|a - b| + eps)^2); time: |t_c| + |t_r|;
feet: |ref|; logarithms: 1 + |ref|):

  |got - ref| <= max(floor, 4 x the ratio of torch in float32 on the CPU on the same case) * magnitude
  floor: distance ((ceil(dim / 64) + 10) / 2 + 1) u, features 4 u   (counts of roundings: graph_feats_ref's docstring)

The distance kernel has a float4 path (dim % 4 == 0, ld % 4 == 0, base on a 16-byte boundary) and a scalar path; every width runs
dense, with ld = dim + 4, with ld = dim + 1 (scalar on a multiple-of-4 width) and from a base 4 bytes past a 16-byte boundary,
the padding columns of the strided forms holding 1e30.  Widths: 256 is the shipped ReID width (every lane busy, k ending at dim),
260 / 512 / 2048 take further iterations of k += 256.

MEASURED on the MI355X (worst ratio over the forms; float32 torch on the CPU in brackets):

  distance, width      4            64           252          256          260          512          2048
    float4 path        2.01 (2.01)  1.72 (1.97)  1.44 (2.17)  1.49 (1.69)  1.36 (2.79)  1.66 (4.07)  1.92 (21.56)
    scalar path        2.24         1.31         1.73         1.42         1.40         1.78         1.59          (ld + 1 and base + 4)
  distance, width      1            3            255          257
    scalar path        1.59 (1.59)  2.02 (2.13)  1.64 (3.21)  1.47 (1.92)
  features             secs_time_dists 1.00 (1.00)   norm_feet_x 2.46 (2.46)   norm_feet_y 2.37 (2.37)
                       bb_height_dists 1.67 (0.54)   bb_width_dists 1.66 (0.99)   (logf within HIP's 1 to 2 ulp; bound 4 u)

On a multiple-of-4 width the scalar forms (ld + 1, base + 4) give the same bits as each other and NOT as the float4 forms: 40 to
64 of the 303 edges differ by an ulp, by design (a lane sums other elements, in another order); both are held to float64.  ld + 4
equals the dense call bit for bit, and so do all four forms on the widths that are no multiple of 4.  No kernel exceeded its
bound; nothing in graph_build.hip or graph.py needed a fix.
"""
import numpy as np
import pytest
import torch

import graph_feats_ref as G
from mpntrackseg_amd import capi, synth

pytestmark = pytest.mark.gpu
U = G.U
SENT = 64
SENT_VALUE = -7.25
VECTOR_DIMS = (4, 64, 252, 256, 260, 512, 2048)
SCALAR_DIMS = (1, 3, 255, 257)
FPS = (29.97, 10.0, 1.0 / 3.0)
dev = lambda: torch.device("cuda:0")


def guarded(n):
    buf = torch.full((n + SENT,), SENT_VALUE, dtype=torch.float32, device=dev())
    buf[:n] = float("nan")
    return buf


def result(buf, n):
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert out[n:].tobytes() == np.full(SENT, SENT_VALUE, np.float32).tobytes(), "written behind the output"
    return out[:n]


# ------------------------------------------------------------------------------------------------ distance
def embedding_forms(emb):
    """-> {name: (tensor holding the rows, ld)}; ``tensor.data_ptr()`` is the base pointer the kernel gets"""
    n, dim = emb.shape
    forms = {"dense": (torch.from_numpy(emb).to(dev()), dim)}
    for name, pad in (("ld+4", 4), ("ld+1", 1)):
        wide = np.full((n, dim + pad), 1e30, np.float32)   # a read past dim cannot hide
        wide[:, :dim] = emb
        forms[name] = (torch.from_numpy(wide).to(dev()), dim + pad)
    big = torch.full((n * dim + 5,), 1e30, dtype=torch.float32, device=dev())
    view = big[1:1 + n * dim]
    view.copy_(torch.from_numpy(emb).to(dev()).view(-1))
    forms["base+4"] = (view, dim)
    assert forms["dense"][0].data_ptr() % 16 == 0 and forms["ld+4"][0].data_ptr() % 16 == 0
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return forms


def device_distance(t, ld, dim, ei):
    e = ei.shape[1]
    eit = torch.from_numpy(np.ascontiguousarray(ei)).to(dev())
    out = guarded(e)
    capi.check(capi.load().mpnhip_pairwise_distance(capi.ptr(t), ld, dim, capi.ptr(eit), e, G.EPS, capi.ptr(out), capi.stream_ptr()),
               "mpnhip_pairwise_distance")
    return result(out, e)


@pytest.mark.parametrize("dim", VECTOR_DIMS + SCALAR_DIMS)
def test_pairwise_distance(dim):
    emb, ei = G.dist_inputs(dim)
    assert emb.shape == (40, dim) and ei.shape == (2, 303) and ei.max() < 40 and ei.min() >= 0
    ref, mag = G.pairwise_distance(emb, ei)
    cmp = G.pairwise_distance_f32(emb, ei)
    got = {}
    for name, (t, ld) in embedding_forms(emb).items():
        got[name] = device_distance(t, ld, dim, ei)
        G.check("distance dim %d %s" % (dim, name), got[name], ref, mag, cmp, G.dist_floor(dim))
        for k in (1, 3, 4, 5):   # a block holds four edges; the last k edges: the self edge, the identical and the scaled pair
            part = device_distance(t, ld, dim, np.ascontiguousarray(ei[:, -k:]))
            assert part.tobytes() == got[name][-k:].tobytes(), (name, k)
    # the self edge and the identical rows: every difference is exactly 0, every term eps^2
    eps = float(np.float32(G.EPS))
    for name in got:
        assert abs(got[name][-3] - np.sqrt(dim) * eps) <= G.dist_floor(dim) * np.sqrt(dim) * eps and got[name][-3] == got[name][-2]
    print("distance dim %d: base+4 against dense: %s; ld+1 against dense: %s; ld+4 against dense: %s" % (
        dim, *("same bits" if got[k].tobytes() == got["dense"].tobytes() else
               "%d of 303 differ" % (got[k] != got["dense"]).sum() for k in ("base+4", "ld+1", "ld+4"))))
    assert got["ld+4"].tobytes() == got["dense"].tobytes()   # the same path, the same order


# ------------------------------------------------------------------------------------------------ edge features
def device_features(cols, ei, fps):
    e = ei.shape[1]
    eit = torch.from_numpy(np.ascontiguousarray(ei)).to(dev())
    frame = torch.from_numpy(cols["frame"]).to(dev())
    assert frame.dtype == torch.int64
    f = [torch.from_numpy(cols[k]).to(dev()) for k in ("bb_height", "bb_width", "feet_x", "feet_y")]
    out = guarded(e * 5)
    capi.check(capi.load().mpnhip_edge_features(capi.ptr(eit), e, frame.numel(), capi.ptr(frame), float(fps), capi.ptr(f[0]), capi.ptr(f[1]),
                                                capi.ptr(f[2]), capi.ptr(f[3]), capi.ptr(out), capi.stream_ptr()), "mpnhip_edge_features")
    return result(out, e * 5).reshape(e, 5)


def check_features(label, cols, ei, fps):
    got = device_features(cols, ei, fps)
    ref, mag = G.edge_features(ei, fps, *G.feat_args(cols))
    cmp = G.edge_features_f32(ei, fps, *G.feat_args(cols))
    for i, name in enumerate(G.FEAT_NAMES):
        G.check("%s fps %.4g %s" % (label, fps, name), got[:, i], ref[:, i], mag[:, i], cmp[:, i], G.FEAT_FLOOR)
    assert not got[ei[0] == ei[1]].any()   # a self edge: all five exactly 0
    return got


@pytest.mark.parametrize("fps", FPS)
def test_edge_features_of_all_pairs(fps):
    d = synth.make_detections(frames=10, seed=11)
    n = d["frame"].shape[0]
    r, c = np.divmod(np.arange(n * n, dtype=np.int64), n)
    ei = np.stack([r, c])
    assert ei.shape[1] > 257 and (r == c).sum() == n
    full = check_features("all pairs", d, ei, fps)
    for e in (1, 255, 256, 257):   # one block is 256 edges
        part = check_features("first %d pairs" % e, d, np.ascontiguousarray(ei[:, :e]), fps)
        assert part.tobytes() == full[:e].tobytes()


@pytest.mark.parametrize("fps", FPS)
def test_edge_features_hand_table(fps):
    cols, ei = G.hand_table()
    got = check_features("hand table", cols, ei, fps)
    assert not got[:3].any()                                 # three self edges
    assert not got[3:5, 3:].any() and got[3:5, :3].all()      # equal heights and widths at different nodes: both logs exactly 0
    assert got[5, 3] > 16 and got[6, 3] < -16                 # heights 1e-3 against 1e4
    assert got[7, 0] == 0 and got[8, 0] == 0                  # frames 2^24 and 2^24 + 1 are one float32
    assert got[9, 0] < -1e5 and got[10, 0] == -got[9, 0]
