"""Operator-level parity of the mask branch's neighbour aggregation (csrc/attention.hip: mpnhip_attention_aggregate and
mpnhip_attention_aggregate_backward, four kernels) against the float64 CPU oracle (oracle/attention_oracle.py, pinned to the
reference's own TimeAwareAttentionModel.forward by tests/golden/g18_attention.npz), called through the C ABI with every output
prefilled with NaN; and of mpnhip_avgpool against the float64 mean.

Error measure (as in the other operator tests): max |got - ref64| / max(max |ref64|, 1e-30) per tensor, over ALL elements.  The
only slots left out of a comparison are the ``weights`` and ``grad_logits`` slots of self-loop edges (row == col: in neither
direction), which are asserted UNTOUCHED instead.

Tolerances.  Segments of at most ~1000 edges: 3e-6, the bound tests/test_gpu_wgrad.py uses for fp32 accumulations of that length (a
float32 CPU evaluation of the same formula stays below 6e-7 on the random shapes below).  The hub graph (segments of 15,360 and
15,361 edges summed sequentially in fp32): 4 x the error of the float32 CPU evaluation of the oracle on the same inputs, never less
than 3e-6 -- the 4 x covers the different summation order and expf of two fp32 evaluations of one formula.  Every case prints the
kernel's error and the float32 CPU evaluation's error (DESIGN.md section 2 keeps the table of an MI355X run)."""
import numpy as np
import pytest
import torch

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.mpn import TimeAwareAttentionModel, _AttentionAggregate
from oracle import attention_oracle as AO

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 3e-6
TENSORS = ("flow_in", "flow_out", "weights", "grad_x", "grad_logits")
SENTINEL = 7.25   # prefill of the grad_logits slots of self-loop edges (grad_logits is "+=": it cannot be prefilled with NaN)


def err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def directions(ei):
    return np.where(ei[0] < ei[1], 0, np.where(ei[0] > ei[1], 1, 2))


class Run:
    """One prepared graph with its inputs on the device; forward() / backward() go straight through the C ABI."""

    def __init__(self, N, ei, x, lg):
        self.N, self.E, self.F = int(N), int(ei.shape[1]), int(x.shape[1])
        self.ei = np.ascontiguousarray(ei, np.int64).reshape(2, self.E)
        self.lib = capi.load()
        self.pg = capi.PreparedGraph(torch.from_numpy(self.ei).to(dev()), self.N, validate=True, full=True)
        self.x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev())
        self.lg = torch.from_numpy(np.ascontiguousarray(lg, np.float32)).to(dev())
        # perm is the first int array after the 256-byte header (as tests/test_gpu_parity.py::test_graph_prep_order reads it):
        # sorted position -> edge_index position; direction 0 (row < col), then 1 (row > col), then the self loops
        d = directions(self.ei)
        self.perm = self.pg.buf.cpu().numpy()[256:256 + 4 * self.E].view(np.int32).astype(np.int64)
        assert np.array_equal(self.perm, np.argsort(d * self.N + self.ei[0], kind="stable"))
        self.n_dir = int((d < 2).sum())
        self.loops = d == 2

    def forward(self, want_weights=True):
        out_in, out_out = nan_like((self.N, self.F)), nan_like((self.N, self.F))
        wts = nan_like((max(self.E, 1),)) if want_weights else None
        capi.check(self.lib.mpnhip_attention_aggregate(capi.ptr(self.pg.buf), self.N, self.E, capi.ptr(self.x), self.F, capi.ptr(self.lg),
                                                       capi.ptr(out_in), capi.ptr(out_out), capi.ptr(wts), capi.stream_ptr()), "attention")
        torch.cuda.synchronize()
        return out_in, out_out, wts

    def backward(self, wts, g_in, g_out, grad_x, accumulate, grad_logits):
        dw = nan_like((max(self.E, 1),))
        capi.check(self.lib.mpnhip_attention_aggregate_backward(capi.ptr(self.pg.buf), self.N, self.E, capi.ptr(self.x), self.F, capi.ptr(wts),
                                                                capi.ptr(g_in), capi.ptr(g_out), capi.ptr(grad_x), int(accumulate),
                                                                capi.ptr(grad_logits), capi.ptr(dw), capi.stream_ptr()), "attention_backward")
        torch.cuda.synchronize()

    def weights_in_edge_order(self, wts):
        """(weights of the non-self-loop edges scattered to edge_index order, NaN elsewhere; the untouched tail)"""
        w = wts.cpu().numpy()
        out = np.full(self.E, np.nan, np.float32)
        out[self.perm[:self.n_dir]] = w[:self.n_dir]
        return out, w[self.n_dir:self.E]

    def gl_prefill(self):
        gl = torch.zeros(max(self.E, 1), dtype=torch.float32, device=dev())
        gl[:self.E][torch.from_numpy(self.loops).to(dev())] = SENTINEL
        return gl


def check_case(name, N, ei, x, lg, hub=False, seed=100):
    """Forward and backward of one graph against the float64 oracle, all elements; the forward again with weights = NULL and
    each half of the backward alone (bitwise equal to the first run: no atomics anywhere); exact zeros where nothing lands; the
    self-loop slots untouched.  Returns {tensor: (kernel error, float32 CPU evaluation's error)} and the run's tensors."""
    r = Run(N, ei, x, lg)
    g_in = synth.normal(seed, (r.N, r.F), stream=1)
    g_out = synth.normal(seed, (r.N, r.F), stream=2)
    ref = AO.attention_aggregate_with_grads(x, r.ei, lg, g_in, g_out, torch.float64)
    f32 = AO.attention_aggregate_with_grads(x, r.ei, lg, g_in, g_out, torch.float32)

    out_in, out_out, wts = r.forward()
    gi_d, go_d = torch.from_numpy(g_in).to(dev()), torch.from_numpy(g_out).to(dev())
    gx, gl = nan_like((r.N, r.F)), r.gl_prefill()
    r.backward(wts, gi_d, go_d, gx, 0, gl)
    w_edge, w_tail = r.weights_in_edge_order(wts)
    got = {"flow_in": out_in.cpu().numpy(), "flow_out": out_out.cpu().numpy(), "weights": w_edge, "grad_x": gx.cpu().numpy(),
           "grad_logits": gl[:r.E].cpu().numpy()}

    keep = ~r.loops
    # self loops: weight slots still hold the NaN prefill, grad_logits slots still hold the sentinel
    assert np.isnan(w_tail).all() and w_tail.size == int(r.loops.sum()), name
    assert (got["grad_logits"][r.loops] == np.float32(SENTINEL)).all(), name
    errs = {}
    for k in TENSORS:
        a, b, c = got[k], ref[k], f32[k]
        if k in ("weights", "grad_logits"):
            a, b, c = a[keep], b[keep], c[keep]
        assert np.isfinite(a).all(), (name, k, "non-finite output")
        errs[k] = (err(a, b), err(c, b))
        print("ATTN_ERR %-28s %-12s kernel %.2e  float32-cpu %.2e" % (name, k, errs[k][0], errs[k][1]))
    for k in TENSORS:
        tol = max(4.0 * errs[k][1], TOL) if hub else TOL
        assert errs[k][0] <= tol, (name, k, errs[k], tol)

    # exact zeros: rows of empty segments, grad_x of nodes that are nobody's neighbour in either direction
    d = directions(r.ei)
    for dirn, key in ((1, "flow_in"), (0, "flow_out")):
        empty = np.ones(r.N, bool)
        empty[r.ei[0][d == dirn]] = False
        assert not got[key][empty].any(), (name, key, "empty segment rows must be exactly 0")
    lonely = np.ones(r.N, bool)
    lonely[r.ei[1][d < 2]] = False
    assert not got["grad_x"][lonely].any(), name

    # again: the forward with weights = NULL, the backward one gradient at a time -- bitwise the same
    out_in2, out_out2, _ = r.forward(want_weights=False)
    assert torch.equal(out_in, out_in2) and torch.equal(out_out, out_out2), name
    out_in3, out_out3, wts3 = r.forward()
    assert torch.equal(out_in, out_in3) and torch.equal(out_out, out_out3), name
    assert torch.equal(wts[:r.n_dir], wts3[:r.n_dir]), name
    gx2 = nan_like((r.N, r.F))
    r.backward(wts, gi_d, go_d, gx2, 0, None)
    gl2 = r.gl_prefill()
    r.backward(wts, gi_d, go_d, None, 0, gl2)
    assert torch.equal(gx, gx2) and torch.equal(gl, gl2), name
    return errs, r, got, ref


def random_graph(N, E, F, std, seed):
    """Uniformly random (row, col): self loops and duplicate edges occur on their own."""
    ei = np.stack([(synth.uniform01(seed, E, stream=0) * N).astype(np.int64), (synth.uniform01(seed, E, stream=1) * N).astype(np.int64)])
    return ei, synth.normal(seed, (N, F), stream=2), synth.normal(seed, (E,), stream=3, std=std)


# ------------------------------------------------------------------------------------ the reference's own numbers
def test_fixture_g18(golden):
    z = golden("g18_attention.npz")
    N, F = z["x"].shape[0], int(np.prod(z["x"].shape[1:]))
    x, lg, up = z["x"].reshape(N, F), z["logits"].reshape(-1), z["upstream"]
    r = Run(N, z["edge_index"], x, lg)
    out_in, out_out, wts = r.forward()
    gi_d = torch.from_numpy(np.ascontiguousarray(up[:, 4:8].reshape(N, F))).to(dev())
    go_d = torch.from_numpy(np.ascontiguousarray(up[:, 8:12].reshape(N, F))).to(dev())
    gx, gl = nan_like((N, F)), r.gl_prefill()
    r.backward(wts, gi_d, go_d, gx, 0, gl)
    ref = AO.attention_aggregate_with_grads(x, z["edge_index"], lg, up[:, 4:8], up[:, 8:12], torch.float64)
    keep = ~r.loops
    # the reference concatenates (x, flow_in, flow_out): its gradient of x holds the pass-through term as well
    total = gx.cpu().numpy().astype(np.float64) + up[:, :4].reshape(N, F)
    pairs = {"flow_in": (out_in.cpu().numpy(), ref["flow_in"], z["flow_in"].reshape(N, F)),
             "flow_out": (out_out.cpu().numpy(), ref["flow_out"], z["flow_out"].reshape(N, F)),
             "grad_x": (total, ref["grad_x"] + up[:, :4].reshape(N, F), z["grad_x_total"].reshape(N, F)),
             "grad_logits": (gl[:r.E].cpu().numpy()[keep], ref["grad_logits"][keep], z["grad_logits"].reshape(-1)[keep])}
    for k, (a, b, c) in pairs.items():
        e64, e_fix, e_ref = err(a, b), err(a, c), err(c, b)
        print("ATTN_ERR %-28s %-12s kernel %.2e  float32-cpu %.2e  (kernel against the fixture %.2e)" % ("g18", k, e64, e_ref, e_fix))
        assert e64 <= TOL, (k, e64)
        # the fixture is the reference's float32 run: within 1e-6 of float64 (tests/test_oracle_golden.py), on top of the 3e-6
        assert e_fix <= TOL + 1e-6, (k, e_fix)
    assert (gl[:r.E].cpu().numpy()[r.loops] == np.float32(SENTINEL)).all()
    assert not out_in[:2].cpu().numpy().any() and not out_out[:2].cpu().numpy().any()
    w_edge, w_tail = r.weights_in_edge_order(wts)
    assert np.isnan(w_tail).all() and err(w_edge[keep], ref["weights"][keep]) <= TOL


# ------------------------------------------------------------------------------------ random graphs
@pytest.mark.parametrize("N,E,F,std", [(300, 5000, 12544, 1.0), (50, 3000, 260, 3.0), (700, 2000, 4, 30.0), (40, 12000, 1028, 1.0),
                                       (60, 1500, 1020, 2.0), (60, 1500, 1024, 2.0)])
def test_random_graphs(N, E, F, std):
    """F / 4 = 3136, 65, 1, 257, 255 and 256 columns of four floats against the 256-lane stride; segments of a few to ~190 edges."""
    ei, x, lg = random_graph(N, E, F, std, seed=N + E)
    check_case("random N%d E%d F%d" % (N, E, F), N, ei, x, lg)


# ------------------------------------------------------------------------------------ segment lengths
SEG_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1000]


def segment_graph():
    """Centre node k has exactly SEG_LENGTHS[k] past neighbours (row > col: nodes 0 .. len-1) and as many future neighbours
    (row < col), in a shuffled edge order; the neighbour pools have no segment of their own."""
    M, C = max(SEG_LENGTHS), len(SEG_LENGTHS)
    rows, cols = [], []
    for k, n in enumerate(SEG_LENGTHS):
        rows += [M + k] * (2 * n)
        cols += list(range(n)) + list(range(M + C, M + C + n))
    ei = np.array([rows, cols], dtype=np.int64)
    ei = ei[:, np.argsort(synth.uniform01(41, ei.shape[1], stream=0), kind="stable")]
    return 2 * M + C, ei


@pytest.mark.parametrize("where", ["last", "first"])
def test_segment_lengths(where):
    """Every length around the 4-wide unrolled tail (len % 4 = 0..3) and around the 256-lane strided loops, each segment's
    largest logit moved (swapped) to its last (first) sorted edge: a dropped or doubled tail edge moves the row by its largest
    weight -- O(1) in the short segments, 0.8 % in the 1000-edge one, against a bound of 3e-6.

    The largest logit is NOT raised above the others.  With one weight w -> 1 the logit gradient w (dw - sum_k w_k dw_k) shrinks
    like (1 - w) while the error of any float32 evaluation stays at eps * |dw| (float32 weights sum to 1 only within rounding), so
    max |err| / max |ref| stops measuring the kernel: with the largest logit raised by 8 over N(0, 1) logits an MI355X run gave
    grad_logits 3.8e-6 (last) / 5.2e-6 (first) with every other tensor <= 6.6e-7, and the float32 CPU evaluation of the oracle
    itself 1.8e-7 / 1.7e-6."""
    N, ei = segment_graph()
    E = ei.shape[1]
    lg = synth.normal(42, (E,), stream=0)
    d = directions(ei)
    top = []
    for k, n in enumerate(SEG_LENGTHS):
        for dirn in (0, 1):
            ids = np.nonzero((ei[0] == max(SEG_LENGTHS) + k) & (d == dirn))[0]    # ascending = the sorted order (stable sort)
            assert ids.size == n
            if n:
                a, b = ids[np.argmax(lg[ids])], (ids[-1] if where == "last" else ids[0])
                lg[a], lg[b] = lg[b], lg[a]
                top.append(b)
    assert len(top) == 2 * (len(SEG_LENGTHS) - 1)
    x = synth.normal(43, (N, 8), stream=0)
    errs, r, got, ref = check_case("segment lengths, largest " + where, N, ei, x, lg)
    # the edge that a wrong tail would drop or double carries a weight of at least 300 x the bound in every segment
    assert float(ref["weights"][top].min()) > 1e-3


# ------------------------------------------------------------------------------------ hub segments around the LDS buffer
HUB_A, HUB_B = 15360, 15361    # the 60 KB weight buffer holds 15,360 floats


def hub_graph():
    """Node 0 with 15,360 future neighbours (fits the LDS weight buffer), node 1 with 15,361 (does not), and the reverse
    edges: the two hubs are then the neighbour of as many rows in k_attention_dx.  Shuffled edge order."""
    a = np.arange(2, 2 + HUB_A, dtype=np.int64)
    b = np.arange(2 + HUB_A, 2 + HUB_A + HUB_B, dtype=np.int64)
    rows = np.concatenate([np.zeros(HUB_A, np.int64), np.ones(HUB_B, np.int64), a, b])
    cols = np.concatenate([a, b, np.zeros(HUB_A, np.int64), np.ones(HUB_B, np.int64)])
    ei = np.stack([rows, cols])
    ei = ei[:, np.argsort(synth.uniform01(51, ei.shape[1], stream=0), kind="stable")]
    return 2 + HUB_A + HUB_B, ei


@pytest.mark.parametrize("dominant_last", [False, True])
def test_hub_segments(dominant_last):
    N, ei = hub_graph()
    E = ei.shape[1]
    assert E * 4 > 60 * 1024   # the weight buffer is at its cap
    lg = synth.normal(52, (E,), stream=0, std=3.0)
    if dominant_last:
        ids = np.nonzero((ei[0] == 1) & (ei[1] > 1))[0]
        assert ids.size == HUB_B
        lg[ids[-1]] = lg[ids].max() + 8.0
    x = synth.normal(53, (N, 8), stream=0)
    errs, r, got, ref = check_case("hub 15360/15361" + (", dominant last" if dominant_last else ""), N, ei, x, lg, hub=True)
    if dominant_last:
        assert float(ref["weights"][ids[-1]]) > 0.9


# ------------------------------------------------------------------------------------ degenerate inputs
def test_no_edges():
    N, F = 7, 8
    errs, r, got, ref = check_case("E = 0", N, np.zeros((2, 0), np.int64), synth.normal(61, (N, F)), np.zeros(0, np.float32))
    assert not got["flow_in"].any() and not got["flow_out"].any() and not got["grad_x"].any()


def test_no_nodes():
    """N = 0: a successful no-op that touches nothing (the graph buffer is only checked for null)."""
    lib = capi.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev())
    capi.check(lib.mpnhip_attention_aggregate(capi.ptr(buf), 0, 0, None, 8, None, None, None, None, capi.stream_ptr()), "attention")
    capi.check(lib.mpnhip_attention_aggregate_backward(capi.ptr(buf), 0, 0, None, 8, None, None, None, None, 0, None, None,
                                                       capi.stream_ptr()), "attention_backward")
    torch.cuda.synchronize()
    assert not buf.any()


def test_self_loops_only():
    N, F = 6, 8
    ei = np.array([[0, 1, 1, 3, 5, 5, 5], [0, 1, 1, 3, 5, 5, 5]], np.int64)
    lg = synth.normal(62, (7,))
    errs, r, got, ref = check_case("self loops only", N, ei, synth.normal(63, (N, F)), lg)
    assert not got["flow_in"].any() and not got["flow_out"].any() and not got["grad_x"].any() and r.n_dir == 0


def test_all_equal_logits():
    """Equal logits need no max-subtraction: every weight is 1 / len up to the 1e-12 of the composite."""
    N, E, F = 30, 900, 16
    ei, x, _ = random_graph(N, E, F, 1.0, seed=64)
    lg = np.full(E, 0.7, np.float32)
    errs, r, got, ref = check_case("all-equal logits", N, ei, x, lg)
    d = directions(ei)
    for dirn in (0, 1):
        m = d == dirn
        cnt = np.bincount(ei[0][m], minlength=N)
        assert err(got["weights"][m], 1.0 / cnt[ei[0][m]]) <= TOL


def test_logit_spread_of_160():
    """Logits of +-80: exp(-160) is far below the smallest float32, so next to a +80 edge a -80 edge weighs exactly 0 --
    and nothing overflows, because the segment's maximum is subtracted first."""
    N, E, F = 30, 900, 16
    ei, x, _ = random_graph(N, E, F, 1.0, seed=65)
    lg = np.where(synth.uniform01(65, E, stream=7) < 0.5, 80.0, -80.0).astype(np.float32)
    errs, r, got, ref = check_case("logits +-80", N, ei, x, lg)
    d = directions(ei)
    zero = np.zeros(E, bool)
    for dirn in (0, 1):
        m = d == dirn
        has_hi = np.zeros(N, bool)
        has_hi[ei[0][m & (lg > 0)]] = True
        zero |= m & (lg < 0) & has_hi[ei[0]]
    assert zero.sum() > 100 and (got["weights"][zero] == 0.0).all() and (got["grad_logits"][zero] == 0.0).all()


# ------------------------------------------------------------------------------------ containment
@pytest.mark.parametrize("which", ["g18", "random"])
def test_nan_logits_on_self_loops_are_contained(golden, which):
    """A self loop is in neither direction: a NaN logit on it reaches no output, no weight and no gradient (check_case asserts
    every output finite and correct, the self loops' weight slots still NaN and their grad_logits slots untouched)."""
    if which == "g18":
        z = golden("g18_attention.npz")
        ei, N = z["edge_index"], z["x"].shape[0]
        x, lg = z["x"].reshape(N, -1), z["logits"].reshape(-1).copy()
    else:
        N = 20
        ei, x, lg = random_graph(N, 1200, 40, 2.0, seed=66)
    loops = ei[0] == ei[1]
    assert loops.sum() >= 6
    lg[loops] = np.nan
    check_case("NaN self loops, " + which, N, ei, x, lg)


# ------------------------------------------------------------------------------------ accumulation
def test_accumulate_grad_x_and_grad_logits():
    """accumulate_grad_x = 1 adds to what grad_x holds; grad_logits is always "+=" (include/mpnhip.h).  The prefill is of the
    size of the gradient itself, so old + new is compared at the same 3e-6 (one more float32 rounding, 6e-8)."""
    N, E, F = 50, 3000, 260
    ei, x, lg = random_graph(N, E, F, 3.0, seed=67)
    r = Run(N, ei, x, lg)
    g_in, g_out = synth.normal(68, (N, F), stream=1), synth.normal(68, (N, F), stream=2)
    ref = AO.attention_aggregate_with_grads(x, ei, lg, g_in, g_out, torch.float64)
    old_x = synth.normal(69, (N, F), stream=1, std=float(np.abs(ref["grad_x"]).max()) / 3)
    old_l = synth.normal(69, (E,), stream=2, std=float(np.abs(ref["grad_logits"]).max()) / 3)
    _, _, wts = r.forward()
    gi_d, go_d = torch.from_numpy(g_in).to(dev()), torch.from_numpy(g_out).to(dev())
    gx, gl = torch.from_numpy(old_x).to(dev()), torch.from_numpy(old_l).to(dev())
    r.backward(wts, gi_d, go_d, gx, 1, gl)
    want_x, want_l = ref["grad_x"] + old_x, ref["grad_logits"] + old_l
    e_x, e_l = err(gx.cpu().numpy(), want_x), err(gl.cpu().numpy(), want_l)
    print("ATTN_ERR %-28s %-12s kernel %.2e" % ("accumulate", "grad_x", e_x))
    print("ATTN_ERR %-28s %-12s kernel %.2e" % ("accumulate", "grad_logits", e_l))
    assert e_x <= TOL and e_l <= TOL
    assert np.array_equal(gl.cpu().numpy()[r.loops], old_l[r.loops])
    # the old values really matter: without them the same comparison fails by far
    assert err(ref["grad_x"], want_x) > 1e-2 and err(ref["grad_logits"], want_l) > 1e-2
    # accumulate_grad_x = 0 over the same non-zero buffer overwrites
    gx0 = torch.from_numpy(old_x).to(dev())
    r.backward(wts, gi_d, go_d, gx0, 0, None)
    assert err(gx0.cpu().numpy(), ref["grad_x"]) <= TOL


# ------------------------------------------------------------------------------------ the autograd glue
@pytest.mark.parametrize("needs", ["x", "logits", "both"])
def test_autograd_function_and_module(needs):
    """_AttentionAggregate.apply and TimeAwareAttentionModel.aggregate (identity node_model) with every needs_input_grad
    combination: the null grad_x / null grad_logits calls of the backward, and the "+=" of grad_logits over the glue's zeros."""
    N, E, C = 40, 2500, 65
    ei, x, lg = random_graph(N, E, 4 * C, 2.0, seed=70)
    x4 = x.reshape(N, C, 2, 2)
    g_in, g_out = synth.normal(71, (N, 4 * C), stream=1), synth.normal(71, (N, 4 * C), stream=2)
    ref = AO.attention_aggregate_with_grads(x, ei, lg, g_in, g_out, torch.float64)
    ei_d = torch.from_numpy(ei).to(dev())
    xd = torch.from_numpy(x4).to(dev()).requires_grad_(needs in ("x", "both"))
    ld = torch.from_numpy(lg).view(E, 1).to(dev()).requires_grad_(needs in ("logits", "both"))
    gi_d, go_d = torch.from_numpy(g_in).view(N, C, 2, 2).to(dev()), torch.from_numpy(g_out).view(N, C, 2, 2).to(dev())

    pg = capi.PreparedGraph(ei_d, N, full=True)
    flow_in, flow_out = _AttentionAggregate.apply(pg, xd, ld)
    assert flow_in.shape == x4.shape and flow_out.shape == x4.shape
    ((flow_in * gi_d).sum() + (flow_out * go_d).sum()).backward()
    assert err(flow_in.detach().cpu().numpy().reshape(N, -1), ref["flow_in"]) <= TOL
    assert err(flow_out.detach().cpu().numpy().reshape(N, -1), ref["flow_out"]) <= TOL
    if needs in ("x", "both"):
        assert xd.grad.shape == xd.shape and err(xd.grad.cpu().numpy().reshape(N, -1), ref["grad_x"]) <= TOL
    else:
        assert xd.grad is None
    if needs in ("logits", "both"):
        assert ld.grad.shape == ld.shape and err(ld.grad.cpu().numpy().reshape(-1), ref["grad_logits"]) <= TOL
        assert not ld.grad.cpu().numpy().reshape(-1)[ei[0] == ei[1]].any()
    else:
        assert ld.grad is None

    # the module: cat(x, flow_in, flow_out) through an identity node_model (reference models/mpn.py:136-137)
    xd2 = xd.detach().clone().requires_grad_(xd.requires_grad)
    ld2 = ld.detach().clone().requires_grad_(ld.requires_grad)
    flow = TimeAwareAttentionModel(torch.nn.Identity()).aggregate(xd2, ei_d, ld2)
    assert flow.shape == (N, 3 * C, 2, 2) and torch.equal(flow[:, :C], xd2)
    assert torch.equal(flow[:, C:2 * C], flow_in) and torch.equal(flow[:, 2 * C:], flow_out)
    ((flow[:, C:2 * C] * gi_d).sum() + (flow[:, 2 * C:] * go_d).sum()).backward()
    if xd.requires_grad:
        assert torch.equal(xd2.grad, xd.grad)
    if ld.requires_grad:
        assert torch.equal(ld2.grad, ld.grad)


# ------------------------------------------------------------------------------------ mpnhip_avgpool
@pytest.mark.parametrize("hw", [1, 3, 49, 64, 196, 1000])
@pytest.mark.parametrize("rows", [1, 255, 257, 37 * 64])
def test_avgpool_matches_float64_mean(rows, hw):
    """nn.AdaptiveAvgPool2d((1, 1)) + view over [rows, hw]: production runs hw = 196 (14 x 14) and hw = 1; hw below, at and
    above the 64 lanes that share a row; row counts around the 256-thread block.  1e-6 as tests/test_gpu_parity.py::test_avg_pool."""
    lib = capi.load()
    x = synth.normal(80 + hw, (rows, hw), stream=rows) + np.float32(0.5)
    xd = torch.from_numpy(x).to(dev())
    y = nan_like((rows + 3,))                 # three guard slots behind the output
    capi.check(lib.mpnhip_avgpool(capi.ptr(xd), rows, hw, capi.ptr(y), capi.stream_ptr()), "mpnhip_avgpool")
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.isnan(got[rows:]).all()
    e = err(got[:rows], x.astype(np.float64).mean(axis=1))
    print("AVGPOOL_ERR rows %d hw %d kernel %.2e" % (rows, hw, e))
    assert e < 1e-6
    if hw == 1:
        assert np.array_equal(got[:rows], x[:, 0])


def test_avgpool_without_rows_is_a_noop():
    lib = capi.load()
    y = nan_like((4,))
    capi.check(lib.mpnhip_avgpool(None, 0, 196, capi.ptr(y), capi.stream_ptr()), "mpnhip_avgpool")
    capi.check(lib.mpnhip_avgpool(None, 0, 196, None, capi.stream_ptr()), "mpnhip_avgpool")
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
    from mpntrackseg_amd.mpn import avg_pool
    out = avg_pool(torch.zeros((0, 64, 14, 14), device=dev()))
    assert out.shape == (0, 64)
