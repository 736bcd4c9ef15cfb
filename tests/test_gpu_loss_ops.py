"""The three kernels that end a training step against tests/loss_ref.py (numpy float64), through the Python entry points:
the tracking loss and its logit gradient (csrc/loss.hip: k_count_pos, k_bce, k_graph_counts, k_bce_graphs, k_loss_reduce), the
segmentation loss (csrc/train_targets.hip: k_mask_counts, k_mask_bce in its three forms, k_mask_loss_reduce) and the optimizer step
(k_adam: mpnhip_adam_step and the counted form under train.FlatAdam).  The inputs are tests/loss_cases.py's table, which
tests/test_loss_ref_cpu.py evaluates in float32 on the CPU against the same bounds.

Bounds, u = 2^-24, every error measured per element against the MAGNITUDE the reference returns (the formulas cancel):

  gradients         |got - ref| <= max(16 u, 4 x the float32 CPU ratio of the case) * grad_mag
  losses [0 .. L]   |got - ref| <= max(16 u, 4 x the float32 CPU ratio of the case) * loss_mag
  Adam              |m' - ref| <= 4 u m_mag,  |v' - ref| <= 8 u v_mag,  |p' - ref| <= ulp32(|p|) + 1e-4 dp

16 u counts the roundings of the kernels' expression, it is not a measurement: expf / log1pf at HIP's documented 1 to 2 ulp, one
division, four or five multiply-adds, an 8-level float32 tree over 256 non-negative terms for the loss, double after that.  The
1e-4 dp of Adam covers 1 - powf(b2, t) at small t.  Where the reference is exactly 0 (steps below first_step, ids outside [0, K),
rows that are not valid, all-positive labels) the result must be exactly 0.

MEASURED on the MI355X (worst ratio of each group; the float32 CPU evaluation of the same cases in brackets):

  tracking loss, plain form (25 cases)      gradient 4.18 u (3.12 u)   loss 0.87 u (1.25 u)
  ... labels off a 16-byte boundary         gradient 3.70 u (3.08 u)   loss 0.54 u (0.68 u)   bit-equal to the aligned call
  tracking loss, per graph (5 cases)        gradient 3.42 u (3.02 u)   loss 0.56 u (0.56 u)   K = 1 against the plain form: 0 u
  mask loss (9 cases)                       gradient 3.36 u (2.81 u)   loss 0.83 u (1.37 u)
  Adam, one step (12 cases), of the bound   m 0.61 (0.72)   v 0.47 (0.62)   p 0.71 (0.71)
  Adam, guarded, 12 calls, accumulated      m 0.43 (0.43)   v 0.40 (0.40)   p 0.27 (0.27)
  z = -100 .. 100                           losses finite; gradients at 0.014 of 16 u grad_mag + 2^-126 weight / E

No case needed more than the fixed 16 u.  What the file did find: the mask loss of a row length that is a multiple of 4 depended on
the ALIGNMENT of the tensors -- off a 16-byte boundary the kernel fell back to single floats AND to another assignment of elements
to threads, so the float32 block sums came out one ulp apart (loss_out[0] of k = 3, P = 2048: 0x40c84762 against 0x40c84763;
gradients equal).  k_mask_bce now keeps the units of four floats of the row length whatever the access width.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_cases as LC
import loss_ref as LR
from mpntrackseg_amd import capi
from mpntrackseg_amd.loss import mask_loss_and_grad, tracking_loss_and_grad

pytestmark = pytest.mark.gpu
U = LR.U
dev = lambda: torch.device("cuda:0")


def on(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(t):
    return t.detach().cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ tracking loss
def run_tracking(inp, labels=None):
    eg = on(inp["edge_graph"]) if "edge_graph" in inp else None
    loss, grad = tracking_loss_and_grad(on(inp["logits"]), on(inp["labels"]) if labels is None else labels, inp["first_step"],
                                        inp["weight"], edge_graph=eg, n_graphs=inp.get("n_graphs", 1))
    assert loss.shape == (1 + inp["logits"].shape[0],) and grad.shape == inp["logits"].shape
    return loss, grad


@pytest.mark.parametrize("c", LC.PLAIN_CASES, ids=[LC.case_id(c) for c in LC.PLAIN_CASES])
def test_tracking_loss_plain(c):
    inp = LC.plain_inputs(c)
    loss, grad = run_tracking(inp)
    LC.check_loss("tracking " + LC.case_id(c), loss.cpu().numpy(), grad.cpu().numpy(), LC.tracking_ref(inp), LC.tracking_f32(inp))
    if c[2] >= c[1] or c[3] == 1.0:   # no classified step, or no negative label (pw = 0): everything exactly 0
        assert not loss.cpu().numpy().any() and not grad.cpu().numpy().any()


@pytest.mark.parametrize("c", LC.SLICE_CASES, ids=[LC.case_id(c) for c in LC.SLICE_CASES])
def test_tracking_loss_labels_off_a_16_byte_boundary(c):
    """labels as the slice [1 : 1 + E] of a larger tensor: k_count_pos' scalar path; bit-identical to the aligned call"""
    inp = LC.plain_inputs(c)
    E = c[0]
    big = torch.zeros(E + 9, dtype=torch.float32, device=dev())
    big[0] = 1.0          # (a neighbour that must not be counted, in front and behind)
    big[1 + E:] = 1.0
    view = big[1:1 + E]
    view.copy_(on(inp["labels"]))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and capi.f32c(view).view(-1).data_ptr() == view.data_ptr()
    aligned = on(inp["labels"])
    assert aligned.data_ptr() % 16 == 0
    l0, g0 = run_tracking(inp, aligned)
    l1, g1 = run_tracking(inp, view)
    assert bits(l0) == bits(l1) and bits(g0) == bits(g1)
    LC.check_loss("tracking slice " + LC.case_id(c), l1.cpu().numpy(), g1.cpu().numpy(), LC.tracking_ref(inp), LC.tracking_f32(inp))


@pytest.mark.parametrize("tag", LC.GRAPH_CASES)
def test_tracking_loss_graphs(tag):
    inp = LC.graph_inputs(tag)
    loss, grad = run_tracking(inp)
    ref = LC.tracking_ref(inp)
    LC.check_loss("tracking graphs " + tag, loss.cpu().numpy(), grad.cpu().numpy(), ref, LC.tracking_f32(inp))
    if tag == "one":   # K = 1: the plain form
        plain = dict((k, v) for k, v in inp.items() if k not in ("edge_graph", "n_graphs"))
        l1, g1 = run_tracking(plain)
        dg = LR.worst_ratio(grad.cpu().numpy().astype(np.float64) - g1.cpu().numpy(), np.zeros_like(ref[1]), ref[2])
        dl = LR.worst_ratio(loss.cpu().numpy().astype(np.float64) - l1.cpu().numpy(), np.zeros_like(ref[0]), ref[3])
        print("K = 1 against the plain form: gradient %.2f u, loss %.2f u" % (dg / U, dl / U))
        assert dg <= 2 * U and dl <= 2 * U
    if tag == "three_shuffled":   # an edge's gradient depends on its graph's counts only: the same bits wherever the edge lies
        base = LC.graph_inputs("three")
        _, g0 = run_tracking(base)
        (moved,) = LC._shuffle(5, g0.cpu().numpy())
        assert moved.tobytes() == grad.cpu().numpy().tobytes()
    if tag == "eight_out_of_range":
        out = (inp["edge_graph"] < 0) | (inp["edge_graph"] >= inp["n_graphs"])
        assert out.sum() == 10 and not grad.cpu().numpy()[:, out].any()


def test_tracking_loss_extreme_logits():
    """z in {-100, -88, 88, 100}: beyond |z| = 60 the sigmoid leaves the normal float32 range and no relative bound holds (for
    torch either): finite, and within 16 u grad_mag + 2^-126 weight / E"""
    inp = LC.extreme_inputs()
    loss, grad = run_tracking(inp)
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    _, rg, gm, _ = LC.tracking_ref(inp)
    print("extreme logits: loss", loss, "worst gradient error / (16 u grad_mag + 2^-126 w / E): %.3g"
          % float((np.abs(grad - rg) / (16 * U * gm + 2.0 ** -126 * inp["weight"] / 8)).max()))
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    assert (np.abs(grad - rg) <= 16 * U * gm + 2.0 ** -126 * inp["weight"] / 8).all()


# ------------------------------------------------------------------------------------------------ mask loss
def run_mask(inp, preds=None):
    pt = [on(p) for p in inp["preds"]] if preds is None else preds   # separate allocations
    ng = on(inp["node_graph"]) if "node_graph" in inp else None
    loss, grads = mask_loss_and_grad(pt, on(inp["labels"]), on(inp["valid"]), inp["weight"], node_graph=ng, n_graphs=inp.get("n_graphs", 1))
    assert loss.shape == (1 + len(pt),) and len(grads) == len(pt)
    return loss, torch.stack([g.view(inp["labels"].shape) for g in grads])


def check_mask(label, inp, loss, grad):
    ref = LC.mask_ref(inp)
    LC.check_loss(label, loss.cpu().numpy(), grad.cpu().numpy(), ref, LC.mask_f32(inp))
    ok = inp["valid"] & ((inp["node_graph"] >= 0) & (inp["node_graph"] < inp["n_graphs"]) if "node_graph" in inp else True)
    assert not grad.cpu().numpy()[:, ~ok].any() and grad.cpu().numpy()[:, ok].all()


@pytest.mark.parametrize("k,P", LC.MASK_CASES)
def test_mask_loss(k, P):
    inp = LC.mask_inputs(k, P)
    loss, grad = run_mask(inp)
    check_mask("mask k=%d P=%d" % (k, P), inp, loss, grad)


def test_mask_loss_graphs_with_an_id_out_of_range():
    """3 graphs over the 5 rows: a valid row with id 3 belongs to none of them, graph 1 has no valid row"""
    inp = LC.mask_inputs(3, 3136, graphs=True)
    loss, grad = run_mask(inp)
    check_mask("mask graphs k=3 P=3136", inp, loss, grad)


def test_mask_loss_off_a_16_byte_boundary_on_a_vector_shape():
    """P = 2048 with every prediction, and then every gradient tensor as well, 4 bytes past a 16-byte boundary: the scalar path on
    a vector shape, bit-identical to the aligned call"""
    k, P, N = 3, 2048, 5
    inp = LC.mask_inputs(k, P)
    l0, g0 = run_mask(inp)
    check_mask("mask aligned k=3 P=2048", inp, l0, g0)
    big = torch.zeros(1 + k * N * P, dtype=torch.float32, device=dev())
    views = [big[1 + s * N * P:1 + (s + 1) * N * P].view(N, P) for s in range(k)]
    for s in range(k):
        views[s].copy_(on(inp["preds"][s]))
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views)
    l1, g1 = run_mask(inp, views)
    assert bits(l0) == bits(l1) and bits(g0) == bits(g1)
    # ... and the gradients too, which mask_loss_and_grad allocates itself: the C entry
    lib = capi.load()
    gbig = torch.full((1 + k * N * P + 3,), 7.0, dtype=torch.float32, device=dev())
    gviews = [gbig[1 + s * N * P:1 + (s + 1) * N * P] for s in range(k)]
    assert all(v.data_ptr() % 16 == 4 for v in gviews)
    y, valid = on(inp["labels"]), on(inp["valid"]).view(torch.uint8)
    loss = torch.empty(1 + k, dtype=torch.float32, device=dev())
    ws = capi.workspace(lib.mpnhip_mask_loss_workspace_bytes(k, N, P, 1), dev(), "mask_loss")
    pa = (C.c_void_p * k)(*[v.data_ptr() for v in views])
    ga = (C.c_void_p * k)(*[v.data_ptr() for v in gviews])
    capi.check(lib.mpnhip_mask_loss(pa, k, capi.ptr(y), capi.ptr(valid), None, 1, N, P, float(inp["weight"]), capi.ptr(loss), ga,
                                    capi.ptr(ws), ws.numel(), capi.stream_ptr()), "mpnhip_mask_loss")
    assert bits(loss) == bits(l0) and bits(gbig[1:1 + k * N * P]) == bits(g0)
    assert bits(gbig[:1]) + bits(gbig[1 + k * N * P:]) == np.full(4, 7.0, np.float32).tobytes()   # nothing outside the views


# ------------------------------------------------------------------------------------------------ Adam
SPARE = np.array([7.5, -3.25, 1e30, -1e-30], np.float32)   # behind the n elements: must stay, bit for bit


def adam_call(p, g, m, v, t, wd):
    """one mpnhip_adam_step over the first n elements of buffers of n + 4 -> (p', m', v') as float32 arrays [n + 4]"""
    n = p.shape[0]
    bufs = [on(np.concatenate([a, SPARE])) for a in (p, g, m, v)]
    hp = LC.HYPER
    capi.check(capi.load().mpnhip_adam_step(capi.ptr(bufs[0]), capi.ptr(bufs[1]), capi.ptr(bufs[2]), capi.ptr(bufs[3]), n, hp["lr"], hp["b1"],
                                            hp["b2"], hp["eps"], wd, t, capi.stream_ptr()), "mpnhip_adam_step")
    out = [b.cpu().numpy() for b in bufs]
    assert out[1].tobytes() == np.concatenate([g, SPARE]).tobytes()   # the gradients are read only
    for o in out:
        assert o[n:].tobytes() == SPARE.tobytes()
    return out[0], out[2], out[3]


@pytest.mark.parametrize("c", LC.ADAM_CASES, ids=[LC.case_id(c) for c in LC.ADAM_CASES])
def test_adam_step(c):
    t, n, wd, scale = c
    p, g, m, v = LC.adam_inputs(c)
    got = [a[:n] for a in adam_call(p, g, m, v, t, wd)]
    ref = LR.adam_ref(p, g, m, v, t, wd=wd, **LC.HYPER)
    rm, rv, rp = LC.adam_ratios(got, p, ref)
    cm, cv, cp = LC.adam_ratios(LC.adam_f32(p, g, m, v, t, wd=wd, **LC.HYPER), p, ref)
    print("adam %s: of the bound: m kernel %.2f, float32 CPU %.2f; v kernel %.2f, float32 CPU %.2f; p kernel %.2f, float32 CPU %.2f"
          % (LC.case_id(c), rm, cm, rv, cv, rp, cp))
    assert rm <= 1 and rv <= 1 and rp <= 1


def test_adam_step_without_gradient_or_state_leaves_the_parameters():
    """g = 0, m = v = 0, wd = 0: the update is 0 / eps"""
    n = 257
    p = LC.synth.normal(77, (n,))
    z = np.zeros(n, np.float32)
    for t in (1, 1000):
        p1, m1, v1 = adam_call(p, z, z, z, t, 0.0)
        assert p1[:n].tobytes() == p.tobytes() and not m1[:n].any() and not v1[:n].any()


def test_guarded_adam_over_skipped_calls():
    """FlatAdam.step(guarded=True), 12 calls, skips 1,0,0,1,1,0,0,0,1,0,0,0: after every call p, exp_avg and exp_avg_sq equal
    adam_ref iterated over the APPLIED steps only (t is evaluated on the device), within the per-step bounds summed over those
    steps; a skipped call changes none of the three buffers"""
    from mpntrackseg_amd.train import FlatAdam, FlatBucket
    offs, n, p0, grads = LC.guarded_inputs()
    params = [on(p0[o:o + int(np.prod(s))].reshape(s)).requires_grad_(True) for s, o in zip(LC.GUARD_SHAPES, offs)]
    bucket = FlatBucket(params)
    assert bucket.n == n and bits(bucket.flat_params[:n]) == p0.tobytes()
    fopt = FlatAdam(bucket, lr=LC.GUARD_LR, weight_decay=LC.GUARD_WD)
    state = lambda: (bits(bucket.flat_params), bits(fopt.exp_avg), bits(fopt.exp_avg_sq))
    ref, f32 = LC.guarded_reference(p0, grads), LC.guarded_f32(p0, grads)
    worst = [0.0, 0.0, 0.0]
    for i, skip in enumerate(LC.GUARD_SKIPS):
        before = state()
        bucket.flat[:n].copy_(on(grads[i]))
        bucket.flat[n:].fill_(float(skip))
        fopt.step(guarded=True)
        if skip:
            assert state() == before
        else:
            assert state() != before
        rp, rm, rv, (bm, bv, bp) = ref[i]
        got = [t[:n].cpu().numpy() for t in (bucket.flat_params, fopt.exp_avg, fopt.exp_avg_sq)]
        r = (LC.ratio(np.abs(got[1] - rm), bm), LC.ratio(np.abs(got[2] - rv), bv), LC.ratio(np.abs(got[0] - rp), bp))
        c = (LC.ratio(np.abs(f32[i][1] - rm), bm), LC.ratio(np.abs(f32[i][2] - rv), bv), LC.ratio(np.abs(f32[i][0] - rp), bp))
        print("guarded call %2d (skip %d): of the accumulated bound: m kernel %.2f, float32 CPU %.2f; v kernel %.2f, float32 CPU %.2f; "
              "p kernel %.2f, float32 CPU %.2f" % (i, skip, r[0], c[0], r[1], c[1], r[2], c[2]))
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert max(r) <= 1, (i, r)
        assert not bucket.flat_params[n:].cpu().numpy().any() and not fopt.exp_avg[n:].cpu().numpy().any()
    assert fopt.t == 12 and fopt.applied_steps == 8
