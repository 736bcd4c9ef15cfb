"""tests/loss_ref.py is right, and float32 alone fits the bounds of tests/test_gpu_loss_ops.py.  No GPU.

(a) The float64 references equal torch in float64 (binary_cross_entropy_with_logits with autograd, torch.optim.Adam) to 1e-12 of
the magnitudes they return, and agree with oracle/loss_oracle.py and the g9 / g16 fixtures at those tests' tolerances.

(b) For every input set of the GPU file (tests/loss_cases.py: one table for both files) a float32 evaluation on the CPU -- torch
for the losses, a numpy restatement of k_adam's expression order for Adam -- stays inside the bounds the kernels are held to:

  * loss values and gradients: at most 8 u of loss_mag / grad_mag, half of the fixed 16 u (measured: gradients 3.2 u, losses 1.4 u);
  * Adam m and v: inside 4 u m_mag and 8 u v_mag.  These two are the WORST-CASE rounding counts of the unfused expression (m: the
    roundings of wd p, g + wd p, (1 - b1) gi, b1 m and the last sum, each at most u of its own result: at most 4 u of m_mag when
    wd p dominates; v: twice the 2 u of gi, two products, b2 v and the sum: at most 7 u), so no factor 2 can be promised for them:
    over 4099 elements the restatement reaches 0.72 of the m bound and 0.62 of the v bound where |wd p| >> |g|.  (The device
    contracts to fused multiply-adds and rounds less often.)
  * Adam p: inside ulp32(|p|) + 1e-4 dp, and with a factor 2 to spare once the rounding of p' itself to float32 is set aside
    (|float32(ref) - ref|, half an ulp of p', which is a whole ulp of p where the step crosses into the next binade: 0.71 of the
    bound as a whole).
"""
import numpy as np
import pytest
import torch

import loss_cases as LC
import loss_ref as LR
import training_targets_ref as TR
from oracle import loss_oracle as LO

U = LR.U
PIN = 1e-12


def pinned(got, ref, mag):
    """|got - ref| <= 1e-12 mag per element (and exact zeros where mag is 0)"""
    return LR.worst_ratio(got, ref, mag) <= PIN


ALL_TRACKING = [("plain:" + LC.case_id(c), lambda c=c: LC.plain_inputs(c)) for c in LC.PLAIN_CASES] \
    + [("graphs:" + t, lambda t=t: LC.graph_inputs(t)) for t in LC.GRAPH_CASES]
ORACLE_CASES = [a for a in ALL_TRACKING if a[0] not in ("graphs:three_shuffled", "graphs:eight_out_of_range")]
ALL_MASK = [(k, P, False) for k, P in LC.MASK_CASES] + [(3, 3136, True)]


# ------------------------------------------------------------------------------------------------ (a) the references
@pytest.mark.parametrize("label,make", ALL_TRACKING, ids=[a for a, _ in ALL_TRACKING])
def test_tracking_reference_equals_float64_torch(label, make):
    inp = make()
    ref = LC.tracking_ref(inp)
    loss, grad = LC.tracking_f32(inp, torch.float64)
    assert pinned(grad, ref[1], ref[2]) and pinned(loss, ref[0], ref[3])
    assert (ref[2] >= np.abs(ref[1])).all() and (ref[3] >= np.abs(ref[0]) * (1 - 1e-15)).all()


def test_tracking_reference_zeroes():
    """steps below first_step, ids outside [0, K), all-positive labels: loss and gradient exactly 0, magnitude 0"""
    inp = LC.graph_inputs("eight_out_of_range")
    _, grad, mag, _ = LC.tracking_ref(inp)
    out = (inp["edge_graph"] < 0) | (inp["edge_graph"] >= inp["n_graphs"])
    assert out.sum() == 10 and not grad[:, out].any() and not mag[:, out].any() and (mag[:, ~out] > 0).sum() > 0
    loss, grad, mag, lmag = LC.tracking_ref(LC.plain_inputs((16389, 3, 0, 1.0, 1.0, 3.0)))
    assert not loss.any() and not grad.any() and not mag.any() and not lmag.any()
    loss, grad, mag, lmag = LC.tracking_ref(LC.plain_inputs((257, 3, 1, 0.3, 1.0, 3.0)))
    assert loss[1] == 0 and not grad[0].any() and loss[2] > 0 and grad[1:].all()


@pytest.mark.parametrize("label,make", ORACLE_CASES, ids=[a for a, _ in ORACLE_CASES])
def test_tracking_reference_against_the_oracle(label, make):
    """oracle/loss_oracle.py (float32 torch) at the tolerances of tests/test_gpu_loss.py; the per-graph form where the ids are
    contiguous blocks inside the range (what the oracle takes)"""
    inp = make()
    ids = inp.get("edge_graph")
    assert ids is None or (np.all(np.diff(ids) >= 0) and ids.min() >= 0 and ids.max() < inp["n_graphs"])
    L, E = inp["logits"].shape
    first = inp["first_step"]
    ref = LC.tracking_ref(inp)
    if first >= L:
        assert not ref[0].any() and not ref[1].any()
        return
    z = torch.from_numpy(inp["logits"]).clone().requires_grad_(True)
    y = torch.from_numpy(inp["labels"])
    steps = [z[s].view(E, 1) for s in range(first, L)]
    if ids is None:
        want = LO.tracking_loss(steps, y, weight=inp["weight"])
    else:
        ptr = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=inp["n_graphs"]))])
        nonempty = np.diff(ptr) > 0   # (the oracle's mean over an empty slice is NaN: an empty graph contributes 0)
        want = sum(LO.tracking_loss([c.view(-1)[a:b] for c in steps], y[a:b], inp["weight"])
                   for a, b in zip(ptr[:-1][nonempty], ptr[1:][nonempty])) / inp["n_graphs"]
    want.backward()
    want = float(want.detach())
    assert abs(ref[0][0] - want) <= 1e-5 * max(1.0, abs(want))
    assert np.abs(ref[1] - z.grad.numpy()).max() <= 1e-6 * max(1.0, float(z.grad.abs().max()))


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_tracking_reference_against_the_g9_fixture(golden, tag):
    z = golden("g9_loss_metrics.npz")
    loss, grad, _, _ = LR.tracking_loss_ref(z[f"{tag}:logits"], z[f"{tag}:labels"], 0, float(z[f"{tag}:weight"]))
    ref = float(z[f"{tag}:loss"])
    assert abs(loss[0] - ref) <= 1e-5 * max(1.0, abs(ref))
    assert np.abs(grad - z[f"{tag}:grad"]).max() <= 1e-6 * max(1.0, float(np.abs(z[f"{tag}:grad"]).max()))
    # the fixture's own float32 gradient (the reference's torch run), per element under the bound the kernels are held to
    LC.check_tracking("g9 fixture " + tag, None, z[f"{tag}:grad"], z[f"{tag}:logits"], z[f"{tag}:labels"], 0, float(z[f"{tag}:weight"]))


@pytest.mark.parametrize("tag", ["g3", "g8"])
def test_tracking_reference_against_the_g16_fixture(golden, tag):
    z = golden("g16_loss_graphs.npz")
    ptr = z[f"{tag}:edge_ptr"]
    K = len(ptr) - 1
    ids = np.repeat(np.arange(K, dtype=np.int32), np.diff(ptr))
    loss, grad, _, _ = LR.tracking_loss_ref(z[f"{tag}:logits"], z[f"{tag}:labels"], 0, float(z[f"{tag}:weight"]), ids, K)
    ref = float(z[f"{tag}:loss"])
    assert abs(loss[0] - ref) <= 1e-5 * max(1.0, abs(ref))
    assert np.abs(grad - z[f"{tag}:grad"]).max() <= 1e-6 * max(1.0, float(np.abs(z[f"{tag}:grad"]).max()))
    LC.check_tracking("g16 fixture " + tag, None, z[f"{tag}:grad"], z[f"{tag}:logits"], z[f"{tag}:labels"], 0, float(z[f"{tag}:weight"]),
                      ids, K)


@pytest.mark.parametrize("k,P,graphs", ALL_MASK)
def test_mask_reference_equals_float64_torch(k, P, graphs):
    inp = LC.mask_inputs(k, P, graphs)
    ref = LC.mask_ref(inp)
    loss, grad = LC.mask_f32(inp, torch.float64)
    assert pinned(grad, ref[1], ref[2]) and pinned(loss, ref[0], ref[3])
    ok = inp["valid"] & ((inp["node_graph"] < 3) if graphs else True)
    assert not ref[1][:, ~ok].any() and not ref[2][:, ~ok].any() and ref[1][:, ok].all()
    if not graphs:   # the restatement the g21 fixture is checked with
        lv, grads = TR.mask_loss(list(inp["preds"]), inp["labels"], inp["valid"], inp["weight"])
        assert np.abs(lv - ref[0]).max() <= PIN * ref[3].max() and np.abs(np.stack(grads) - ref[1]).max() <= PIN * ref[2].max()


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_adam_reference_equals_float64_torch_adam(wd):
    """8 steps of torch.optim.Adam on float64 tensors, constructed with the float32-rounded hyper-parameters"""
    lr, b1, b2, eps, wdr = LR.adam_hyper(wd=wd, **LC.HYPER)
    n = 257
    p0 = LC.synth.normal(31, (n,)).astype(np.float64)
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdr)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    for t in range(1, 9):
        g = LC.synth.normal(40 + t, (n,)).astype(np.float64) * (1e-8 if t % 2 else 1.0)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v, m_mag, v_mag, dp = LR.adam_ref(p, g, m, v, t, wd=wd, **LC.HYPER)
        st = opt.state[tp]
        assert np.abs(tp.detach().numpy() - p).max() <= PIN * np.abs(p).max()
        assert (np.abs(st["exp_avg"].numpy() - m) <= PIN * m_mag).all() and (np.abs(st["exp_avg_sq"].numpy() - v) <= PIN * v_mag).all()


def test_the_table_holds_every_value_the_kernels_branch_on():
    for i, want in enumerate([{1, 3, 255, 256, 257, 4099, 16389}, {1, 3}, None, {0.0, "one", 0.02, 0.3, 1.0}, {1.0, 0.37}]):
        if want is not None:
            assert {c[i] for c in LC.PLAIN_CASES} == want
    assert {(c[2] == 0, c[2] == 1, c[2] == c[1]) for c in LC.PLAIN_CASES} >= {(True, False, False), (False, True, False), (False, False, True)}
    assert len(LC.PLAIN_CASES) <= 40 and {c[0] for c in LC.SLICE_CASES} == {4099, 16389}
    assert {LC.graph_inputs(t)["n_graphs"] for t in LC.GRAPH_CASES} == {1, 3, 8, 1024}
    big = LC.graph_inputs("k1024")
    sizes = np.bincount(big["edge_graph"], minlength=1024)
    assert 2500 < sizes.sum() < 4000 and sizes.min() == 0 and sizes.max() == 7
    assert {k for k, _ in LC.MASK_CASES} == {1, 3, 16} and {P for _, P in LC.MASK_CASES} == {15, 513, 2048, 2052, 3136}
    for i, want in enumerate([{1, 2, 10, 1000, 100000}, {1, 255, 256, 257, 4099}, {0.0, 1e-4}, {1.0, 1e-8}]):
        assert {c[i] for c in LC.ADAM_CASES} == want
    for c in LC.ADAM_CASES:
        assert np.abs(LC.adam_inputs(c)[1]).min() >= np.float32(1e-12)
    for c in LC.PLAIN_CASES:
        assert np.abs(LC.plain_inputs(c)["logits"]).max() <= 60.0
    assert np.abs(LC.plain_inputs(LC.PLAIN_CASES[-1])["logits"]).max() == 60.0


# ------------------------------------------------------------------------------------------------ (b) float32 fits the bounds
@pytest.mark.parametrize("label,make", ALL_TRACKING, ids=[a for a, _ in ALL_TRACKING])
def test_float32_tracking_loss_fits_half_the_bound(label, make):
    inp = make()
    loss, grad = LC.tracking_f32(inp)
    rg, rl = LC.loss_ratios(loss, grad, LC.tracking_ref(inp))
    print("%s: float32 CPU gradient %.2f u, loss %.2f u" % (label, rg / U, rl / U))
    assert 2 * rg <= LC.FIXED and 2 * rl <= LC.FIXED


@pytest.mark.parametrize("k,P,graphs", ALL_MASK)
def test_float32_mask_loss_fits_half_the_bound(k, P, graphs):
    inp = LC.mask_inputs(k, P, graphs)
    loss, grad = LC.mask_f32(inp)
    rg, rl = LC.loss_ratios(loss, grad, LC.mask_ref(inp))
    print("mask k=%d P=%d: float32 CPU gradient %.2f u, loss %.2f u" % (k, P, rg / U, rl / U))
    assert 2 * rg <= LC.FIXED and 2 * rl <= LC.FIXED


def test_float32_extreme_logits():
    """z in {-100, -88, 88, 100}: finite, and within 16 u grad_mag + 2^-126 weight / E"""
    inp = LC.extreme_inputs()
    loss, grad = LC.tracking_f32(inp)
    rl, rg, gm, _ = LC.tracking_ref(inp)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    assert (2 * np.abs(grad - rg) <= LC.FIXED * gm + 2.0 ** -126 * inp["weight"] / 8).all()


def p_rounding(ref_p):
    """what storing p' as float32 costs by itself"""
    return np.abs(ref_p.astype(np.float32).astype(np.float64) - ref_p)


@pytest.mark.parametrize("c", LC.ADAM_CASES, ids=[LC.case_id(c) for c in LC.ADAM_CASES])
def test_float32_adam_fits_the_bounds(c):
    t, n, wd, scale = c
    p, g, m, v = LC.adam_inputs(c)
    ref = LR.adam_ref(p, g, m, v, t, wd=wd, **LC.HYPER)
    got = LC.adam_f32(p, g, m, v, t, wd=wd, **LC.HYPER)
    rm, rv, rp = LC.adam_ratios(got, p, ref)
    bp = LC.adam_bounds(p, ref)[2]
    spare = LC.ratio(np.maximum(np.abs(got[0] - ref[0]) - p_rounding(ref[0]), 0.0), bp)
    print("adam %s: float32 CPU m %.2f, v %.2f, p %.2f of the bound (p without the rounding of p' itself %.3f)"
          % (LC.case_id(c), rm, rv, rp, spare))
    assert rm <= 1 and rv <= 1 and rp <= 1 and 2 * spare <= 1
    if scale == 1e-8 and wd == 0.0:   # the inputs that tell where eps sits: sqrt(v') within two decades of it
        assert np.median(np.sqrt(ref[2])) < 100 * LC.HYPER["eps"]


def test_float32_guarded_adam_fits_the_accumulated_bounds():
    offs, n, p0, grads = LC.guarded_inputs()
    ref, f32 = LC.guarded_reference(p0, grads), LC.guarded_f32(p0, grads)
    for i, ((rp, rm, rv, (bm, bv, bp)), (p, m, v)) in enumerate(zip(ref, f32)):
        r = (LC.ratio(np.abs(m - rm), bm), LC.ratio(np.abs(v - rv), bv), LC.ratio(np.abs(p - rp), bp))
        print("guarded call %d: float32 CPU m %.2f, v %.2f, p %.2f of the accumulated bound" % ((i,) + r))
        assert max(r) <= 1
    assert sum(1 - s for s in LC.GUARD_SKIPS) == 8 and LC.GUARD_SKIPS == (1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0)
