"""TrainStep(train_mask_branch=True): the reference's joint step (pl_module.py:88-135) -- native forward / backward for the hot path,
the mask branch under autograd on the native logits, both loss terms from the native loss kernels, ONE flat bucket and ONE Adam
launch -- against the existing route (model(data) + compute_loss + backward + torch.optim.Adam) on a two-graph batch; and the
pieces around it: evaluate(), EpochLog, state_dict() / load_state_dict()."""
import numpy as np
import pytest
import torch

import joint_train_common as J
import step_metrics_ref as R
from mpntrackseg_amd import capi
from mpntrackseg_amd.loss import mask_loss_and_grad, step_metric_counts
from mpntrackseg_amd.train import EpochLog, TrainStep

pytestmark = pytest.mark.gpu

TENSORS = ("x", "edge_index", "edge_attr")
MASK_KW = ("x_ext", "mask_labels", "mask_gt_ixs", "node_graph")


def call(step, b, **kw):
    """The explicit call (step.batch(b) is the same thing)."""
    return step(b["x"], b["edge_index"], b["edge_attr"], labels=b["edge_labels"], edge_graph=b["edge_graph"], n_graphs=b["n_graphs"],
                **{k: b[k] for k in MASK_KW}, **kw)


_bound = {}


def gradient_bound(p, b, key):
    """2e-5 (the project's bound for two routes to one gradient, tests/dist_train_check.py) unless the yardstick's own run-to-run
    spread exceeds 5e-6 (MIOpen's backward may use atomics): then four times that spread.  Returns (bound, yardstick flat grads
    of the second run as a function of a step, loss)."""
    if key not in _bound:
        twin = J.fresh(p)
        probe = TrainStep(J.fresh(p), train_mask_branch=True)     # (layout only)
        J.yardstick(twin, b)
        g1 = J.flat_like(probe, twin)
        loss, out = J.yardstick(twin, b)
        g2 = J.flat_like(probe, twin)
        spread = max(J.rel(g1[s], g2[s]) for s in J.segments(probe).values())
        bound = 2e-5 if spread <= 5e-6 else 4 * spread
        print("yardstick run-to-run spread %.3e -> bound %.3e (%s)" % (spread, bound, key))
        _bound[key] = (bound, g2, float(loss), [m.detach() for m in out["mask_predictions"]])
    return _bound[key]


@pytest.mark.parametrize("b_rows", ["some", "none"])
def test_joint_gradients_match_the_existing_route(b_rows):
    p = J.model_params(num_class_steps=2)
    b = J.device_batch("AB", b_rows)
    bound, want, want_loss, masks = gradient_bound(p, b, ("k2", b_rows))
    step = TrainStep(J.fresh(p), train_mask_branch=True)
    logits = step.batch(b, optimizer_step=False)
    torch.cuda.synchronize()
    assert logits.shape == (3, 400) and not logits.requires_grad
    got = step.bucket.flat[:step.bucket.n].double().cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(step.bucket.flat.cpu().numpy()).all()
    for name, s in J.segments(step).items():
        err = J.rel(got[s], want[s])
        print("joint vs yardstick, %s segment (%s): %.3e (bound %.3e)" % (name, b_rows, err, bound))
        assert err < bound, (name, err, bound)
    lt, ls = step.last_losses["tracking"], step.last_losses["segmentation"]
    assert lt.shape == (4,) and ls.shape == (3,) and lt.is_cuda and ls.is_cuda and step.last_loss is lt
    total = float(lt[0]) + float(ls[0])
    assert abs(total - want_loss) <= 1e-6 * abs(want_loss), (total, want_loss)
    if b_rows == "none":
        # graph B has no valid row: its segmentation term is exactly 0, the batch's is graph A's divided by the two graphs
        la, _ = mask_loss_and_grad([m[:J.N_A] for m in masks], b["mask_labels"][:J.N_A], b["mask_gt_ixs"][:J.N_A], 1.0)
        assert abs(float(ls[0]) - float(la[0]) / 2) <= 1e-6 * float(la[0]) / 2, (float(ls[0]), float(la[0]))
        assert float(ls[0]) > 0


def test_the_mask_loss_reaches_the_early_logits():
    """num_class_steps = 1: the tracking term seeds the last step's logits only; the mask loss also pulls on the two earlier steps'
    (through their attention aggregations), so the hot-path gradient differs from a tracking-only step's -- and is still the
    existing route's."""
    p = J.model_params(num_class_steps=1)
    b = J.device_batch("AB", "some")
    bound, want, _, _ = gradient_bound(p, b, ("k1", "some"))
    step = TrainStep(J.fresh(p), train_mask_branch=True)
    call(step, b, optimizer_step=False)
    plain = TrainStep(J.fresh(p))
    plain(*(b[k] for k in TENSORS), labels=b["edge_labels"], edge_graph=b["edge_graph"], n_graphs=2, optimizer_step=False)
    torch.cuda.synchronize()
    got = step.bucket.flat[:step.bucket.n].double().cpu().numpy()
    hot = J.segments(step)["hot"]
    only_tracking = plain.bucket.flat[:plain.bucket.n].double().cpu().numpy()
    assert only_tracking.shape == got[hot].shape
    diff = J.rel(got[hot], only_tracking)
    print("hot-path gradient, joint against tracking-only: %.3e (bound %.3e)" % (diff, bound))
    assert diff > bound          # another gradient: further apart than two routes to ONE gradient may be
    for name, s in J.segments(step).items():
        assert J.rel(got[s], want[s]) < bound, name


def test_one_adam_launch_moves_every_parameter_like_torch_adam():
    p = J.model_params()
    b = J.device_batch("AB", "some")
    step = TrainStep(J.fresh(p), train_mask_branch=True, lr=1e-3, weight_decay=1e-4)
    start = [q.detach().clone() for q in step.bucket.params]
    ptrs = [q.grad.data_ptr() for q in step.bucket.params]
    call(step, b)
    torch.cuda.synchronize()
    ref = [torch.nn.Parameter(s.clone()) for s in start]
    for r, q in zip(ref, step.bucket.params):
        r.grad = step.bucket.views[id(q)].detach().clone()          # the bucket's own gradients
    torch.optim.Adam(ref, lr=1e-3, weight_decay=1e-4).step()
    mask_ids = set(id(q) for q in TrainStep.mask_branch_parameters(step.model))
    assert len(mask_ids) == 26 and step.opt.t == 1
    for r, q, s, ptr in zip(ref, step.bucket.params, start, ptrs):
        assert float((r.detach() - q.detach()).abs().max()) <= 2e-6 * max(1.0, float(r.detach().abs().max()))
        if id(q) in mask_ids:
            assert not torch.equal(q.detach(), s)                   # every mask-branch tensor has moved
        assert q.grad.data_ptr() == ptr == step.bucket.views[id(q)].data_ptr()
        assert q.data_ptr() == step.bucket.flat_params.data_ptr() + 4 * step.bucket.offsets[id(q)]


def test_default_step_keeps_its_layout_and_leaves_the_mask_branch_alone():
    p = J.model_params()
    b = J.device_batch("AB", "some")
    model = J.fresh(p)
    step = TrainStep(model)
    offs, n = [], 0
    for q in model.hot_path_parameters():
        offs.append(n)
        n += (q.numel() + 3) // 4 * 4
    assert step.bucket.n == n and step.mask_elems == 0 and not step.train_mask_branch
    assert [step.bucket.offsets[id(q)] for q in model.hot_path_parameters()] == offs and len(step.bucket.params) == len(offs)
    mask = TrainStep.mask_branch_parameters(model)
    before = [q.detach().clone() for q in mask]
    step(*(b[k] for k in TENSORS), labels=b["edge_labels"], edge_graph=b["edge_graph"], n_graphs=2)
    torch.cuda.synchronize()
    assert all(torch.equal(q.detach(), s) for q, s in zip(mask, before)) and all(q.grad is None for q in mask)
    assert step.last_losses["segmentation"] is None and step.last_losses["tracking"] is step.last_loss
    # the joint layout: [mask | encoder | message passing + classifier | spare], every parameter on a 16-byte boundary
    joint = TrainStep(J.fresh(p), train_mask_branch=True)
    assert joint.bucket.n == joint.mask_elems + n and joint.enc_elems == joint.mask_elems + step.enc_elems
    assert [joint.bucket.offsets[id(q)] - joint.mask_elems for q in joint.model.hot_path_parameters()] == offs
    assert all(o % 4 == 0 for o in joint.bucket.offsets.values()) and joint.bucket.flat.numel() == joint.bucket.n + 4
    sd = list(joint.model.state_dict())
    names = joint._param_names()[:26]
    assert names == [k for k in sd if k.startswith(("node_ext_encoder.", "mask_predictor.", "MPAttentionNet."))]


def test_refusals_enqueue_nothing():
    p = J.model_params()
    b = J.device_batch("AB", "some")
    step = TrainStep(J.fresh(p), train_mask_branch=True)
    before = step.bucket.flat_params.clone()
    for missing in ("x_ext", "mask_labels", "mask_gt_ixs"):
        kw = {k: (None if k == missing else b[k]) for k in MASK_KW}
        with pytest.raises(capi.MpnhipError, match=missing):
            step(*(b[k] for k in TENSORS), labels=b["edge_labels"], edge_graph=b["edge_graph"], n_graphs=2, **kw)
    torch.cuda.synchronize()
    assert torch.equal(before, step.bucket.flat_params) and step.opt.t == 0 and int(step.bucket.flat.abs().sum()) == 0
    # no mask branch in the model
    p0 = J.model_params(mask=False)
    m0 = J.fresh(p0)
    w0 = [q.data_ptr() for q in m0.parameters()]
    with pytest.raises(capi.MpnhipError, match="mask branch"):
        TrainStep(m0, train_mask_branch=True)
    assert [q.data_ptr() for q in m0.parameters()] == w0                 # (no bucket was built: the storage did not move)
    # BatchNorm2d in a mask module and two ranks: refused at construction (one rank is allowed)
    pb = J.model_params()
    pb["node_ext_model_feats_dict"] = dict(pb["node_ext_model_feats_dict"], use_batchnorm=True)
    from mpntrackseg_amd.mpn import MOTMPNet
    mb = MOTMPNet(pb).to(J.DEV).train()
    wb = [q.detach().clone() for q in mb.parameters()]
    pb_ptrs = [q.data_ptr() for q in mb.parameters()]
    with pytest.raises(capi.MpnhipError, match="BatchNorm"):
        TrainStep(mb, world_size=2, train_mask_branch=True)
    assert [q.data_ptr() for q in mb.parameters()] == pb_ptrs and all(torch.equal(q.detach(), s) for q, s in zip(mb.parameters(), wb))
    TrainStep(mb, world_size=1, train_mask_branch=True)


def test_evaluate_and_epoch_log():
    p = J.model_params()
    b = J.device_batch("AB", "some")
    step = TrainStep(J.fresh(p), train_mask_branch=True)
    call(step, b, optimizer_step=False)                                   # (gradients in the bucket, weights unchanged)
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in step.last_losses.items()}
    state = [t.clone() for t in (step.bucket.flat_params, step.bucket.flat, step.opt.exp_avg, step.opt.exp_avg_sq)]
    log = EpochLog(capacity_steps=3, max_graphs=2)
    ev = step.evaluate(*(b[k] for k in TENSORS), b["edge_labels"], edge_graph=b["edge_graph"], n_graphs=2,
                       **{k: b[k] for k in MASK_KW}, log=log)
    torch.cuda.synchronize()
    for t, s in zip((step.bucket.flat_params, step.bucket.flat, step.opt.exp_avg, step.opt.exp_avg_sq), state):
        assert torch.equal(t, s)
    assert step.opt.t == 0 and all(q.grad.data_ptr() == step.bucket.views[id(q)].data_ptr() for q in step.bucket.params)
    # two fp32 forwards of the same weights (the training forward keeps activations, this one does not): the loss is a mean of
    # per-edge / per-pixel terms that agree to a few ulp -- 1e-5 relative, the bound tests/test_gpu_loss.py uses for loss values
    for k in ("tracking", "segmentation"):
        assert ev["losses"][k].is_cuda and ev["losses"][k].shape == want[k].shape
        assert float((ev["losses"][k] - want[k]).abs().max()) <= 1e-5 * float(want[k].abs().max()), k
    counts = step_metric_counts(ev["logits"][-1], b["edge_labels"], b["edge_index"], b["x"].shape[0], edge_graph=b["edge_graph"],
                                node_graph=b["node_graph"], n_graphs=2)
    assert ev["counts"].dtype == torch.int32 and ev["counts"].shape == (2, 8) and torch.equal(ev["counts"], counts)
    hb = J.host_batch("AB", "some")
    ref_counts = R.graph_counts(ev["logits"][-1].cpu().numpy(), hb["edge_labels"], hb["edge_index"], 68, hb["edge_graph"], hb["node_graph"], 2)
    assert np.array_equal(counts.cpu().numpy(), ref_counts)
    # the epoch: that step (2 graphs), a training step with log= (2 graphs), and a one-graph step appended by hand whose row has
    # no flow constraint (constr_out = constr_in = 0): its constr_sr is NaN and must be skipped by the epoch mean
    call(step, b, optimizer_step=False, log=log)
    empty = torch.zeros((1, 8), dtype=torch.int32, device=J.DEV)
    empty[0, :4] = torch.tensor([1, 0, 2, 1], dtype=torch.int32)
    l3 = {"tracking": torch.tensor([0.75, 0.75], device=J.DEV), "segmentation": None}
    log.append(l3, empty, 1)
    with pytest.raises(capi.MpnhipError):
        log.append(l3, empty, 1)                                          # capacity
    torch.cuda.synchronize()
    s = log.summary()
    c2 = log.counts[1].cpu().numpy()
    steps = [(float(ev["losses"]["tracking"][0]), float(ev["losses"]["segmentation"][0]), ref_counts),
             (float(step.last_losses["tracking"][0]), float(step.last_losses["segmentation"][0]), c2),
             (0.75, 0.0, empty.cpu().numpy())]
    ref = R.epoch_mean(steps)
    assert np.isnan(R.metrics(empty.cpu().numpy())["constr_sr"][0])
    assert sorted(s) == sorted(ref) == sorted(["loss", "loss_tracking", "loss_segmentation", "accuracy", "recall", "precision", "constr_sr"])
    for k in ref:
        assert abs(s[k] - ref[k]) <= 1e-6 * max(1.0, abs(ref[k])), (k, s[k], ref[k])


def run_steps(step, b, n):
    for _ in range(n):
        step(*(b[k] for k in TENSORS), labels=b["edge_labels"], edge_graph=b["edge_graph"], n_graphs=2)


def test_resume_is_bitwise_the_uninterrupted_run():
    p = J.model_params()
    b = J.device_batch("AB", "some")
    a = TrainStep(J.fresh(p), lr=1e-3, weight_decay=1e-4)
    run_steps(a, b, 2)
    saved = a.state_dict()
    run_steps(a, b, 2)
    W0 = {k: v * 0.5 for k, v in J.weights(p).items()}                    # a fresh model with OTHER weights
    r = TrainStep(J.fresh(p, W0), lr=5e-2)
    r.load_state_dict(saved)
    assert r.opt.lr == 1e-3 and r.opt.weight_decay == 1e-4 and r.opt.t == 2
    run_steps(r, b, 2)
    torch.cuda.synchronize()
    assert torch.equal(a.bucket.flat_params, r.bucket.flat_params)
    assert torch.equal(a.opt.exp_avg, r.opt.exp_avg) and torch.equal(a.opt.exp_avg_sq, r.opt.exp_avg_sq)
    assert a.opt.applied_steps == r.opt.applied_steps == 4
    for (ka, va), (kr, vr) in zip(a.model.state_dict().items(), r.model.state_dict().items()):
        assert ka == kr and torch.equal(va, vr), ka


def test_joint_checkpoints_and_their_refusals():
    p = J.model_params()
    b = J.device_batch("AB", "some")
    a = TrainStep(J.fresh(p), train_mask_branch=True, lr=1e-3)
    call(a, b)
    saved = a.state_dict()
    assert saved["train_mask_branch"] is True and saved["t"] == 1 and saved["skipped"].is_cuda
    assert sorted(saved["exp_avg"]) == sorted(a._param_names()) and len(saved["exp_avg"]) == len(a.bucket.params)
    W0 = {k: v * 0.5 for k, v in J.weights(p).items()}
    epoch = capi._weights_epoch[0]
    r = TrainStep(J.fresh(p, W0), train_mask_branch=True)
    r.load_state_dict(saved)
    torch.cuda.synchronize()
    assert capi._weights_epoch[0] > epoch
    assert torch.equal(a.bucket.flat_params, r.bucket.flat_params)
    assert torch.equal(a.opt.exp_avg, r.opt.exp_avg) and torch.equal(a.opt.exp_avg_sq, r.opt.exp_avg_sq) and r.opt.t == 1
    assert all(q.data_ptr() == r.bucket.flat_params.data_ptr() + 4 * r.bucket.offsets[id(q)] for q in r.bucket.params)
    # a hot-path-only checkpoint into a joint step: mask moments zero, hot-path moments the checkpoint's
    h = TrainStep(J.fresh(p), lr=1e-3)
    run_steps(h, b, 1)
    hs = h.state_dict()
    assert hs["train_mask_branch"] is False and len(hs["exp_avg"]) == len(h.bucket.params)
    j = TrainStep(J.fresh(p, W0), train_mask_branch=True)
    j.opt.exp_avg.fill_(3.0)
    j.load_state_dict(hs)
    torch.cuda.synchronize()
    m = j.mask_elems
    assert float(j.opt.exp_avg[:m].abs().max()) == 0 and float(j.opt.exp_avg_sq[:m].abs().max()) == 0
    assert torch.equal(j.opt.exp_avg[m:j.bucket.n], h.opt.exp_avg[:h.bucket.n]) and torch.equal(j.bucket.flat_params[m:j.bucket.n], h.bucket.flat_params[:h.bucket.n])
    # ... and a joint checkpoint into a hot-path-only step: the mask moments are ignored
    h2 = TrainStep(J.fresh(p, W0))
    h2.load_state_dict(saved)
    torch.cuda.synchronize()
    assert torch.equal(h2.opt.exp_avg[:h2.bucket.n], a.opt.exp_avg[a.mask_elems:a.bucket.n])
    # a wrong-shaped encoder weight, a missing hot-path moment: refused by name, nothing written
    key = "encoder.node_model.fc_layers.0.weight"
    broken = dict(saved, model=dict(saved["model"]))
    broken["model"][key] = saved["model"][key][:, :-1].clone()
    before = h2.bucket.flat_params.clone()
    with pytest.raises(capi.MpnhipError, match=key.replace(".", r"\.")):
        h2.load_state_dict(broken)
    gone = dict(saved, exp_avg={k: v for k, v in saved["exp_avg"].items() if k != "classifier.edge_model.fc_layers.0.bias"})
    with pytest.raises(capi.MpnhipError, match=r"classifier\.edge_model\.fc_layers\.0\.bias"):
        h2.load_state_dict(gone)
    torch.cuda.synchronize()
    assert torch.equal(before, h2.bucket.flat_params)
