"""TrainStep(train_mask_branch=True) with ``mask_conv_grads = 'native_all'``: every layer of the mask branch native in both
directions inside the joint step (mpnhip_conv2d_backward, mpnhip_conv_transpose2d_backward, mpnhip_layer_norm_backward) -- against
the existing route (model(data) + compute_loss + backward) with the SAME selector, at the bound of
tests/test_gpu_joint_train_native_grad.py (2e-5, two routes to one gradient); the selector through a checkpoint; and two fresh steps
from one ``state_dict`` whose mask-branch parameters after Adam must be bitwise equal."""
import numpy as np
import pytest
import torch

import joint_train_common as J
from mpntrackseg_amd import capi
from mpntrackseg_amd.train import TrainStep

pytestmark = pytest.mark.gpu
BOUND = 2e-5


def fresh_all(p):
    m = J.fresh(p)
    m.mask_conv_grads = 'native_all'
    return m


def test_joint_step_with_all_native_mask_gradients():
    p = J.model_params(num_class_steps=2)
    b = J.device_batch("AB", "some")
    step = TrainStep(fresh_all(p), train_mask_branch=True)
    twin = fresh_all(p)
    capi.path_counters(reset=True)
    want_loss, _ = J.yardstick(twin, b)
    torch.cuda.synchronize()
    yard = capi.path_counters(reset=True)
    want = J.flat_like(step, twin)
    logits = step.batch(b, optimizer_step=False)
    torch.cuda.synchronize()
    mine = capi.path_counters()
    # L = 3, two class steps: per class step one LayerNorm and two transposed convolutions, forward and backward
    for c in (yard, mine):
        assert c["conv_transpose"] == 4 and c["layer_norm"] == 2 and c["conv_transpose_bwd"] == 4 and c["layer_norm_bwd"] == 2, \
            {k: c[k] for k in ("conv_transpose", "layer_norm", "conv_transpose_bwd", "layer_norm_bwd")}
        assert c["conv_bwd_gate"] == 20 and c["conv_wgrad"] == 18 and c["conv_wgrad_plain"] == 2
    assert logits.shape == (3, 400)
    got = step.bucket.flat[:step.bucket.n].double().cpu().numpy()
    assert np.isfinite(got).all()
    for name, s in J.segments(step).items():
        err = J.rel(got[s], want[s])
        print("joint step vs existing route, all-native mask gradients, %s segment: %.3e (bound %.1e)" % (name, err, BOUND))
        assert float(np.abs(want[s]).max()) > 0 and err < BOUND, (name, err)
    total = float(step.last_losses["tracking"][0]) + float(step.last_losses["segmentation"][0])
    assert abs(total - float(want_loss)) <= 1e-6 * abs(float(want_loss))
    # the gradients of the transposed convolutions and of the LayerNorm landed in the bucket's views
    mm = step.model.mask_predictor
    for q in (mm.layer_norm.weight, mm.layer_norm.bias, mm.mask_predictor.layers[0].weight, mm.mask_predictor.layers[4].bias):
        assert q.grad.data_ptr() == step.bucket.views[id(q)].data_ptr() and float(q.grad.abs().max()) > 0


def test_the_selector_survives_a_checkpoint():
    p = J.model_params()
    a = TrainStep(fresh_all(p), train_mask_branch=True)
    saved = a.state_dict()
    assert saved["mask_conv_grads"] == 'native_all' and saved["train_mask_branch"] is True
    r = TrainStep(J.fresh(p), train_mask_branch=True)
    assert r.model.mask_conv_grads == 'stock'
    r.load_state_dict(saved)
    assert r.model.mask_conv_grads == 'native_all' and r.state_dict()["mask_conv_grads"] == 'native_all'


def test_two_fresh_steps_from_one_checkpoint_agree_bit_for_bit():
    """Every mask-branch parameter after one Adam step, from two TrainStep objects restored from the same ``state_dict``.  The mask
    branch's gradients are a function of its inputs and the image count alone; its inputs include the hot path's logits, so their
    run-to-run comparison is printed first."""
    p = J.model_params(num_class_steps=2)
    b = J.device_batch("AB", "some")
    saved = TrainStep(fresh_all(p), train_mask_branch=True).state_dict()
    steps, logits = [], []
    for _ in range(2):
        s = TrainStep(J.fresh(p), train_mask_branch=True)
        s.load_state_dict(saved)
        assert s.model.mask_conv_grads == 'native_all'
        logits.append(s.batch(b).detach().clone())
        steps.append(s)
    torch.cuda.synchronize()
    print("the two steps' logits are %s" % ("bitwise equal" if torch.equal(logits[0], logits[1]) else
                                           "NOT bitwise equal: max difference %.3g" % float((logits[0] - logits[1]).abs().max())))
    names = {id(q): n for n, q in steps[0].model.named_parameters()}
    other = dict(steps[1].model.named_parameters())
    mask = TrainStep.mask_branch_parameters(steps[0].model)
    assert len(mask) == 26
    differing = [names[id(q)] for q in mask if not torch.equal(q.detach(), other[names[id(q)]].detach())]
    print("%d of %d mask-branch parameters are bitwise equal after Adam" % (len(mask) - len(differing), len(mask)))
    assert not differing, differing
    # ... and the step moved them
    before = dict(J.fresh(p).named_parameters())
    still = [names[id(q)] for q in mask if torch.equal(q.detach(), before[names[id(q)]].detach())]
    assert not still, still
