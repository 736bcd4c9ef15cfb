"""TrainStep(train_mask_branch=True) with ``mask_conv_grads = 'native'``: the mask branch's Conv2d layers through the native forward
and mpnhip_conv2d_backward (csrc/conv_backward.hip) inside the joint step -- against the existing route (model(data) +
compute_loss + backward) with the SAME selector, in one process: both sides run the same deterministic convolution kernels, so the
flat gradient's mask and hot-path segments agree within the project's 2e-5 for two routes to one gradient.  The bucket views must
still receive the gradients in place, and the selector must survive a checkpoint."""
import numpy as np
import pytest
import torch

import joint_train_common as J
from mpntrackseg_amd import capi
from mpntrackseg_amd.train import TrainStep

pytestmark = pytest.mark.gpu
BOUND = 2e-5
NEW = ("conv_bwd_gate", "conv_wgrad", "conv_wgrad_plain")


def fresh_native(p):
    m = J.fresh(p)
    m.mask_conv_grads = 'native'
    return m


def test_joint_step_with_native_mask_gradients():
    p = J.model_params(num_class_steps=2)
    b = J.device_batch("AB", "some")
    step = TrainStep(fresh_native(p), train_mask_branch=True)
    twin = fresh_native(p)
    capi.path_counters(reset=True)
    want_loss, _ = J.yardstick(twin, b)
    torch.cuda.synchronize()
    yard = capi.path_counters(reset=True)
    want = J.flat_like(step, twin)
    conv_w = step.model.mask_predictor.mask_head.layers[0].weight
    ptr = conv_w.grad.data_ptr()
    logits = step.batch(b, optimizer_step=False)
    torch.cuda.synchronize()
    mine = capi.path_counters()
    # L = 3, two class steps: 2 + 3 x 2 + 2 x (1 + 3 + 2) = 20 Conv2d layers, 2 of them (the last 1 x 1, 64 -> 1) small-cout
    for c in (yard, mine):
        assert c["conv_wgrad"] == 18 and c["conv_wgrad_plain"] == 2 and c["conv_bwd_gate"] == 20, {k: c[k] for k in NEW}
    assert logits.shape == (3, 400)
    got = step.bucket.flat[:step.bucket.n].double().cpu().numpy()
    assert np.isfinite(got).all()
    for name, s in J.segments(step).items():
        err = J.rel(got[s], want[s])
        print("joint step vs existing route, native mask gradients, %s segment: %.3e (bound %.1e)" % (name, err, BOUND))
        assert float(np.abs(want[s]).max()) > 0 and err < BOUND, (name, err)
    total = float(step.last_losses["tracking"][0]) + float(step.last_losses["segmentation"][0])
    assert abs(total - float(want_loss)) <= 1e-6 * abs(float(want_loss))
    # p.grad of a mask-branch convolution weight is still the bucket's view, and holds what the flat buffer holds
    assert conv_w.grad.data_ptr() == ptr == step.bucket.views[id(conv_w)].data_ptr()
    o = step.bucket.offsets[id(conv_w)]
    assert ptr == step.bucket.flat.data_ptr() + 4 * o
    assert torch.equal(conv_w.grad.reshape(-1), step.bucket.flat[o:o + conv_w.numel()]) and float(conv_w.grad.abs().max()) > 0
    for q in step.bucket.params:
        assert q.grad.data_ptr() == step.bucket.views[id(q)].data_ptr()


def test_the_selector_survives_a_checkpoint():
    p = J.model_params()
    a = TrainStep(fresh_native(p), train_mask_branch=True)
    saved = a.state_dict()
    assert saved["mask_conv_grads"] == 'native' and saved["train_mask_branch"] is True
    r = TrainStep(J.fresh(p), train_mask_branch=True)
    assert r.model.mask_conv_grads == 'stock' and r.state_dict()["mask_conv_grads"] == 'stock'
    r.load_state_dict(saved)
    assert r.model.mask_conv_grads == 'native'
    # a checkpoint written before the selector existed leaves the model's as it is
    old = {k: v for k, v in saved.items() if k != "mask_conv_grads"}
    r.model.mask_conv_grads = 'stock'
    r.load_state_dict(old)
    assert r.model.mask_conv_grads == 'stock'
