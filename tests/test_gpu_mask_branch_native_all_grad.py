"""The mask branch with ``MOTMPNet.mask_conv_grads = 'native_all'``: while gradients are recorded every layer of
``mask_predictions`` is native in both directions -- the Conv2d layers as with 'native', the two ConvTranspose2d layers through
``conv_transpose2d_native_autograd`` (mpnhip_conv_transpose2d_backward) and the LayerNorm through ``layer_norm_native_autograd``
(mpnhip_layer_norm_backward) on (feats, node_embeds) as two segments.  No stock convolution, transposed convolution or LayerNorm
module runs.

The problem, the float64 reference differentiated on the route's own ReLU decisions, the measure and the bound
max(2e-5, 4 x the stock route's error) are those of tests/test_gpu_mask_branch_native_grad.py (see its docstring); its helpers are
imported.  ``recorded_gates`` here also records the ReLU fused into the native transposed convolution, in execution order."""
import contextlib

import pytest
import torch

import test_gpu_mask_branch_native_grad as B
from mpntrackseg_amd import capi, cnn

pytestmark = pytest.mark.gpu
COUNTED = B.NEW + B.NATIVE_FWD + ("conv_transpose", "layer_norm", "conv_transpose_bwd", "layer_norm_bwd")


@contextlib.contextmanager
def recorded_gates(model, gates):
    """``B.recorded_gates`` plus the ReLUs fused into ``cnn.conv_transpose2d_native_autograd``."""
    native = cnn.conv_transpose2d_native_autograd

    def recording(segments, weight, bias, relu=False):
        y = native(segments, weight, bias, relu=relu)
        if relu:
            gates.append((y.detach() > 0).cpu())
        return y
    cnn.conv_transpose2d_native_autograd = recording
    try:
        with B.recorded_gates(model, gates):
            yield
    finally:
        cnn.conv_transpose2d_native_autograd = native


@contextlib.contextmanager
def stock_module_calls(model, calls):
    """Counts the forward calls of every nn.ConvTranspose2d and of the LayerNorm of the mask branch."""
    mods = [m for _, top in B.mask_modules(model) for m in top.modules() if isinstance(m, (torch.nn.ConvTranspose2d, torch.nn.LayerNorm))]
    assert sum(isinstance(m, torch.nn.ConvTranspose2d) for m in mods) == 2 and sum(isinstance(m, torch.nn.LayerNorm) for m in mods) == 1
    handles = [m.register_forward_hook(lambda mod, i, o: calls.append(type(mod).__name__)) for m in mods]
    try:
        yield
    finally:
        for h in handles:
            h.remove()


def run(model, x_ext, ei, logits, selector, gates=None):
    """``B.run`` with this file's ``recorded_gates``."""
    model.mask_conv_grads = selector
    model.zero_grad()
    logits.grad = None
    with recorded_gates(model, gates) if gates is not None else contextlib.nullcontext():
        preds = model.mask_predictions(x_ext, ei, logits)
    sum((p * r.to(B.dev())).sum() for p, r in zip(preds, B.loss_weights(len(preds)))).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().clone() for n, p in B.mask_parameters(model)}
    grads["logits"] = logits.grad.detach().cpu().clone()
    return [p.detach().cpu() for p in preds], grads


@pytest.fixture(scope="module")
def problem():
    """The problem, the stock and the all-native route's results and the float64 references, computed once and left unchanged."""
    model, x_ext, ei, logits = B.window_problem()
    stock_gates, all_gates = [], []
    stock = run(model, x_ext, ei, logits, 'stock', stock_gates)
    calls = []
    capi.path_counters(reset=True)
    with stock_module_calls(model, calls):
        native_all = run(model, x_ext, ei, logits, 'native_all', all_gates)
    counts = capi.path_counters(reset=True)
    assert len(stock_gates) == len(all_gates) == 2 + 2 * 2 + 2 * (1 + 3 + 3)
    ref = B.reference_gradients(model, x_ext, ei, logits, all_gates, "native_all")
    ref_stock = B.reference_gradients(model, x_ext, ei, logits, stock_gates, "stock")
    return dict(model=model, x_ext=x_ext, ei=ei, logits=logits, stock=stock, native_all=native_all, ref=ref, ref_stock=ref_stock,
                counts=counts, calls=calls)


def test_every_layer_is_native_and_no_stock_module_runs(problem):
    c = problem["counts"]
    # L = 2, two class steps: per class step one LayerNorm and two transposed convolutions, forward and backward; the 18 Conv2d
    # layers as with 'native'.  The data gradient of a transposed layer is one more 1 x 1 forward product (conv_tile); its weight
    # gradient has a kernel of its own.
    assert c["conv_transpose"] == 4 and c["layer_norm"] == 2 and c["conv_transpose_bwd"] == 4 and c["layer_norm_bwd"] == 2, \
        {k: c[k] for k in COUNTED}
    assert c["conv_bwd_gate"] == 18 and c["conv_wgrad"] == 16 and c["conv_wgrad_plain"] == 2
    assert c["conv_tile"] + c["conv_small_cout"] == 18 + (18 - 1 - 2) + 4
    assert problem["calls"] == [], problem["calls"]
    # ... while 'native' runs them: 4 transposed convolutions and 2 LayerNorms
    calls = []
    with stock_module_calls(problem["model"], calls):
        run(problem["model"], problem["x_ext"], problem["ei"], problem["logits"], 'native')
    assert sorted(calls) == ["ConvTranspose2d"] * 4 + ["LayerNorm"] * 2, calls
    preds, grads = problem["native_all"]
    assert len(preds) == 2 and all(tuple(p.shape) == (B.N, 1, 56, 56) for p in preds)
    assert len(grads) == 26 + 1
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name


def test_native_all_gradients_against_float64(problem):
    ref_preds, ref = problem["ref"]
    ref_stock = problem["ref_stock"][1]
    for s, (a, b) in enumerate(zip(problem["native_all"][0], ref_preds)):
        print("predictions against float64, class step %d: native_all %.3g, stock %.3g" % (
            s, B.nerr(a.numpy(), b.numpy()), B.nerr(problem["stock"][0][s].numpy(), b.numpy())))
    failures = []
    for name in ref:
        e_native = B.nerr(problem["native_all"][1][name].numpy(), ref[name].numpy())
        e_stock = B.nerr(problem["stock"][1][name].numpy(), ref_stock[name].numpy())
        bound = max(2e-5, 4 * e_stock)
        print("%-55s native_all %.3e   stock %.3e   (bound %.3e)" % (name, e_native, e_stock, bound))
        if not e_native < bound:
            failures.append((name, e_native, bound))
    assert len(ref) == 27 and not failures, failures


def test_all_27_gradients_repeat_bit_for_bit(problem):
    """A second pass in the same process: every parameter gradient of the branch -- the two transposed convolutions and the
    LayerNorm affine included -- and ``logits.grad`` are bitwise the first's."""
    again = run(problem["model"], problem["x_ext"], problem["ei"], problem["logits"], 'native_all')[1]
    first = problem["native_all"][1]
    assert len(first) == 27 and set(first) == set(again)
    assert any("layer_norm.weight" in n for n in first) and sum("mask_predictor.mask_predictor" in n for n in first) == 8
    differing = [n for n in first if not torch.equal(first[n], again[n])]
    print("%d of %d gradients repeat bit for bit" % (len(first) - len(differing), len(first)))
    assert not differing, differing


def test_predictions_are_bitwise_the_native_inference_route(problem):
    """Both are the same forward kernels on the same inputs."""
    model = problem["model"]
    model.mask_convs = 'native'
    try:
        with torch.no_grad():
            capi.path_counters(reset=True)
            preds = model.mask_predictions(problem["x_ext"], problem["ei"], problem["logits"].detach())
            c = capi.path_counters()
    finally:
        model.mask_convs = 'stock'
    assert c["conv_transpose"] == 4 and c["layer_norm"] == 2
    for a, b in zip(preds, problem["native_all"][0]):
        assert torch.equal(a.cpu(), b)


def check_fallback(model, x_ext, ei, logits):
    model.mask_conv_grads = 'native_all'
    assert not all(m.native_supported() for m in model._mask_modules())
    capi.path_counters(reset=True)
    preds = model.mask_predictions(x_ext, ei, logits)
    sum(p.sum() for p in preds).backward()
    torch.cuda.synchronize()
    c = capi.path_counters()
    assert not any(c[k] for k in COUNTED), {k: c[k] for k in COUNTED}
    for name, p in B.mask_parameters(model):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert logits.grad is not None


def test_a_5x5_stack_takes_the_stock_path():
    model, x_ext, ei, logits = B.window_problem()
    old = model.mask_predictor.mask_head.layers[0]
    wide = torch.nn.Conv2d(64, 64, kernel_size=5, padding=2).to(B.dev())
    with torch.no_grad():
        wide.weight.zero_()
        wide.weight[:, :, 1:4, 1:4] = old.weight
        wide.bias.copy_(old.bias)
    model.mask_predictor.mask_head.layers[0] = wide
    check_fallback(model, x_ext, ei, logits)


def test_training_dropout_takes_the_stock_path():
    model, x_ext, ei, logits = B.window_problem()
    model.MPAttentionNet.node_model.layers.append(torch.nn.Dropout2d(p=0.4))
    assert model.training
    check_fallback(model, x_ext, ei, logits)
    # in eval mode the Dropout is off and the stack is covered again
    model.eval()
    capi.path_counters(reset=True)
    sum(p.sum() for p in model.mask_predictions(x_ext, ei, logits)).backward()
    c = capi.path_counters()
    assert c["conv_transpose_bwd"] == 4 and c["layer_norm_bwd"] == 2
