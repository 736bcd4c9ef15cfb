"""The mask branch with ``MOTMPNet.mask_conv_grads = 'native'``: while gradients are recorded every Conv2d of ``mask_predictions``
runs the native forward under autograd with mpnhip_conv2d_backward (csrc/conv_backward.hip) as its backward; ConvTranspose2d,
LayerNorm and the concatenation in front of it stay stock modules.

Accuracy: the model is deep-copied to the CPU in float64 and ``mask_predictions`` restated in plain torch with the oracle's
attention aggregation (oracle/attention_oracle.py); the loss is sum_i sum(pred_i * r_i) with fixed synth.normal tensors r_i.  Error
measure: max |got - ref64| / max |ref64| per parameter and for ``logits.grad``.  Bound for the native route:
max(2e-5, 4 x the stock route's error against the same reference in the same process) -- 2e-5 is the project's gradient bound
(DESIGN.md section 4h); the stock term is there because MIOpen's own distance from float64 depends on the algorithm it picked.

The reference is differentiated on the branch the route under test took: the ~5 million ReLU inputs of this problem include a few
within float32 rounding of zero, where a route's forward (either route's) may land on the other side than float64 does, and one
such element moves a convolution's weight gradient by 1e-4 .. 1e-3 of its largest entry -- the gradient of a ReLU network is not
continuous there, so the comparison would measure the coin, not the kernels.  Every route's post-ReLU signs are recorded during
its forward and the float64 copy multiplies by those 0 / 1 masks in place of its ReLUs (the hot-path parity tests read the
forward's decisions the same way); the number of elements where the mask differs from float64's own is printed."""
import contextlib
import copy

import numpy as np
import pytest
import torch

from mpntrackseg_amd import capi, cnn, synth
from mpntrackseg_amd.mpn import MOTMPNet
from oracle import attention_oracle as AO

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
NEW = ("conv_bwd_gate", "conv_wgrad", "conv_wgrad_plain")
NATIVE_FWD = ("conv_tile", "conv_small_cout")
N, E = 7, 24


def nerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


def make_model(L, num_class_steps=2, reattach=True, gain=0.6):
    params = synth.model_params(32, L, "sum", num_class_steps=num_class_steps, node_in_dim=64)
    params.update(synth.MASK_PARAMS)
    params["reattach_initial_nodes"] = reattach
    model = MOTMPNet(params)
    W = synth.make_weights(params, seed=7, gain=gain)
    W.update(synth.make_mask_weights(seed=17))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    return model.to(dev()).train()


def window_problem(L=2):
    """The 7-node, 24-edge problem of tests/test_gpu_mask_branch_native.py, in training mode; ``logits`` is a leaf that wants a
    gradient, ``x_ext`` wants none (as in the joint training step)."""
    model = make_model(L)
    g = synth.make_graph(N, E, T=4, seed=6, node_in_dim=64)
    x = torch.from_numpy(g["x"]).to(dev())
    ei = torch.from_numpy(g["edge_index"]).to(dev())
    ea = torch.from_numpy(g["edge_attr"]).to(dev())
    x_ext = torch.from_numpy(synth.normal(8, (N, 256, 14, 14), stream=1, std=0.5)).to(dev())
    with torch.no_grad():
        logits = model.hot_path(x, ei, ea)
    return model, x_ext, ei, logits.detach().clone().requires_grad_(True)


def loss_weights(n_preds):
    return [torch.from_numpy(synth.normal(9, (N, 1, 56, 56), stream=20 + i)) for i in range(n_preds)]


def mask_modules(model):
    return (("node_ext_encoder", model.node_ext_encoder), ("MPAttentionNet.node_model", model.MPAttentionNet.node_model),
            ("mask_predictor", model.mask_predictor))


def mask_parameters(model):
    return [(top + "." + n, p) for top, m in mask_modules(model) for n, p in m.named_parameters()]


def new_counts():
    c = capi.path_counters()
    return {k: c[k] for k in NEW}


@contextlib.contextmanager
def recorded_gates(model, gates):
    """Appends the 0 / 1 mask (output > 0) of every ReLU the mask branch evaluates to ``gates``, in execution order: the stock
    nn.ReLU modules through forward hooks, the ReLUs fused into the native convolutions through ``cnn.conv2d_native_autograd``."""
    handles = [mod.register_forward_hook(lambda m, i, o: gates.append((o.detach() > 0).cpu()))
               for _, top in mask_modules(model) for mod in top.modules() if isinstance(mod, torch.nn.ReLU)]
    native = cnn.conv2d_native_autograd

    def recording(segments, weight, bias, relu=False):
        y = native(segments, weight, bias, relu=relu)
        if relu:
            gates.append((y.detach() > 0).cpu())
        return y
    cnn.conv2d_native_autograd = recording
    try:
        yield
    finally:
        cnn.conv2d_native_autograd = native
        for h in handles:
            h.remove()


def run(model, x_ext, ei, logits, selector, gates=None):
    """forward + backward of the weighted loss with ``mask_conv_grads = selector``: (predictions, {name: gradient}) on the host;
    ``gates``: a list that receives the forward's ReLU masks."""
    model.mask_conv_grads = selector
    model.zero_grad()
    logits.grad = None
    with recorded_gates(model, gates) if gates is not None else contextlib.nullcontext():
        preds = model.mask_predictions(x_ext, ei, logits)
    sum((p * r.to(dev())).sum() for p, r in zip(preds, loss_weights(len(preds)))).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().clone() for n, p in mask_parameters(model)}
    grads["logits"] = logits.grad.detach().cpu().clone()
    return [p.detach().cpu() for p in preds], grads


class Gate(torch.nn.Module):
    """Stands in for a ReLU of the float64 copy: multiplies by the next recorded mask and counts where float64 disagrees with it."""

    def __init__(self, queue, stats):
        super().__init__()
        self.queue, self.stats = queue, stats

    def forward(self, x):
        g = self.queue.pop(0)
        self.stats[0] += int(((x.detach() > 0) != g).sum())
        self.stats[1] += g.numel()
        return x * g.to(x.dtype)


def reference_gradients(model, x_ext, ei, logits, gates, label):
    """``mask_predictions`` (mpn.py:356,373-392) on a float64 CPU copy of the model, the attention aggregation from the oracle, the
    ReLU decisions those of ``gates`` (see the module docstring)."""
    m = copy.deepcopy(model).cpu().double()
    queue, stats = list(gates), [0, 0]
    for _, top in mask_modules(m):
        for seq in [s for s in top.modules() if isinstance(s, torch.nn.Sequential)]:
            for i, mod in enumerate(seq):
                if isinstance(mod, torch.nn.ReLU):
                    seq[i] = Gate(queue, stats)
    x_ext, ei = x_ext.detach().cpu().double(), ei.cpu()
    lg = logits.detach().cpu().double().requires_grad_(True)
    L, k = int(m.num_enc_steps), int(m.num_class_steps)
    latent = m.node_ext_encoder(x_ext)
    initial = latent
    preds = []
    for step in range(1, L + 1):
        if m.reattach_initial_nodes:
            latent = torch.cat((initial, latent), dim=1)
        flow_in, flow_out, _ = AO.attention_aggregate(latent, ei, lg[step - 1])
        latent = m.MPAttentionNet.node_model(torch.cat((latent, flow_in, flow_out), dim=1))
        if step >= L - k + 1:
            preds.append(m.mask_predictor(x_ext, latent))
    assert not queue
    print("%s route: %d of %d ReLU decisions differ from float64's own" % (label, stats[0], stats[1]))
    sum((p * r.double()).sum() for p, r in zip(preds, loss_weights(len(preds)))).backward()
    grads = {n: p.grad.detach().clone() for n, p in mask_parameters(m)}
    grads["logits"] = lg.grad.detach().clone()
    return [p.detach() for p in preds], grads


@pytest.fixture(scope="module")
def problem():
    """The problem, the stock and the native route's results and the float64 reference, computed once and left unchanged."""
    model, x_ext, ei, logits = window_problem()
    stock_gates, native_gates = [], []
    capi.path_counters(reset=True)
    stock = run(model, x_ext, ei, logits, 'stock', stock_gates)
    stock_counts = capi.path_counters(reset=True)
    native = run(model, x_ext, ei, logits, 'native', native_gates)
    native_counts = capi.path_counters(reset=True)
    assert len(stock_gates) == len(native_gates) == 2 + 2 * 2 + 2 * (1 + 3 + 3)
    ref = reference_gradients(model, x_ext, ei, logits, native_gates, "native")
    ref_stock = reference_gradients(model, x_ext, ei, logits, stock_gates, "stock")
    return dict(model=model, x_ext=x_ext, ei=ei, logits=logits, stock=stock, native=native, ref=ref, ref_stock=ref_stock,
                stock_counts=stock_counts, native_counts=native_counts)


def test_native_gradient_route_runs_and_reaches_everything(problem):
    sc, nc = problem["stock_counts"], problem["native_counts"]
    assert not any(sc[k] for k in NEW + NATIVE_FWD), sc
    # L = 2, two class steps: 2 encoder + 2 x 2 node-model layers, per class step 1 feature-encoder + 3 mask-head + 2 predictor
    # Conv2d layers (the last of them 64 -> 1: the small-cout kernels); the data gradient skips the two layers that read x_ext
    assert nc["conv_bwd_gate"] == 18 and nc["conv_wgrad"] == 16 and nc["conv_wgrad_plain"] == 2, {k: nc[k] for k in NEW}
    assert nc["conv_tile"] + nc["conv_small_cout"] == 18 + (18 - 1 - 2) and nc["conv_transpose"] == 0 and nc["layer_norm"] == 0
    preds, grads = problem["native"]
    assert len(preds) == 2 and all(tuple(p.shape) == (N, 1, 56, 56) for p in preds)
    assert len(grads) == 26 + 1
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
    for s, (a, b) in enumerate(zip(preds, problem["stock"][0])):
        e = nerr(a.numpy(), b.numpy())
        print("predictions, native-gradient route against stock, class step %d: %.3g (bound 2e-4)" % (s, e))
        assert e < 2e-4


def test_native_gradients_against_float64(problem):
    ref_preds, ref = problem["ref"]
    ref_stock = problem["ref_stock"][1]
    for s, (a, b) in enumerate(zip(problem["native"][0], ref_preds)):
        print("predictions against float64, class step %d: native %.3g, stock %.3g" % (s, nerr(a.numpy(), b.numpy()),
                                                                                         nerr(problem["stock"][0][s].numpy(), b.numpy())))
    failures = []
    for name in ref:
        e_native = nerr(problem["native"][1][name].numpy(), ref[name].numpy())
        e_stock = nerr(problem["stock"][1][name].numpy(), ref_stock[name].numpy())
        bound = max(2e-5, 4 * e_stock)
        print("%-55s native %.3e   stock %.3e   (bound %.3e)" % (name, e_native, e_stock, bound))
        if not e_native < bound:
            failures.append((name, e_native, bound))
    assert not failures, failures


def test_native_gradients_repeat_bit_for_bit(problem):
    """A second native-gradient pass in the same process: the weight and bias gradient of every Conv2d -- the layers whose backward
    is mpnhip_conv2d_backward, the last of them at the far end of the whole chain -- is bitwise the first's.  The two
    ConvTranspose2d layers stay stock modules: their weight gradient is MIOpen's, which may add with atomics, so their comparison
    is printed, not asserted (their DATA gradient feeds the Conv2d layers behind them, which are asserted)."""
    again = run(problem["model"], problem["x_ext"], problem["ei"], problem["logits"], 'native')[1]
    first = problem["native"][1]
    kinds = {top + "." + n: type(mod) for top, m in mask_modules(problem["model"]) for n, mod in m.named_modules()
             if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))}
    assert sum(k is torch.nn.Conv2d for k in kinds.values()) == 10 and sum(k is torch.nn.ConvTranspose2d for k in kinds.values()) == 2
    differing = []
    for name, kind in kinds.items():
        for leaf in ("weight", "bias"):
            same = torch.equal(first[name + "." + leaf], again[name + "." + leaf])
            if kind is torch.nn.ConvTranspose2d:
                print("stock ConvTranspose2d %s.%s: run-to-run %s" % (name, leaf, "bitwise equal" if same else "max difference %.3g of the largest"
                      % nerr(again[name + "." + leaf].numpy(), first[name + "." + leaf].numpy())))
            elif not same:
                differing.append(name + "." + leaf)
    assert not differing, differing


def check_fallback(model, x_ext, ei, logits):
    model.mask_conv_grads = 'native'
    assert not all(m.native_supported() for m in model._mask_modules())
    capi.path_counters(reset=True)
    preds = model.mask_predictions(x_ext, ei, logits)
    sum(p.sum() for p in preds).backward()
    torch.cuda.synchronize()
    c = capi.path_counters()
    assert not any(c[k] for k in NEW + NATIVE_FWD), {k: c[k] for k in NEW + NATIVE_FWD}
    for name, p in mask_parameters(model):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert logits.grad is not None


def test_a_5x5_stack_takes_the_stock_path():
    model, x_ext, ei, logits = window_problem()
    old = model.mask_predictor.mask_head.layers[0]
    wide = torch.nn.Conv2d(64, 64, kernel_size=5, padding=2).to(dev())
    with torch.no_grad():
        wide.weight.zero_()
        wide.weight[:, :, 1:4, 1:4] = old.weight
        wide.bias.copy_(old.bias)
    model.mask_predictor.mask_head.layers[0] = wide
    check_fallback(model, x_ext, ei, logits)


def test_training_dropout_takes_the_stock_path():
    model, x_ext, ei, logits = window_problem()
    model.MPAttentionNet.node_model.layers.append(torch.nn.Dropout2d(p=0.4))
    assert model.training
    check_fallback(model, x_ext, ei, logits)
    # in eval mode the Dropout is off and the stack is covered again
    model.eval()
    capi.path_counters(reset=True)
    sum(p.sum() for p in model.mask_predictions(x_ext, ei, logits)).backward()
    assert new_counts()["conv_wgrad"] > 0


def test_bad_selector_raises():
    model, x_ext, ei, logits = window_problem()
    model.mask_conv_grads = 'fast'
    with pytest.raises(capi.MpnhipError, match="mask_conv_grads"):
        model.mask_predictions(x_ext, ei, logits)
    with pytest.raises(capi.MpnhipError, match="mask_conv_grads"):
        with torch.no_grad():
            model.mask_predictions(x_ext, ei, logits)
