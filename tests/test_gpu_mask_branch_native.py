"""The mask branch with ``MOTMPNet.mask_convs = 'native'``: every convolution, transposed convolution and the LayerNorm of
``mask_predictions`` through mpnhip_conv2d_forward / mpnhip_layer_norm_forward (csrc/conv.hip) -- against the reference's own
output (tests/golden/g6_mask_branch.npz, bounds of tests/test_gpu_mask_branch.py), against the stock PyTorch-ROCm modules on the
same commit (2e-4 of the largest value, the fixture's bound), and through the tracker's window loop; plus the conditions under which
the call silently takes the stock path instead (gradients recorded, a stack outside what the kernels cover)."""
import numpy as np
import pytest
import torch

from mpntrackseg_amd import capi, synth, tracker
from mpntrackseg_amd.cnn import CNN
from mpntrackseg_amd.mpn import MOTMPNet

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
NATIVE = ("conv_tile", "conv_small_cout", "conv_transpose", "layer_norm")


def nerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-6))


def native_counts():
    c = capi.path_counters()
    return {k: c[k] for k in NATIVE}


def make_model(L, num_class_steps=2, node_in_dim=64, reattach=True, gain=1.0):
    params = synth.model_params(32, L, "sum", num_class_steps=num_class_steps, node_in_dim=node_in_dim)
    params.update(synth.MASK_PARAMS)
    params["reattach_initial_nodes"] = reattach
    model = MOTMPNet(params)
    W = synth.make_weights(params, seed=7, gain=gain)
    W.update(synth.make_mask_weights(seed=17))
    sd = model.state_dict()
    for k, v in W.items():
        if tuple(sd[k].shape) == tuple(v.shape):
            sd[k] = torch.from_numpy(v)
        else:      # without reattach the first node-model convolution has 96 input channels: He-scaled weights of that shape
            sd[k] = torch.from_numpy(synth.normal(23, tuple(sd[k].shape), std=float(np.sqrt(2.0 / (sd[k].shape[1] * 9)))))
    model.load_state_dict(sd, strict=True)
    return model.to(dev()).eval()


def g6(z):
    N, E, L, nin = int(z["N"]), int(z["E"]), int(z["L"]), int(z["node_in_dim"])
    model = make_model(L, node_in_dim=nin)
    g = synth.make_graph(N, E, T=8, seed=4, node_in_dim=nin)

    class D:
        pass
    d = D()
    d.x = torch.from_numpy(g["x"]).view(N, nin, 1, 1).to(dev())
    d.x_ext = torch.from_numpy(synth.normal(5, (N, 256, 14, 14), stream=1, std=0.5)).to(dev())
    d.edge_index = torch.from_numpy(g["edge_index"]).to(dev())
    d.edge_attr = torch.from_numpy(g["edge_attr"]).to(dev())
    return model, d, N, E


def test_g6_forward_native(golden):
    z = golden("g6_mask_branch.npz")
    model, d, N, E = g6(z)
    assert int(z["L"]) == 3
    model.mask_convs = 'native'
    capi.path_counters(reset=True)
    with torch.no_grad():
        out = model(d)
    torch.cuda.synchronize()
    counts = native_counts()
    assert len(out["classified_edges"]) == 2 and len(out["mask_predictions"]) == 2
    for s in range(2):
        assert nerr(out["classified_edges"][s].cpu().numpy().reshape(-1), z["logits"][s]) < 1e-4
        m = out["mask_predictions"][s]
        assert m.shape == (N, 1, 56, 56)
        e = nerr(m[:12].cpu().numpy(), z["mask_rows"][s])
        print("g6 native, class step %d: mask rows %.3g (bound 2e-4)" % (s, e))
        assert e < 2e-4
        assert abs(float(m.double().abs().sum()) - float(z["mask_abssum"][s])) < 2e-4 * float(z["mask_abssum"][s])
    # L = 3, two class steps: 2 encoder + 3 x 2 node-model convolutions; per class step the feature encoder, 3 mask-head and 2
    # predictor convolutions (the last of them, 64 -> 1, in the small-cout kernel), 2 transposed convolutions and the LayerNorm
    assert counts == {"conv_tile": 2 + 6 + 2 * 5, "conv_small_cout": 2, "conv_transpose": 2 * 2, "layer_norm": 2}, counts


def window_problem(N=7, E=24, L=2, reattach=True, num_class_steps=2):
    model = make_model(L, num_class_steps=num_class_steps, reattach=reattach, gain=0.6)
    g = synth.make_graph(N, E, T=4, seed=6, node_in_dim=64)
    x = torch.from_numpy(g["x"]).to(dev())
    ei = torch.from_numpy(g["edge_index"]).to(dev())
    ea = torch.from_numpy(g["edge_attr"]).to(dev())
    x_ext = torch.from_numpy(synth.normal(8, (N, 256, 14, 14), stream=1, std=0.5)).to(dev())
    with torch.no_grad():
        logits = model.hot_path(x, ei, ea)
    return model, x_ext, ei, logits


def both_ways(model, x_ext, ei, logits, **kw):
    with torch.no_grad():
        model.mask_convs = 'stock'
        capi.path_counters(reset=True)
        stock = model.mask_predictions(x_ext, ei, logits, **kw)
        assert not any(native_counts().values())
        model.mask_convs = 'native'
        native = model.mask_predictions(x_ext, ei, logits, **kw)
        assert native_counts()["layer_norm"] == len(native)
    return stock, native


def test_last_only_is_the_full_lists_last():
    model, x_ext, ei, logits = window_problem()
    model.mask_convs = 'native'
    with torch.no_grad():
        every = model.mask_predictions(x_ext, ei, logits)
        capi.path_counters(reset=True)
        last = model.mask_predictions(x_ext, ei, logits, last_only=True)
    assert len(every) == 2 and len(last) == 1
    assert native_counts()["layer_norm"] == 1
    assert torch.equal(last[0], every[-1])


@pytest.mark.parametrize("L,reattach", [(2, True), (2, False), (0, True)], ids=["L2", "L2_no_reattach", "L0"])
def test_native_against_stock(L, reattach):
    model, x_ext, ei, logits = window_problem(L=L, reattach=reattach, num_class_steps=min(2, max(L, 1)))
    assert model.MPAttentionNet.node_model.layers[0].in_channels == (192 if reattach else 96)
    stock, native = both_ways(model, x_ext, ei, logits)
    assert len(stock) == len(native) == (2 if L else 1)
    for s, n in zip(stock, native):
        assert tuple(n.shape) == tuple(s.shape) == (7, 1, 56, 56)
        e = nerr(n.cpu().numpy(), s.cpu().numpy())
        print("native against stock, L %d reattach %s: %.3g (bound 2e-4)" % (L, reattach, e))
        assert e < 2e-4


def test_training_forward_falls_back_to_stock():
    model, x_ext, ei, logits = window_problem()
    model.mask_convs = 'native'
    model.train()
    x_ext.requires_grad_(True)
    capi.path_counters(reset=True)
    preds = model.mask_predictions(x_ext, ei, logits)
    assert not any(native_counts().values())
    sum(p.sum() for p in preds).backward()
    for m in (model.node_ext_encoder, model.MPAttentionNet.node_model, model.mask_predictor):
        for name, p in m.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(model.MPAttentionNet.node_model.layers[0].weight.grad.abs().max()) > 0
    assert x_ext.grad is not None


def test_unsupported_stack_takes_the_stock_path():
    cnn = CNN(input_dim=4, dims=[6], kernel_sizes=[5], strides=[1], paddings=[2], dropout_p=0)
    assert not cnn.native_supported()
    with pytest.raises(capi.MpnhipError):
        cnn.to(dev()).forward_native([torch.zeros((1, 4, 8, 8), device=dev())])
    model, x_ext, ei, logits = window_problem()
    with torch.no_grad():
        want = model.mask_predictions(x_ext, ei, logits)
    # the same weights in a 5 x 5 frame of zeros: the same function, but not a stack the kernels cover
    old = model.mask_predictor.mask_head.layers[0]
    wide = torch.nn.Conv2d(64, 64, kernel_size=5, padding=2).to(dev())
    with torch.no_grad():
        wide.weight.zero_()
        wide.weight[:, :, 1:4, 1:4] = old.weight
        wide.bias.copy_(old.bias)
    model.mask_predictor.mask_head.layers[0] = wide
    assert not model.mask_predictor.mask_head.native_supported() and not model.mask_predictor.native_supported()
    model.mask_convs = 'native'
    capi.path_counters(reset=True)
    with torch.no_grad():
        got = model.mask_predictions(x_ext, ei, logits)
    assert not any(native_counts().values())
    for g, w in zip(got, want):
        assert nerr(g.cpu().numpy(), w.cpu().numpy()) < 2e-4


def test_bad_selector_raises():
    model, x_ext, ei, logits = window_problem()
    model.mask_convs = 'fast'
    with pytest.raises(capi.MpnhipError):
        with torch.no_grad():
            model.mask_predictions(x_ext, ei, logits)


def small_sequence(frames=6, dets=4):
    n = frames * dets
    frame = np.repeat(1 + np.arange(frames, dtype=np.int64), dets)
    lo, hi = np.nonzero(np.triu(frame[:, None] != frame[None, :], 1))
    half = lo.size
    ei = np.stack([np.concatenate([lo, hi]), np.concatenate([hi, lo])]).astype(np.int64)
    ea = synth.normal(41, (half, 6), stream=0)
    dist = synth.uniform01(41, half, stream=1).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev())
    args = (t(synth.normal(41, (n, 64), stream=2)), t(ei), t(np.concatenate([ea, ea])), t(np.concatenate([dist, dist])), frame)
    return args, t(synth.normal(41, (n, 256, 14, 14), stream=3, std=0.5))


def test_tracker_native_against_stock_and_across_batchings():
    model = make_model(4, gain=0.6)
    args, x_ext = small_sequence()
    cfg = dict(frames_per_graph=3, top_k_nns=3, x_ext=x_ext)
    stock = tracker.evaluate_sequence(model, *args, **cfg)
    model.mask_convs = 'native'
    capi.path_counters(reset=True)
    one = tracker.evaluate_sequence(model, *args, windows_per_launch=1, **cfg)
    assert native_counts()["layer_norm"] == 4                    # 6 frames, 3 per graph: 4 windows, the last step's masks of each
    capi.path_counters(reset=True)
    four = tracker.evaluate_sequence(model, *args, windows_per_launch=4, **cfg)
    assert native_counts()["layer_norm"] == 1
    assert tuple(one.node_preds.shape) == (24, 1, 56, 56) and not bool(torch.isnan(one.node_preds).any())
    e = float((one.node_preds - stock.node_preds).abs().max())
    print("tracker node_preds, native against stock: %.3g (bound 2e-4)" % e)
    assert e < 2e-4
    assert torch.equal(one.final_edge_preds, stock.final_edge_preds)
    assert torch.equal(one.node_preds, four.node_preds)
