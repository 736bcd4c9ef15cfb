"""The ReID network's host module without a GPU: reid_net.ResNet against the fixture of the reference's resnet50_fc256
(tests/golden/g26_reid_resnet.npz, written by tools/make_golden_reid_resnet.py: the reference in float64 on the CPU with
synth.make_reid_weights), the checkpoint loader's tolerance, and the folded BatchNorm constants of prepare_native."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mpntrackseg_amd import capi, reid_net, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_reid_resnet.npz")
TOL64 = 1e-12      # float64 on both sides, only the summation order may differ


def nerr(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def seeded(golden):
    """(the float64 module with the fixture's weights, its (f, v) on the fixture's inputs), computed once"""
    net = reid_net.resnet50_fc256(10, loss='xent')
    synth.make_reid_weights(net, int(golden["seed"]))
    net = net.eval().double()
    x = torch.from_numpy(synth.normal(int(golden["seed"]), (3, 3, 128, 64), stream=synth.REID_INPUT_STREAM)).double()
    with torch.no_grad():
        f, v = net(x)
    return net, f, v


def test_state_dict_names_and_shapes_match_the_reference(golden):
    sd = reid_net.resnet50_fc256(10).state_dict()
    assert list(sd) == [str(k) for k in golden["names"]]
    assert len(sd) == 334
    for k, shp in zip(sd, golden["shapes"]):
        assert list(sd[k].shape) == [int(s) for s in shp if s >= 0], k
    for k in ("layer1.0.downsample.0.weight", "layer4.0.downsample.1.running_var", "layer3.5.bn3.num_batches_tracked", "fc.0.weight",
              "fc.1.running_mean", "fc.3.bias", "fc.4.weight", "classifier.bias"):
        assert k in sd, k


def test_float64_forward_matches_the_reference(golden, seeded):
    _, f, v = seeded
    assert tuple(f.shape) == tuple(int(s) for s in golden["f_shape"]) == (3, 2048, 8, 4) and tuple(v.shape) == (3, 256)
    flat = f.reshape(-1)
    e_v, e_f = nerr(v, golden["v"]), nerr(flat[::int(golden["f_step"])], golden["f_sample"])
    e_sum = abs(float(flat.sum()) - float(golden["f_sum"])) / float(golden["f_abs_sum"])
    e_abs = abs(float(flat.abs().sum()) - float(golden["f_abs_sum"])) / float(golden["f_abs_sum"])
    print("v %.3g, f sample %.3g, f sum %.3g, f abs-sum %.3g (bound %.1g)" % (e_v, e_f, e_sum, e_abs, TOL64))
    assert e_v < TOL64 and e_f < TOL64 and e_sum < TOL64 and e_abs < TOL64
    # the ReLUs are neither dead nor idle
    zero_share = float((flat == 0).double().mean())
    assert 0.1 <= zero_share <= 0.9, zero_share
    assert abs(zero_share - float(golden["f_zero_share"])) < 1e-3


def test_load_pretrained_weights_round_trip(tmp_path, golden):
    src = reid_net.resnet50_fc256(10)
    synth.make_reid_weights(src, 5)
    sd = src.state_dict()
    # DataParallel's prefix, inside a {'state_dict': ...} wrapper, with a classifier of another size and a key nobody has
    saved = {"module." + k: v.clone() for k, v in sd.items()}
    saved["module.classifier.weight"] = torch.zeros(751, 256)
    saved["module.classifier.bias"] = torch.zeros(751)
    saved["module.not_a_layer.weight"] = torch.zeros(3)
    path = str(tmp_path / "ckpt.pth.tar")
    torch.save({"state_dict": saved, "epoch": 3}, path)
    dst = reid_net.resnet50_fc256(10)
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    loaded, skipped = reid_net.load_pretrained_weights(dst, path)
    assert sorted(skipped) == ["classifier.bias", "classifier.weight", "not_a_layer.weight"]
    assert len(loaded) == len(sd) - 2
    after = dst.state_dict()
    for k in sd:
        want = before[k] if k.startswith("classifier.") else sd[k]
        assert torch.equal(after[k], want), k
    # a bare state_dict without prefix loads as well
    path2 = str(tmp_path / "bare.pth")
    torch.save(sd, path2)
    dst2 = reid_net.resnet50_fc256(10)
    loaded2, skipped2 = reid_net.load_pretrained_weights(dst2, path2)
    assert skipped2 == [] and len(loaded2) == len(sd)
    assert all(torch.equal(dst2.state_dict()[k], sd[k]) for k in sd)


def test_folded_constants_reproduce_batchnorm_in_float64(seeded):
    """prepare_native on CPU tensors: conv -> * scale + shift with the folded constants is bn(conv(x)) in float64, on the first
    block of layer2 (a strided 3 x 3 and a strided downsample) and on fc."""
    net, _, _ = seeded
    native = net.prepare_native()
    assert net._native is native and len(native["affine"]) == 53 and len(native["fc"]) == 2
    blk = net.layer2[0]
    x = torch.from_numpy(synth.normal(3, (2, 256, 16, 8), stream=7)).double()
    worst = 0.0
    with torch.no_grad():
        t = x
        for conv, bn, name in ((blk.conv1, blk.bn1, "layer2.0.conv1"), (blk.conv2, blk.bn2, "layer2.0.conv2"),
                               (blk.conv3, blk.bn3, "layer2.0.conv3")):
            scale, shift = native["affine"][name]
            assert scale.dtype == torch.float64 and not scale.is_cuda
            c = conv(t)
            want = bn(c)
            worst = max(worst, nerr(c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), want))
            t = want.relu()
        scale, shift = native["affine"]["layer2.0.downsample.0"]
        c = blk.downsample[0](x)
        worst = max(worst, nerr(c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), blk.downsample[1](c)))
        h = torch.from_numpy(synth.normal(3, (4, 2048), stream=8)).double()
        for (w, b), i in zip(native["fc"], (0, 3)):
            want = net.fc[i + 1](net.fc[i](h))
            worst = max(worst, nerr(F.linear(h, w, b), want))
            h = want.relu()
    print("folded constants: %.3g (bound %.1g)" % (worst, TOL64))
    assert worst < TOL64


def test_cache_is_dropped_and_refusals_need_no_gpu(seeded):
    net, _, _ = seeded
    net.prepare_native()
    assert net._native is not None
    net.load_state_dict(net.state_dict())
    assert net._native is None
    net.prepare_native()
    net.train()
    assert net._native is None
    with pytest.raises(capi.MpnhipError):
        net.forward_native(torch.zeros(1, 3, 128, 64))          # training mode
    net.eval()
    net.prepare_native()
    net.double()
    assert net._native is None
    with pytest.raises(capi.MpnhipError):
        net.forward_native(torch.zeros(1, 3, 128, 64))          # a CPU input
    with pytest.raises(capi.MpnhipError):
        reid_net.ResNet(10, 'xent', reid_net.Bottleneck, [1, 1, 1, 1], fc_dims=[16], dropout_p=0.5).eval().forward_native(
            torch.zeros(1, 3, 32, 32))
