"""The Mask R-CNN FPN backbone's native inference forward (fpn_net.BackboneWithFPN.forward_native over csrc/conv_strided.hip)
with seeded weights on two frames of 45 x 70 transformed with (min_size, max_size) = (60, 90) -- a [2, 3, 64, 96] batch, the
smallest at which every level still has more than one pixel and the padding is exercised --, against the module's own float64 CPU
forward on the same float32 batch.

Bound, per output: max(2e-6, 4 x max(nerr of the float32 CPU forward, nerr of the stock device forward)), nerr = max |got - ref64| /
max |ref64|.  No value is fixed: the accumulated error of 61 exact-fp32 layers on the device is not known in advance.  The test
prints all the errors; should a native error exceed its bound it prints the error after the stem, after C2 .. C5 and of the four
inner maps, to find the layer."""
import copy

import numpy as np
import pytest
import torch

from mpntrackseg_amd import capi, embed_inputs as E, embeddings as EM, fpn_net, synth

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 2e-6
SEED = 37
NAMES = ('0', '1', '2', '3', 'pool')
TRANSFORM = dict(min_size=60, max_size=90)


def nerr(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


class Seeded:
    """everything the tests share, computed once: the module on the device, the frames, the four forwards, the bounds"""

    def __init__(self):
        host = fpn_net.resnet50_fpn_backbone()
        synth.make_fpn_weights(host, SEED)
        host.eval()
        self.frames = torch.from_numpy((synth.uniform01(SEED, 2 * 45 * 70 * 3, stream=1) * 256).astype(np.uint8).reshape(2, 45, 70, 3)).to(dev())
        self.xd, self.image_size = E.rcnn_transform(self.frames, **TRANSFORM)
        self.x = self.xd.cpu()
        with torch.no_grad():
            self.cpu32 = host(self.x)
            self.host64 = copy.deepcopy(host).double()
            self.ref = self.host64(self.x.double())
        self.net = host.to(dev())
        with torch.no_grad():
            self.stock = self.net(self.xd)
        capi.path_counters(reset=True)
        self.native = self.net.forward_native(self.xd)
        torch.cuda.synchronize()
        self.counters = capi.path_counters()
        self.err = {name: {k: nerr(out[k].cpu(), self.ref[k]) for k in NAMES}
                    for name, out in (("cpu32", self.cpu32), ("stock", self.stock), ("native", self.native))}
        self.bound = {k: max(TOL, 4 * max(self.err["cpu32"][k], self.err["stock"][k])) for k in NAMES}


@pytest.fixture(scope="module")
def seeded():
    return Seeded()


def stage_errors(s):
    """the native activations after the stem, after every stage and of the inner maps against the float64 CPU forward"""
    stages = []
    s.net.forward_native(s.xd, stages=stages)
    h, t = s.host64, s.x.double()
    with torch.no_grad():
        b = h.body
        t = b.maxpool(b.relu(b.bn1(b.conv1(t))))
        want = [("stem", t)]
        body = {}
        for i in range(4):
            t = getattr(b, "layer%d" % (i + 1))(t)
            want.append(("C%d" % (i + 2), t))
            body[str(i)] = t
        want += [("inner%d" % (3 - i), m) for i, m in enumerate(h.fpn.inner_maps(body))]
    assert [n for n, _ in stages] == [n for n, _ in want]
    return [(name, nerr(got.cpu(), ref)) for (name, got), (_, ref) in zip(stages, want)]


def test_native_forward_against_float64(seeded):
    s = seeded
    assert s.image_size == (57, 90) and tuple(s.xd.shape) == (2, 3, 64, 96)
    assert list(s.native) == list(NAMES)
    shapes = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
    for k, hw in zip(NAMES, shapes):
        print("%s: native %.3g, stock device %.3g, float32 CPU %.3g (bound %.3g)"
              % (k, s.err["native"][k], s.err["stock"][k], s.err["cpu32"][k], s.bound[k]))
        assert tuple(s.native[k].shape) == (2, 256) + hw and s.native[k].is_contiguous()
    if any(s.err["native"][k] >= s.bound[k] for k in NAMES):
        for name, e in stage_errors(s):
            print("  %s: %.3g" % (name, e))
    for k in NAMES:
        assert s.err["native"][k] < s.bound[k], k
    assert torch.equal(s.native['pool'], s.native['3'][:, :, ::2, ::2])


def test_the_stages_are_the_modules_stages(seeded):
    """the diagnosis hook names nine activations, each within the loosest output bound of the float64 forward"""
    errs = stage_errors(seeded)
    assert [n for n, _ in errs] == ["stem", "C2", "C3", "C4", "C5", "inner3", "inner2", "inner1", "inner0"]
    print(", ".join("%s %.3g" % ne for ne in errs))
    assert all(e < max(seeded.bound.values()) for _, e in errs)


def test_which_kernels_ran(seeded):
    c = seeded.counters
    assert c["conv_affine_tile"] == 61 and c["conv_affine_up"] == 3 and c["maxpool"] == 1, {k: v for k, v in c.items() if v}
    assert c["conv_affine_grouped"] == 6 + 3 + 4       # the 3 x 3 of layer3 and layer4, and the four output convolutions (K = 2304)
    assert c["conv_tile"] == 0 and c["conv_small_cout"] == 0


def test_features_do_not_depend_on_the_batch(seeded):
    s = seeded
    one = s.net.forward_native(s.xd[1:2])
    for k in NAMES:
        assert torch.equal(one[k][0], s.native[k][1]), k
    sliced = s.net.forward_native(s.xd, max_images=1)
    for k in NAMES:
        assert torch.equal(sliced[k], s.native[k]), k
    none = s.net.forward_native(s.xd[:0])
    assert [tuple(none[k].shape) for k in NAMES] == [(0,) + tuple(s.native[k].shape[1:]) for k in NAMES]


def test_one_frame_of_40_by_72(seeded):
    """the upper left 40 x 72 of the first frame: levels of 10 x 18, 5 x 9, 3 x 5 and 2 x 3 -- odd strided sizes, and upsample
    ratios that are no integers (3 -> 5, 5 -> 9).  The module docstring's rule, its comparators measured here."""
    s = seeded
    xd = s.xd[:1, :, :40, :72].contiguous()
    x = xd.cpu()
    with torch.no_grad():
        stock = s.net(xd)
        cpu32 = copy.deepcopy(s.net).cpu()(x)
        ref = s.host64(x.double())
    native = s.net.forward_native(xd)
    shapes = [(10, 18), (5, 9), (3, 5), (2, 3), (1, 2)]
    for k, hw in zip(NAMES, shapes):
        e_native, e_stock, e_cpu = nerr(native[k].cpu(), ref[k]), nerr(stock[k].cpu(), ref[k]), nerr(cpu32[k], ref[k])
        bound = max(TOL, 4 * max(e_cpu, e_stock))
        print("%s: native %.3g, stock device %.3g, float32 CPU %.3g (bound %.3g)" % (k, e_native, e_stock, e_cpu, bound))
        assert tuple(native[k].shape) == (1, 256) + hw
        assert e_native < bound, k


def test_refusals_and_the_dropped_cache(seeded):
    s = seeded
    net = copy.deepcopy(s.net)
    with pytest.raises(capi.MpnhipError):
        net.train().forward_native(s.xd)
    net.eval()
    with pytest.raises(capi.MpnhipError):
        net.forward_native(s.x)                                   # a CPU input
    with pytest.raises(capi.MpnhipError):
        net.forward_native(s.xd.double())
    with pytest.raises(capi.MpnhipError):
        net.forward_native(s.xd[:, :2])
    with pytest.raises(capi.MpnhipError):
        net.forward_native(s.xd[:, :, :, :64])                    # not contiguous
    with pytest.raises(capi.MpnhipError):
        net.forward_native(s.xd.permute(0, 1, 3, 2))
    f0 = net.forward_native(s.xd)
    assert net._native is not None and all(torch.equal(f0[k], s.native[k]) for k in NAMES)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    sd["body.layer4.2.bn3.weight"] *= 2.0
    sd["fpn.inner_blocks.1.bias"] += 1.0
    net.load_state_dict(sd)
    assert net._native is None
    f1 = net.forward_native(s.xd)
    # the rebuilt constants are the new weights': the module docstring's rule against the changed network's own float64 forward
    with torch.no_grad():
        stock = net(s.xd)
        host = copy.deepcopy(net).cpu()
        cpu32 = host(s.x)
        ref = host.double()(s.x.double())
    for k in NAMES:
        assert not torch.equal(f1[k], f0[k]), k
        bound = max(TOL, 4 * max(nerr(cpu32[k], ref[k]), nerr(stock[k].cpu(), ref[k])))
        assert nerr(f1[k].cpu(), ref[k]) < bound, (k, bound)


def test_node_ext_embeddings_from_frames_and_their_files(seeded, tmp_path):
    """five boxes in the frames' own 45 x 70 coordinates, two of them in the second frame's lower right corner -- the cells next
    to the padding"""
    s = seeded
    det = {"frame": np.asarray([4, 4, 4, 9, 9]), "detection_id": np.asarray([12, 15, 70001, 3, 8]),
           "bb_left": np.asarray([2.0, 20.5, 0.0, 48.0, 30.25]), "bb_top": np.asarray([3.0, 10.25, 0.0, 27.0, 20.0]),
           "bb_right": np.asarray([30.0, 45.0, 70.0, 70.0, 69.5]), "bb_bot": np.asarray([40.0, 30.0, 45.0, 45.0, 44.75])}
    got = E.node_ext_embeddings_from_frames(s.net, s.frames, det, convs='native', **TRANSFORM)
    assert tuple(got.shape) == (5, 1 + 256, 14, 14) and got.is_cuda and got.dtype == torch.float32
    assert torch.equal(got[:, 0].cpu(), torch.tensor([12.0, 15.0, 70001.0, 3.0, 8.0]).view(5, 1, 1).expand(5, 14, 14))
    feats, size = E.fpn_features(s.net, s.frames, convs='native', **TRANSFORM)
    assert size == (57, 90) and all(torch.equal(feats[k], s.native[k]) for k in NAMES)
    again = E.node_ext_embeddings([feats[k] for k in NAMES[:4]], det, size, original_size=(45, 70))
    assert torch.equal(again, got)
    # the same call on the float64 forward's features, on the float32 CPU forward's and on the stock device forward's: the rule
    # of the module docstring with nerr relative to the largest embedding.  (A pooled value is an average of bilinear taps -- a
    # convex combination of cells of ONE level, the same cells and weights on every side -- so neither an error nor the largest
    # value can exceed the level's own.)
    pooled = lambda feats: E.node_ext_embeddings([feats[k].float().to(dev()) for k in NAMES[:4]], det, size, original_size=(45, 70))[:, 1:]
    want = pooled(s.ref)
    stock = E.node_ext_embeddings_from_frames(s.net, s.frames, det, **TRANSFORM)               # convs='stock' is the default
    assert tuple(stock.shape) == tuple(got.shape) and torch.equal(stock[:, 0], got[:, 0])
    e_native, e_cpu, e_stock = nerr(got[:, 1:], want), nerr(pooled(s.cpu32), want), nerr(stock[:, 1:], want)
    bound = max(TOL, 4 * max(e_cpu, e_stock))
    print("embeddings: native %.3g, stock device %.3g, float32 CPU %.3g (bound %.3g), max |ref| %.3g"
          % (e_native, e_stock, e_cpu, bound, float(want.abs().max())))
    assert float(want.abs().max()) > 0 and e_native < bound
    with pytest.raises(ValueError):
        E.node_ext_embeddings_from_frames(s.net, s.frames, det, convs='miopen', **TRANSFORM)
    by_number = E.node_ext_embeddings_from_frames(s.net, s.frames.flip(0), det, convs='native', frames_index=[9, 4], **TRANSFORM)
    assert torch.equal(by_number, got)

    rel = E.store_node_ext_embeddings(str(tmp_path), "dets_file", "node_ext", det["frame"], got)
    stored = torch.load(str(tmp_path / "processed_data" / rel / "9.pt"))
    assert tuple(stored.shape) == (2, 257, 14, 14) and stored[:, 0, 13, 13].tolist() == [3.0, 8.0]
    back = EM.load_precomputed_embeddings(det, {"seq_path": str(tmp_path)}, rel, embedding_dim='3D')
    assert back.is_cuda and torch.equal(back, got[:, 1:])
