"""The ReID ResNet50's native inference forward (reid_net.ResNet.forward_native over csrc/conv_strided.hip) with seeded weights on
three 128 x 64 crops, against the module's own float64 CPU forward -- which tests/test_reid_resnet_cpu.py pins to the reference.

Bound, for f and for v separately: max(2e-6, 4 x max(nerr of the float32 CPU forward, nerr of the stock device forward)).  The
stock device forward, through MIOpen, is what the native forward replaces; no value is fixed because nobody has measured the
accumulated error of 53 exact-fp32 layers on the device (the float32 CPU forward sits at 1.05e-6 / 4.3e-7 where the fixture was
written and at 1.05e-6 / 7.7e-7 on the CPU of the MI355X machine: torch's CPU kernels differ by host).  The test
prints all three errors; should the native error exceed the bound it prints the error after the stem and after each of the four
stages against the float64 forward, to find the layer."""
import copy

import numpy as np
import pytest
import torch

from mpntrackseg_amd import capi, embed_inputs as E, embeddings as EM, reid_net, synth

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 2e-6
SEED = 31


def nerr(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


class Seeded:
    """everything the tests share, computed once: the module on the device, the crops, the four forwards, the bounds"""

    def __init__(self):
        host = reid_net.resnet50_fc256(10, loss='xent')
        synth.make_reid_weights(host, SEED)
        host.eval()
        self.x = torch.from_numpy(synth.normal(SEED, (3, 3, 128, 64), stream=synth.REID_INPUT_STREAM))
        with torch.no_grad():
            self.cpu32 = host(self.x)
            self.host64 = copy.deepcopy(host).double()
            self.ref = self.host64(self.x.double())
        self.net = host.to(dev())
        self.xd = self.x.to(dev())
        with torch.no_grad():
            self.stock = self.net(self.xd)
        capi.path_counters(reset=True)
        self.native = self.net.forward_native(self.xd)
        torch.cuda.synchronize()
        self.counters = capi.path_counters()
        self.err = {name: (nerr(out[0].cpu(), self.ref[0]), nerr(out[1].cpu(), self.ref[1]))
                    for name, out in (("cpu32", self.cpu32), ("stock", self.stock), ("native", self.native))}
        self.bound = tuple(max(TOL, 4 * max(self.err["cpu32"][i], self.err["stock"][i])) for i in range(2))


@pytest.fixture(scope="module")
def seeded():
    return Seeded()


def stage_errors(s):
    """the native activations after the stem and after every stage against the float64 CPU forward"""
    stages = []
    s.net.forward_native(s.xd, stages=stages)
    h, t = s.host64, s.x.double()
    with torch.no_grad():
        t = h.maxpool(h.relu(h.bn1(h.conv1(t))))
        want = [("stem", t)]
        for name in ("layer1", "layer2", "layer3", "layer4"):
            t = getattr(h, name)(t)
            want.append((name, t))
    return [(name, nerr(got.cpu(), ref)) for (name, got), (_, ref) in zip(stages, want)]


def test_native_forward_against_float64(seeded):
    s = seeded
    for i, what in enumerate(("f", "v")):
        print("%s: native %.3g, stock device %.3g, float32 CPU %.3g (bound %.3g)"
              % (what, s.err["native"][i], s.err["stock"][i], s.err["cpu32"][i], s.bound[i]))
    assert tuple(s.native[0].shape) == (3, 2048, 8, 4) and tuple(s.native[1].shape) == (3, 256)
    if s.err["native"][0] >= s.bound[0] or s.err["native"][1] >= s.bound[1]:
        for name, e in stage_errors(s):
            print("  after %s: %.3g" % (name, e))
    assert s.err["native"][0] < s.bound[0]
    assert s.err["native"][1] < s.bound[1]


def test_the_stages_are_the_modules_stages(seeded):
    """the diagnosis hook names five activations of the right shapes, each within f's bound of the float64 forward"""
    errs = stage_errors(seeded)
    assert [n for n, _ in errs] == ["stem", "layer1", "layer2", "layer3", "layer4"]
    print(", ".join("%s %.3g" % ne for ne in errs))
    assert all(e < seeded.bound[0] for _, e in errs)


def test_which_kernels_ran(seeded):
    c = seeded.counters
    assert c["conv_affine_tile"] == 1 + 52 and c["maxpool"] == 1, {k: v for k, v in c.items() if v}
    assert c["conv_affine_small_grid"] == 52           # three crops: every launch but the stem's takes the 64 x 64 block
    assert c["conv_affine_grouped"] == 6 + 3          # the 3 x 3 of layer3 (K = 2304) and layer4 (K = 4608): grouped summation
    assert c["conv_tile"] == 0 and c["conv_small_cout"] == 0


def test_f_does_not_depend_on_the_batch(seeded):
    s = seeded
    f1, v1 = s.net.forward_native(s.xd[1:2])
    assert torch.equal(f1[0], s.native[0][1])
    # mpnhip_avgpool sums a row by its length alone, and below 8192 rows mpnhip_linear takes one kernel whatever the row count
    # (launch_gemm, csrc/gemm.hip): v's bits do not depend on the batch either
    assert torch.equal(v1[0], s.native[1][1])
    # slices of one image give the same bits as one slice of three
    f3, v3 = s.net.forward_native(s.xd, max_images=1)
    assert torch.equal(f3, s.native[0])
    assert torch.equal(v3, s.native[1])


def test_one_block_per_layer_on_odd_crops():
    """ResNet [1, 1, 1, 1] with last stride 2 and one fc layer on 2 crops of 37 x 21: every block has a downsample, the last one
    writes f, and the strided launches meet odd sizes (37 x 21 -> 19 x 11 -> pool 10 x 6 -> 5 x 3 -> 3 x 2 -> 2 x 1).  The module
    docstring's rule, its comparators measured here."""
    host = reid_net.ResNet(10, 'xent', reid_net.Bottleneck, [1, 1, 1, 1], fc_dims=[16])
    synth.make_reid_weights(host, SEED)
    host.eval()
    x = torch.from_numpy(synth.normal(SEED, (2, 3, 37, 21), stream=synth.REID_INPUT_STREAM))
    with torch.no_grad():
        cpu32 = host(x)
        ref = copy.deepcopy(host).double()(x.double())
        net = host.to(dev())
        stock = net(x.to(dev()))
    native = net.forward_native(x.to(dev()))
    assert tuple(native[0].shape) == (2, 2048, 2, 1) and tuple(native[1].shape) == (2, 16)
    for i, what in enumerate(("f", "v")):
        e_native, e_stock, e_cpu = nerr(native[i].cpu(), ref[i]), nerr(stock[i].cpu(), ref[i]), nerr(cpu32[i], ref[i])
        bound = max(TOL, 4 * max(e_cpu, e_stock))
        print("%s: native %.3g, stock device %.3g, float32 CPU %.3g (bound %.3g)" % (what, e_native, e_stock, e_cpu, bound))
        assert e_native < bound, what
    sliced = net.forward_native(x.to(dev()), max_images=1)
    assert torch.equal(sliced[0], native[0]) and torch.equal(sliced[1], native[1])


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
    f0, _ = net.forward_native(s.xd)
    assert net._native is not None and torch.equal(f0, s.native[0])
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    sd["layer4.2.bn3.weight"] *= 2.0
    net.load_state_dict(sd)
    assert net._native is None
    f1, _ = net.forward_native(s.xd)
    with torch.no_grad():
        want, _ = net(s.xd)
    assert not torch.equal(f1, f0)
    assert nerr(f1, want) < s.bound[0]


def test_reid_embeddings_and_their_files(seeded, tmp_path):
    """2 frames of 96 x 128, 5 boxes, one partly outside the frame"""
    s = seeded
    frames = torch.from_numpy((synth.uniform01(41, 2 * 96 * 128 * 3, stream=1) * 256).astype(np.uint8).reshape(2, 96, 128, 3)).to(dev())
    boxes = np.asarray([[10.0, 8.0, 50.0, 90.0], [60.5, 20.25, 100.0, 80.0], [-12.0, 30.0, 30.0, 110.0], [5.0, 5.0, 40.0, 60.0],
                        [70.0, 10.0, 120.0, 95.0]], np.float64)
    box_frame = np.asarray([0, 0, 0, 1, 1])
    node_core, reid = E.reid_embeddings(s.net, frames, boxes, box_frame, convs='native')
    assert tuple(node_core.shape) == (5, 2048, 8, 4) and tuple(reid.shape) == (5, 256) and node_core.is_cuda
    f, v = s.net.forward_native(E.reid_crops(frames, boxes, box_frame))
    assert torch.equal(node_core, f) and torch.equal(reid, v)
    f2, v2 = E.reid_embeddings(s.net, frames, boxes, box_frame, convs='native', batch_size=2)
    assert torch.equal(f2, f) and torch.equal(v2, v)
    sf, sv = E.reid_embeddings(s.net, frames, boxes, box_frame)                     # convs='stock' is the default
    e_f, e_v = nerr(node_core, sf), nerr(reid, sv)
    print("native against stock: f %.3g (bound %.3g), v %.3g (bound %.3g)" % (e_f, s.bound[0], e_v, s.bound[1]))
    assert e_f < s.bound[0] and e_v < s.bound[1]
    with pytest.raises(ValueError):
        E.reid_embeddings(s.net, frames, boxes, box_frame, convs='miopen')
    for convs in ('stock', 'native'):                                               # no detections: empty results on both routes
        f0, v0 = E.reid_embeddings(s.net, frames, np.zeros((0, 4)), np.zeros(0, np.int64), convs=convs)
        assert tuple(f0.shape) == (0, 2048, 8, 4) and tuple(v0.shape) == (0, 256) and f0.is_cuda and v0.is_cuda, convs

    det = {"frame": np.asarray([4, 4, 4, 9, 9]), "detection_id": np.asarray([12, 15, 70001, 3, 8])}
    stale = tmp_path / "processed_data" / "embeddings" / "dets_file" / "reid"
    stale.mkdir(parents=True)
    (stale / "77.pt").write_bytes(b"stale")
    reid_rel, core_rel = E.store_reid_embeddings(str(tmp_path), "dets_file", "reid", "node_core", det["frame"], det["detection_id"],
                                                 node_core, reid)
    assert sorted(p.name for p in stale.iterdir()) == ["4.pt", "9.pt"]              # the existing directory was removed first
    stored = torch.load(str(tmp_path / "processed_data" / core_rel / "4.pt"))
    assert tuple(stored.shape) == (3, 2049, 8, 4) and stored[:, 0, 7, 3].tolist() == [12.0, 15.0, 70001.0]
    stored = torch.load(str(stale / "9.pt"))
    assert tuple(stored.shape) == (2, 257) and stored[:, 0].tolist() == [3.0, 8.0]
    info = {"seq_path": str(tmp_path)}
    back1 = EM.load_precomputed_embeddings(det, info, reid_rel, embedding_dim='1D')
    back3 = EM.load_precomputed_embeddings(det, info, core_rel, embedding_dim='3D')
    assert back1.is_cuda and torch.equal(back1, reid) and torch.equal(back3, node_core)
