"""mpnhip_rcnn_transform (csrc/rcnn_transform.hip) through embed_inputs.rcnn_transform against GeneralizedRCNNTransform restated
on the CPU in float64: ((u8 / 255 - mean) / std) -> F.interpolate(size=(oh, ow), mode='bilinear', align_corners=False) -> zero
pad.  Frames: uniform random bytes from synth -- neighbouring pixels differ by up to the whole range, the hardest input for the
interpolation weights.

Error measure: nerr = max |got - ref64| / max |ref64|.  Bound per case: max(2e-6, 4 x max(nerr of torch's float32 CPU evaluation,
nerr of torch's float32 device evaluation)) of the same expression.  Outside oh x ow the output must be exactly 0."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mpntrackseg_amd import embed_inputs as E, synth

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 2e-6

# (label, B, H, W, min_size, max_size, (oh, ow, Hp, Wp) of the issue's table)
CASES = [
    ("up_45x70", 2, 45, 70, 60, 90, (57, 90, 64, 96)),          # up-scaling, the max_size branch, padding on both axes
    ("down_108x192", 1, 108, 192, 80, 133, (74, 133, 96, 160)),  # down-scaling
    ("same_64x96", 1, 64, 96, 64, 96, (64, 96, 64, 96)),        # identity size, no padding
]


def nerr(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def make_frames(seed, b, h, w):
    return torch.from_numpy((synth.uniform01(seed, b * h * w * 3, stream=1) * 256).astype(np.uint8).reshape(b, h, w, 3))


def reference(frames, sizes, dtype, device="cpu"):
    oh, ow, hp, wp = sizes
    x = frames.to(device).permute(0, 3, 1, 2).to(dtype) / 255
    mean = torch.tensor(E.IMAGENET_MEAN, dtype=dtype, device=device).view(1, 3, 1, 1)
    std = torch.tensor(E.IMAGENET_STD, dtype=dtype, device=device).view(1, 3, 1, 1)
    y = F.interpolate((x - mean) / std, size=(oh, ow), mode='bilinear', align_corners=False)
    return F.pad(y, (0, wp - ow, 0, hp - oh))


@pytest.fixture(scope="module")
def cases():
    out = {}
    for label, b, h, w, lo, hi, sizes in CASES:
        frames = make_frames(51, b, h, w)
        out[label] = (frames, reference(frames, sizes, torch.float64))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_transform_against_float64(case, cases):
    label, b, h, w, lo, hi, sizes = case
    oh, ow, hp, wp = sizes
    frames, ref = cases[label]
    got, image_size = E.rcnn_transform(frames.to(dev()), min_size=lo, max_size=hi)
    assert image_size == (oh, ow) and tuple(got.shape) == (b, 3, hp, wp) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu()
    e_gpu = nerr(got[:, :, :oh, :ow], ref[:, :, :oh, :ow])
    e_cpu = nerr(reference(frames, sizes, torch.float32), ref)
    e_dev = nerr(reference(frames, sizes, torch.float32, dev()).cpu(), ref)
    bound = max(TOL, 4 * max(e_cpu, e_dev))
    print("%s: kernel %.3g, float32 CPU %.3g, float32 device %.3g (bound %.3g)" % (label, e_gpu, e_cpu, e_dev, bound))
    assert e_gpu < bound
    outside = torch.ones((hp, wp), dtype=torch.bool)
    outside[:oh, :ow] = False
    assert int(outside.sum()) == hp * wp - oh * ow
    assert torch.equal(got[:, :, outside], torch.zeros_like(got[:, :, outside]))
    assert not torch.signbit(got[:, :, outside]).any()


def test_a_frame_alone_has_the_bits_it_has_in_the_batch(cases):
    frames, _ = cases["up_45x70"]
    whole, _ = E.rcnn_transform(frames.to(dev()), min_size=60, max_size=90)
    for i in range(2):
        one, size = E.rcnn_transform(frames[i:i + 1].to(dev()), min_size=60, max_size=90)
        assert size == (57, 90) and torch.equal(one[0], whole[i]), i
    again, _ = E.rcnn_transform(frames.to(dev()), min_size=60, max_size=90)
    assert torch.equal(again, whole)
    empty, size = E.rcnn_transform(frames[:0].to(dev()), min_size=60, max_size=90)
    assert tuple(empty.shape) == (0, 3, 64, 96) and size == (57, 90)


def test_other_constants_and_divisor(cases):
    """mean / std other than ImageNet's and size_divisible = 1 (no padding at all)"""
    frames, _ = cases["down_108x192"]
    mean, std = (0.1, 0.5, 0.9), (0.5, 0.25, 1.0)
    got, size = E.rcnn_transform(frames.to(dev()), min_size=80, max_size=133, mean=mean, std=std, size_divisible=1)
    assert size == (74, 133) and tuple(got.shape) == (1, 3, 74, 133)
    x = frames.permute(0, 3, 1, 2).double() / 255
    ref = F.interpolate((x - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1),
                        size=(74, 133), mode='bilinear', align_corners=False)
    x32 = frames.permute(0, 3, 1, 2).float() / 255
    cpu32 = F.interpolate((x32 - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1), size=(74, 133), mode='bilinear',
                          align_corners=False)
    e_gpu, e_cpu = nerr(got.cpu(), ref), nerr(cpu32, ref)
    print("other constants: kernel %.3g, float32 CPU %.3g" % (e_gpu, e_cpu))
    assert e_gpu < max(TOL, 4 * e_cpu)
