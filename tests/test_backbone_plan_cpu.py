"""The launch plans of the two native ResNet50s (reid_net.ResNet and fpn_net.BackboneWithFPN over conv_affine.resnet_body_steps)
without a GPU: plans are built from CPU modules.

test_same_launches_as_recorded compares every plan, launch by launch, with tests/golden/backbone_launch_traces.json, which was
recorded from the tuple plans the two networks built on their own before they shared one builder: entry point, layer, buffers,
epilogue, geometry, which constants go in, the stage markers and the buffer sizes.

test_plan_is_sound walks each plan symbolically -- every buffer labelled with the convolution that last wrote it and the shape
of an image -- and holds every launch to the module graph: it reads what its module reads, in the shape its layer takes, never
writes what it reads, and what it writes fits the buffer."""
import json
import os

import pytest
import torch  # noqa: F401

from mpntrackseg_amd import fpn_net, reid_net
from mpntrackseg_amd.conv_affine import Launch, Stage

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_launch_traces.json")
REID_SIZES = [(128, 64), (97, 45)]
FPN_SIZES = [(64, 96), (40, 72)]


@pytest.fixture(scope="module")
def nets():
    return {"reid": reid_net.resnet50_fc256(10).eval(), "fpn": fpn_net.resnet50_fpn_backbone().eval(),
            "reid1111": reid_net.ResNet(10, 'xent', reid_net.Bottleneck, [1, 1, 1, 1], fc_dims=[16]).eval()}


def plan_of(net, H, W):
    native = net._native if net._native is not None else net.prepare_native()
    return native, net._plan(native, H, W)


def describe(net, native, plan, H, W):
    """the plan as names and integers, in the fixture's form"""
    mods = dict(net.named_modules())
    steps = []
    for st in plan["steps"]:
        if isinstance(st, Stage):
            steps.append({"stage": st.name, "buffer": st.buffer})
            continue
        assert isinstance(st, Launch) and st.kind in ("conv", "pool")
        c = st.layer
        d = {"entry": "pool" if st.kind == "pool" else ("up" if st.up is not None else "plain"), "layer": c["name"], "src": st.src,
             "dst": st.dst, "residual": st.residual, "relu": bool(st.relu)}
        for k in ("cin", "cout", "k", "stride", "H", "W"):
            d[k] = int(c[k])
        assert c["geometry"] == tuple(d[k] for k in ("cin", "cout", "H", "W", "k", "stride"))      # what the executor passes on
        assert c["weight"] is mods[c["name"]].weight
        d["up"] = [int(v) for v in st.up] if st.up is not None else None
        if st.kind != "pool":
            d["scale_absent"] = c["scale"] is None
            folded = native["affine"].get(c["name"], (None, None))
            assert c["scale"] is None or c["scale"] is folded[0]
            d["shift"] = "bn" if c["shift"] is folded[1] else ("bias" if c["shift"] is mods[c["name"]].bias else "?")
        steps.append(d)
    out = {"H": H, "W": W, "per_image": int(plan["per_image"]), "steps": steps}
    if "kept" in plan:
        out["kept"] = {k: int(v) for k, v in plan["kept"].items()}
    return out


@pytest.mark.parametrize("which, sizes", [("reid", REID_SIZES), ("fpn", FPN_SIZES)])
def test_same_launches_as_recorded(nets, which, sizes):
    with open(GOLDEN) as f:
        golden = json.load(f)[which]
    assert [(g["H"], g["W"]) for g in golden] == sizes
    for g, (H, W) in zip(golden, sizes):
        native, plan = plan_of(nets[which], H, W)
        got = describe(nets[which], native, plan, H, W)
        assert len(got["steps"]) == len(g["steps"])
        for i, (a, b) in enumerate(zip(got["steps"], g["steps"])):
            assert a == b, (which, H, W, i)
        assert got == g


def module_graph(body, prefix):
    """{conv name: (producer its module reads, producer of the residual or None)} of a ResNet body, in execution order, and the
    last convolution of each layer"""
    reads = {prefix + "conv1": ("input", None)}
    prev, last = "pool", []
    for li in range(1, 5):
        for bi, blk in enumerate(getattr(body, "layer%d" % li)):
            p = "%slayer%d.%d." % (prefix, li, bi)
            reads[p + "conv1"] = (prev, None)
            reads[p + "conv2"] = (p + "conv1", None)
            if blk.downsample is not None:
                reads[p + "downsample.0"] = (prev, None)
            reads[p + "conv3"] = (p + "conv2", p + "downsample.0" if blk.downsample is not None else prev)
            prev = p + "conv3"
        last.append(prev)
    return reads, last


def walk(net, which, H, W):
    native, plan = plan_of(net, H, W)
    if which == "fpn":
        reads, last = module_graph(net.body, "body.")
        shapes = net.level_shapes(H, W)
        for i in range(3, -1, -1):                           # top-down: a level's inner map needs the coarser one
            reads["fpn.inner_blocks.%d" % i] = (last[i], "fpn.inner_blocks.%d" % (i + 1) if i < 3 else None)
            reads["fpn.layer_blocks.%d" % i] = ("fpn.inner_blocks.%d" % i, None)
        capacity = dict(plan["kept"], **{str(i): 256 * shapes[i][0] * shapes[i][1] for i in range(4)})
        stages = dict(zip(("C2", "C3", "C4", "C5"), last), stem="pool", **{"inner%d" % i: "fpn.inner_blocks.%d" % i for i in range(4)})
        results = {str(i): "fpn.layer_blocks.%d" % i for i in range(4)}
        assert sorted(plan["kept"]) == ["c2", "c3", "c4", "c5"]
    else:
        reads, last = module_graph(net, "")
        (c, h, w), _ = net.output_shapes(H, W)
        capacity = {"f": c * h * w}
        stages = dict(zip(("layer1", "layer2", "layer3", "layer4"), last), stem="pool")
        results = {"f": last[-1]}
    capacity.update({i: plan["per_image"] for i in range(3)})
    holds = {"x": ("input", (3, H, W))}                      # buffer -> (who wrote it last, shape of an image)
    launched, staged = [], []
    for st in plan["steps"]:
        if isinstance(st, Stage):
            assert holds[st.buffer][0] == stages[st.name], st
            staged.append(st.name)
            continue
        c, where = st.layer, (which, H, W, st.layer["name"], st.kind)
        assert st.dst != st.src and st.dst != st.residual and st.dst != "x", where
        if st.kind == "pool":
            assert holds[st.src] == (c["name"], (c["cout"], c["Hout"], c["Wout"])) and st.residual is None and st.up is None, where
            shape, name = (c["cout"], (c["Hout"] - 1) // 2 + 1, (c["Wout"] - 1) // 2 + 1), "pool"
        else:
            want_src, want_res = reads[c["name"]]
            assert holds[st.src] == (want_src, (c["cin"], c["H"], c["W"])), where
            shape, name = (c["cout"], c["Hout"], c["Wout"]), c["name"]
            assert (c["Hout"], c["Wout"]) == ((c["H"] - 1) // c["stride"] + 1, (c["W"] - 1) // c["stride"] + 1), where
            lateral = name.startswith("fpn.inner_blocks.") and want_res is not None
            if want_res is None:
                assert st.residual is None and st.up is None, where
            elif lateral:                                     # the coarser inner map, read at the nearest-neighbour source cell
                level = int(name.rsplit(".", 1)[1])
                assert holds[st.residual] == (want_res, (256,) + tuple(shapes[level + 1])) and tuple(st.up) == tuple(shapes[level + 1]), where
            else:
                assert holds[st.residual] == (want_res, shape) and st.up is None, where
            launched.append(name)
        floats = shape[0] * shape[1] * shape[2]
        assert floats <= capacity[st.dst], where
        if st.dst in results:
            assert floats == capacity[st.dst], where
        holds[st.dst] = (name, shape)
    assert launched == list(reads)                            # every convolution of the module graph, once, in execution order
    assert staged == (["stem", "C2", "C3", "C4", "C5", "inner3", "inner2", "inner1", "inner0"] if which == "fpn"
                      else ["stem", "layer1", "layer2", "layer3", "layer4"])
    for buf, name in results.items():
        assert holds[buf][0] == name, (which, H, W, buf)


@pytest.mark.parametrize("which, H, W", [("reid", h, w) for h, w in REID_SIZES + [(33, 17)]] + [("fpn", h, w) for h, w in FPN_SIZES]
                         + [("reid1111", 37, 21)])
def test_plan_is_sound(nets, which, H, W):
    walk(nets[which], "fpn" if which == "fpn" else "reid", H, W)


def test_the_walk_catches_a_wrong_buffer(nets):
    """the check above is not vacuous: a plan whose conv3 writes the buffer its residual sits in is refused"""
    net = nets["reid"]
    native, plan = plan_of(net, 33, 17)
    steps = plan["steps"]
    i = next(i for i, st in enumerate(steps) if isinstance(st, Launch) and st.residual is not None)
    try:
        plan["steps"] = steps[:i] + [steps[i]._replace(dst=steps[i].residual)] + steps[i + 1:]
        with pytest.raises(AssertionError):
            walk(net, "reid", 33, 17)
    finally:
        plan["steps"] = steps
