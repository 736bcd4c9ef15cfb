"""mpnhip_bn_relu_dropout_forward / _backward (csrc/bn_dropout.hip) through the C ABI against tests/bn_dropout_ref.py: numpy float64
on the same float32 inputs, every element compared.  tests/test_bn_dropout_ref_cpu.py pins that reference against float64 torch
and shows that the bounds below bind (six wrong formulas each leave them).

Bounds, u = 2^-24, every error per element against the MAGNITUDE of bn_dropout_ref.magnitudes (the formulas cancel):

  |got - ref| <= max(16 u, 4 x the ratio of the sequential float32 evaluation of the same case) * magnitude

16 u counts the roundings of a short float32 chain, it is not a measurement; the comparator accumulates every column sum row by
row in float32, an order no better than the kernels' (4 row lanes x chunks of 512 rows, then the chunks in order).  Where the
reference is exactly 0 (an element the mask drops) the result must be exactly 0.

ReLU decisions are pinned, not excluded: the device's decisions are read from a forward with p = 0 (y > 0), may differ from the
float64 ones only where |u_ref| <= 32 u u_mag (at most 1e-3 of a case's elements, asserted of the inputs on the CPU), and the
reference's forward AND backward are evaluated with them.

The dropout scale is 1 / (1 - p) formed in float32 from the float32 p, as the entry points form it (at p = 0.999 that is
1000.0129, not 1000: 0.999 is not a float32).

MEASURED on the MI355X (worst ratio of each group; the sequential float32 comparator in brackets):

                                      y             mean          invstd        running_mean  running_var   dz           dgamma       dbeta
  table, BatchNorm + ReLU (8 cases)   5.80 (10.44)  4.00 (10.78)  2.91 (10.15)  8.01 (16.57)  3.08 (11.90)  4.01 (8.73)  2.52 (2.85)  0.99 (1.23)
  ... + dropout 0.3 (2 cases)         5.67 (10.58)  4.00 (10.78)  2.43 (11.70)  8.01 (16.57)  2.80 (11.17)  3.79 (9.14)  0.73 (2.72)  0.55 (2.09)
  variants (7 x 2 cases)              116.2 (153.7) 4.00 (10.78)  2.23 (7.17)   170.4 (217.4) 3.40 (16.65)  3.58 (6.33)  2.52 (2.85)  1.67 (1.67)
  two consecutive calls               at most 0.20 of the accumulated bound
  ReLU alone, the mask (48 (shape, p, seed) triples), columns 0 / 63 / 64 / 129 alone, the same call twice: bit for bit

The two large figures of the variants (gamma and beta both null: y; momentum 1: running_mean) belong to column 6, whose mean is a
cancelling sum (|mu| << mean |z|): with beta null nothing but |gamma| (|z| + |mu|) invstd stands under an element near the mean,
and with momentum 1 nothing but |mu| under running_mean, while the error of mu is a few u of mean |z|.  Every float32 evaluation
has it, the comparator more than the kernels (it is why the bound carries the 4 x comparator term); no kernel exceeded
max(16 u, 4 x comparator), and none needed a fix.

What the file did change: mpnhip_bn_relu_dropout_backward accepted use_bn with a single row, which its forward refuses (BatchNorm1d
in training mode needs more than one value per channel); it refuses it now with the forward's words.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_dropout_ref as B
from mpntrackseg_amd import capi, modular, synth

pytestmark = pytest.mark.gpu
U = B.U
SENT = 64
SENT_VALUE = -7.25
FWD_KEYS = ("y", "mean", "invstd", "running_mean", "running_var")
BWD_KEYS = ("dz", "dgamma", "dbeta")
IDS = ["%dx%d" % c for c in B.CASES]
dev = lambda: torch.device("cuda:0")


def on(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev())


class Guarded:
    """an output buffer of ``shape`` with 64 sentinel floats behind it"""

    def __init__(self, shape, init=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((self.n + SENT,), SENT_VALUE, dtype=torch.float32, device=dev())
        self.t = self.buf[:self.n].view(self.shape)
        if init is not None:
            self.t.copy_(on(init))
        else:
            self.t.fill_(float("nan"))   # an element the kernel leaves out stays NaN

    def get(self):
        tail = self.buf[self.n:].cpu().numpy()
        assert tail.tobytes() == np.full(SENT, SENT_VALUE, np.float32).tobytes(), "written behind the buffer"
        return self.t.cpu().numpy()


class Workspace:
    """exactly mpnhip_bn_dropout_workspace_bytes, 256 guard bytes behind"""

    def __init__(self, m, n):
        self.need = capi.load().mpnhip_bn_dropout_workspace_bytes(m, n)
        self.buf = torch.full((self.need + 256,), 0xA5, dtype=torch.uint8, device=dev())

    def check(self):
        assert (self.buf[self.need:] == 0xA5).all(), "written behind the workspace"


def dev_forward(z, gamma=None, beta=None, running_mean=None, running_var=None, momentum=0.1, use_bn=True, relu=True, p=0.0, seed=0,
                state=None):
    """one mpnhip_bn_relu_dropout_forward -> dict of numpy results plus what dev_backward needs.  ``state``: the dict of an earlier
    call whose running-statistics buffers are updated again."""
    lib = capi.load()
    m, n = z.shape
    zt, g, b = on(z), on(gamma), on(beta)
    y = Guarded((m, n))
    mean, invstd = (Guarded((n,)), Guarded((n,))) if use_bn else (None, None)
    if state is not None:
        rm, rv = state["_rm"], state["_rv"]
    else:
        rm = Guarded((n,), running_mean) if running_mean is not None else None
        rv = Guarded((n,), running_var) if running_var is not None else None
    ws = Workspace(m, n) if use_bn else None
    gp = lambda x: capi.ptr(x.t) if x is not None else None
    capi.check(lib.mpnhip_bn_relu_dropout_forward(capi.ptr(zt), m, n, int(use_bn), capi.ptr(g), capi.ptr(b), gp(rm), gp(rv), float(momentum),
                                                  B.EPS, int(relu), float(p), C.c_uint64(seed), capi.ptr(y.t), gp(mean), gp(invstd),
                                                  capi.ptr(ws.buf) if ws else None, ws.need if ws else 0, capi.stream_ptr()),
               "mpnhip_bn_relu_dropout_forward")
    torch.cuda.synchronize()
    if ws:
        ws.check()
    assert zt.cpu().numpy().tobytes() == np.ascontiguousarray(z, np.float32).tobytes()   # the input is read only
    out = dict(y=y.get(), _z=zt, _g=g, _b=b, _mean=mean, _invstd=invstd, _rm=rm, _rv=rv, _cfg=(use_bn, relu, p, seed))
    out.update(mean=mean.get() if mean else None, invstd=invstd.get() if invstd else None,
               running_mean=rm.get() if rm else None, running_var=rv.get() if rv else None)
    return out


def dev_backward(dy, fwd):
    lib = capi.load()
    use_bn, relu, p, seed = fwd["_cfg"]
    m, n = fwd["y"].shape
    dz = Guarded((m, n))
    dg, db = (Guarded((n,)), Guarded((n,))) if use_bn else (None, None)
    ws = Workspace(m, n) if use_bn else None
    gp = lambda x: capi.ptr(x.t) if x is not None else None
    capi.check(lib.mpnhip_bn_relu_dropout_backward(capi.ptr(on(dy)), capi.ptr(fwd["_z"]), m, n, int(use_bn), capi.ptr(fwd["_g"]),
                                                   capi.ptr(fwd["_b"]), gp(fwd["_mean"]), gp(fwd["_invstd"]), int(relu), float(p),
                                                   C.c_uint64(seed), capi.ptr(dz.t), gp(dg), gp(db), capi.ptr(ws.buf) if ws else None,
                                                   ws.need if ws else 0, capi.stream_ptr()), "mpnhip_bn_relu_dropout_backward")
    torch.cuda.synchronize()
    if ws:
        ws.check()
    return dict(dz=dz.get(), dgamma=dg.get() if dg else None, dbeta=db.get() if db else None)


def pinned_decisions(inp, args):
    """the device's ReLU decisions (forward with p = 0: y > 0); they differ from the float64 ones inside the knife set only"""
    act = dev_forward(inp["z"], **args)["y"] > 0
    f = B.forward(inp["z"], **args)
    knife = B.knife_set(f, B.magnitudes(inp["z"], f, None, args.get("gamma"), args.get("beta")))
    differ = act != f["active"]
    # u_ref exactly 0 (beta null: the constant column's xh = 0, the column of gamma = 0) is no rounding question: xh = 0 or
    # gamma = 0 hold on the device as well, the element is inactive there, and it does not count towards the knife set
    zero = f["u"] == 0
    knife &= ~zero
    print("ReLU decisions: %d differ from float64, knife set %d of %d, u_ref = 0 at %d" % (differ.sum(), knife.sum(), knife.size, zero.sum()))
    assert not act[zero].any() and not (differ & ~knife).any() and knife.sum() <= 1e-3 * knife.size
    return act


def run_and_check(label, inp, keys=FWD_KEYS + BWD_KEYS, relu=True, p=0.0, seed=0, **over):
    """forward and backward of one case on the device against the pinned float64 reference -> (got, ref, mag, ratios)"""
    args = dict(gamma=inp["gamma"], beta=inp["beta"], running_mean=inp["running_mean"], running_var=inp["running_var"], momentum=0.1)
    args.update(over)
    act = pinned_decisions(inp, dict(args, relu=True)) if relu else None
    keep = B.keep_mask(seed, *inp["z"].shape, p) if p > 0 else None
    fwd = dev_forward(inp["z"], relu=relu, p=p, seed=seed, **args)
    got = dict(fwd, **dev_backward(inp["dy"], fwd))
    keys = [k for k in keys if got[k] is not None]
    ref, cmp, mag, _ = B.reference(inp, keys, relu=relu, active=act, p=p, keep=keep, **args)
    ratios = B.check(label, got, ref, cmp, mag, keys)
    if keep is not None:
        assert not got["y"][~keep].any()   # (dz is not 0 there: the two column means reach every row)
    return got, ref, mag, ratios


# ------------------------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("m,n", B.CASES, ids=IDS)
def test_table_against_float64(m, n):
    inp = B.inputs(m, n)
    got, ref, mag, _ = run_and_check("bn relu %dx%d" % (m, n), inp)
    relu_beta = np.maximum(inp["beta"], 0)
    if n > 5:   # the constant column: var = 0, xh = 0
        assert got["mean"][5] == np.float32(0.5) and got["y"][:, 5].tobytes() == np.full(m, relu_beta[5], np.float32).tobytes()
    if n > 6:   # gamma = 0
        assert got["y"][:, 6].tobytes() == np.full(m, relu_beta[6], np.float32).tobytes() and not got["dz"][:, 6].any()


# ------------------------------------------------------------------------------------------------ 2. variants
VARIANTS = {
    "gamma_null": dict(gamma=None), "beta_null": dict(beta=None), "both_null": dict(gamma=None, beta=None), "no_relu": dict(relu=False),
    "no_running": dict(running_mean=None, running_var=None), "momentum_0": dict(momentum=0.0), "momentum_1": dict(momentum=1.0),
}


@pytest.mark.parametrize("m,n", [(513, 64), (5, 64)], ids=["513x64", "5x64"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variants(variant, m, n):
    inp = B.inputs(m, n)
    got, ref, mag, _ = run_and_check("%s %dx%d" % (variant, m, n), inp, **VARIANTS[variant])
    if variant == "no_running":
        assert got["running_mean"] is None and got["running_var"] is None
    if variant == "momentum_0":
        assert got["running_mean"].tobytes() == inp["running_mean"].tobytes() and got["running_var"].tobytes() == inp["running_var"].tobytes()
    if variant == "momentum_1":
        assert got["running_mean"].tobytes() == got["mean"].tobytes()


@pytest.mark.parametrize("m,n", [(513, 64), (5, 64)], ids=["513x64", "5x64"])
def test_two_consecutive_calls_accumulate_the_running_statistics(m, n):
    """second call on z x 1.5 + 0.25 into the same buffers: against the reference iterated on its own float64 state, within the
    first call's bound carried through (1 - momentum) plus the second call's"""
    inp = B.inputs(m, n)
    mom = 0.1
    args = dict(gamma=inp["gamma"], beta=inp["beta"], momentum=mom)
    z2 = inp["z"] * np.float32(1.5) + np.float32(0.25)
    first = dev_forward(inp["z"], running_mean=inp["running_mean"], running_var=inp["running_var"], **args)
    second = dev_forward(z2, state=first, **args)
    allowed = None
    rm, rv = inp["running_mean"], inp["running_var"]
    for name, z, got in (("first", inp["z"], first), ("second", z2, second)):
        ref, cmp, mag, _ = B.reference(dict(inp, z=z, running_mean=rm, running_var=rv), ("running_mean", "running_var"), **args)
        bnd = {k: B.bound(B.worst_ratio(cmp[k], ref[k], mag[k])) * mag[k] for k in ref}
        allowed = bnd if allowed is None else {k: (1 - mom) * allowed[k] + bnd[k] for k in bnd}
        for k in ref:
            err = np.abs(got[k] - ref[k])
            print("%s call: %s worst error / accumulated bound %.3f" % (name, k, (err / allowed[k]).max()))
            assert (err <= allowed[k]).all()
        rm, rv = ref["running_mean"], ref["running_var"]
    assert second["running_mean"].tobytes() != first["running_mean"].tobytes()


# ------------------------------------------------------------------------------------------------ 3. without BatchNorm
@pytest.mark.parametrize("m,n", [(1, 1), (3, 5), (513, 65)], ids=["1x1", "3x5", "513x65"])
def test_relu_alone_is_exact(m, n):
    """use_bn = 0, p = 0, no workspace, no statistics: y = max(z, 0), dz = where(z > 0, dy, 0) bit for bit"""
    z, dy = synth.normal(62, (m, n), stream=1), synth.normal(62, (m, n), stream=2)
    z.reshape(-1)[::5] = 0.0
    fwd = dev_forward(z, use_bn=False)
    assert fwd["y"].tobytes() == np.maximum(z, np.float32(0)).tobytes() and fwd["mean"] is None
    bwd = dev_backward(dy, fwd)
    assert bwd["dz"].tobytes() == np.where(z > 0, dy, np.float32(0)).tobytes() and bwd["dgamma"] is None


# ------------------------------------------------------------------------------------------------ 4. the mask
@pytest.mark.parametrize("m,n", [(1, 1), (3, 5), (513, 65)], ids=["1x1", "3x5", "513x65"])
def test_mask_bit_for_bit(m, n):
    """use_bn = 0, relu = 0, z = 1: y IS the mask times float32 1 / (1 - p); the backward regenerates the same mask"""
    z, dy = np.ones((m, n), np.float32), synth.normal(63, (m, n))
    for p in (0.3, 0.5, 2.0 ** -24, 0.999):
        scale = B.scale32(p)
        for seed in (0, 1234, 2 ** 63 + 5, 2 ** 64 - 1):
            keep = B.keep_mask(seed, m, n, p)
            fwd = dev_forward(z, use_bn=False, relu=False, p=p, seed=seed)
            assert fwd["y"].tobytes() == np.where(keep, scale, np.float32(0)).astype(np.float32).tobytes(), (p, seed)
            bwd = dev_backward(dy, fwd)
            assert bwd["dz"].tobytes() == np.where(keep, dy * scale, np.float32(0)).astype(np.float32).tobytes(), (p, seed)
    print("mask %dx%d: 16 (p, seed) pairs bit for bit; kept share at p = 0.3, seed 1234: %.4f" % (m, n, B.keep_mask(1234, m, n, 0.3).mean()))


# ------------------------------------------------------------------------------------------------ 5. everything together
@pytest.mark.parametrize("m,n", [(513, 64), (1025, 130)], ids=["513x64", "1025x130"])
def test_batchnorm_relu_dropout_together(m, n):
    inp = B.inputs(m, n)
    got, ref, mag, _ = run_and_check("bn relu dropout %dx%d" % (m, n), inp, p=0.3, seed=1234)
    keep = B.keep_mask(1234, m, n, 0.3)
    assert 0.25 < (~keep).mean() < 0.35 and (got["y"][keep] != 0).any()
    # the statistics do not see the mask
    plain = dev_forward(inp["z"], inp["gamma"], inp["beta"], inp["running_mean"], inp["running_var"])
    for k in ("mean", "invstd", "running_mean", "running_var"):
        assert plain[k].tobytes() == got[k].tobytes()


# ------------------------------------------------------------------------------------------------ 6. columns
def test_columns_do_not_see_each_other():
    m, n = 1025, 130
    inp = B.inputs(m, n)
    full = dev_forward(inp["z"], inp["gamma"], inp["beta"])
    full.update(dev_backward(inp["dy"], full))
    for c in (0, 63, 64, 129):
        one = dev_forward(np.ascontiguousarray(inp["z"][:, c:c + 1]), inp["gamma"][c:c + 1], inp["beta"][c:c + 1])
        one.update(dev_backward(np.ascontiguousarray(inp["dy"][:, c:c + 1]), one))
        for k in ("y", "dz"):
            assert torch.equal(torch.from_numpy(full[k][:, c]), torch.from_numpy(one[k][:, 0])), (k, c)
        for k in ("mean", "invstd", "dgamma", "dbeta"):
            assert torch.equal(torch.from_numpy(full[k][c:c + 1]), torch.from_numpy(one[k])), (k, c)


# ------------------------------------------------------------------------------------------------ 7. repeatability
def test_the_same_call_twice_gives_the_same_bits():
    inp = B.inputs(1025, 130)
    runs = []
    for _ in range(2):
        fwd = dev_forward(inp["z"], inp["gamma"], inp["beta"], inp["running_mean"], inp["running_var"], p=0.3, seed=99)
        fwd.update(dev_backward(inp["dy"], fwd))
        runs.append(b"".join(fwd[k].tobytes() for k in FWD_KEYS + BWD_KEYS))
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------ 8. the wrapper
def rel(a, b):   # tests/test_gpu_modular.py's measure
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max()))) if a.size else 0.0


class OneLayer(torch.nn.Module):
    def __init__(self, **bn):
        super().__init__()
        self.fc_layers = torch.nn.Sequential(torch.nn.Linear(20, 40), torch.nn.BatchNorm1d(40, **bn), torch.nn.ReLU())


@pytest.mark.parametrize("bn", [dict(momentum=None), dict(affine=False), dict(track_running_stats=False)],
                         ids=["momentum_none", "not_affine", "no_running_stats"])
def test_wrapper_follows_the_float64_module(bn):
    """modular.mlp_forward on Linear -> BatchNorm1d -> ReLU over three training steps: outputs, gradients, buffers and
    num_batches_tracked against the float64 module (the Linear in front is not this file's subject: rel < 1e-5).

    The Linear's bias gradient is sum_r dz, and behind a BatchNorm that sum is 0 identically (dz = c (du - mean du - xh mean(du xh))
    and sum_r xh = 0): the float64 module returns 1e-15, float32 returns the rounding of ~300 terms of size 1.  ``rel`` divides by
    max(1, |reference|), which is blind to that cancellation, so this one gradient is measured per column against
    max(1, sum_r |dz_ref|), the project's magnitude for a sum that cancels, at the same 1e-5."""
    import copy
    torch.manual_seed(3)
    net = OneLayer(**bn)
    if net.fc_layers[1].affine:
        net.fc_layers[1].weight.data.uniform_(0.5, 1.5)
        net.fc_layers[1].bias.data.normal_(0, 0.3)
    ref = copy.deepcopy(net).double().train()
    net = net.to(dev()).train()
    for step in range(3):
        x = torch.from_numpy(synth.normal(64 + step, (300 + step, 20)))
        w = torch.from_numpy(synth.normal(70 + step, (300 + step, 40)))
        xr = x.double().requires_grad_(True)
        ref.zero_grad()
        zr = ref.fc_layers[0](xr)
        zr.retain_grad()
        yr = ref.fc_layers[2](ref.fc_layers[1](zr))
        (yr * w.double()).sum().backward()
        xd = x.to(dev()).requires_grad_(True)
        net.zero_grad()
        y = modular.mlp_forward(net, xd)
        (y * w.to(dev())).sum().backward()
        worst = [rel(y, yr), rel(xd.grad, xr.grad)]
        for (k, p1), (_, p2) in zip(net.named_parameters(), ref.named_parameters()):
            assert p1.grad is not None, k
            if k == "fc_layers.0.bias":
                worst.append(float(((p1.grad.cpu().double() - p2.grad).abs() / zr.grad.abs().sum(0).clamp_min(1.0)).max()))
            else:
                worst.append(rel(p1.grad, p2.grad))
        bufs, rbufs = dict(net.named_buffers()), dict(ref.named_buffers())
        assert set(bufs) == set(rbufs) and (len(bufs) == 0) == (bn.get("track_running_stats") is False)
        for k in bufs:
            if k.endswith("num_batches_tracked"):
                assert int(bufs[k]) == int(rbufs[k]) == step + 1
            else:
                worst.append(rel(bufs[k], rbufs[k]))
        print("step %d: worst rel %.2e" % (step, max(worst)))
        assert max(worst) < 1e-5, worst
