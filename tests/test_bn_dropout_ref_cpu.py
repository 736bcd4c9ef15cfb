"""tests/bn_dropout_ref.py is right, its bounds bind, and the two entry points of csrc/bn_dropout.hip check their arguments.  No GPU.

(a) ``forward`` / ``backward`` in float64 equal torch.nn.BatchNorm1d + ReLU in float64 under autograd to 1e-12 of the magnitudes,
    on every case of the table: y, dz, dgamma, dbeta, running_mean and running_var (the unbiased factor included), for momentum
    0.1, 1.0 and None (the cumulative average) over three consecutive calls.
(b) The mask restatement: the numpy form equals a plain-Python-int form, the kept share is within 4 sigma of 1 - p, p = 2^-24 drops
    exactly the elements whose 24 bits are 0, and the mask follows the seed.
(c) The knife set (|u_ref| <= 32 u u_mag, where a float32 ReLU decision may differ from the float64 one) holds at most 1e-3 of
    each case's elements: a condition on the committed inputs.
(d) The sequential float32 comparator against the float64 reference: finite ratios, printed; and six deliberately wrong formulas
    each leave max(16 u, 4 x comparator) on some case.
(e) Argument checks of mpnhip_bn_relu_dropout_forward / _backward before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import bn_dropout_ref as B
from mpntrackseg_amd import capi

U = B.U
PIN = 1e-12
FWD_KEYS = ("y", "mean", "invstd", "running_mean", "running_var")
BWD_KEYS = ("dz", "dgamma", "dbeta")
IDS = ["%dx%d" % c for c in B.CASES]


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("momentum", [0.1, 1.0, None])
@pytest.mark.parametrize("m,n", B.CASES, ids=IDS)
def test_reference_equals_float64_torch(m, n, momentum):
    inp = B.inputs(m, n)
    bn = torch.nn.BatchNorm1d(n, eps=B.EPS, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(inp["gamma"]).double())
        bn.bias.copy_(torch.from_numpy(inp["beta"]).double())
        bn.running_mean.copy_(torch.from_numpy(inp["running_mean"]).double())
        bn.running_var.copy_(torch.from_numpy(inp["running_var"]).double())
    rm, rv = inp["running_mean"].astype(np.float64), inp["running_var"].astype(np.float64)
    for call in range(3):
        z = inp["z"] * np.float32(1 + call)
        mom = momentum if momentum is not None else 1.0 / (call + 1)
        f = B.forward(z, inp["gamma"], inp["beta"], rm, rv, mom)
        b = B.backward(inp["dy"], f)
        mag = B.magnitudes(z, f, b, inp["gamma"], inp["beta"], rm, rv, mom)
        zt = torch.from_numpy(z).double().requires_grad_(True)
        bn.zero_grad()
        yt = torch.relu(bn(zt))
        (yt * torch.from_numpy(inp["dy"]).double()).sum().backward()
        got = dict(y=yt.detach().numpy(), dz=zt.grad.numpy(), dgamma=bn.weight.grad.numpy(), dbeta=bn.bias.grad.numpy(),
                   running_mean=bn.running_mean.numpy(), running_var=bn.running_var.numpy())
        for k, v in got.items():
            ref = f[k] if k in f else b[k]
            assert B.worst_ratio(v, ref, mag[k]) <= PIN, (k, call)
        assert int(bn.num_batches_tracked) == call + 1
        rm, rv = f["running_mean"], f["running_var"]


def test_reference_without_affine_relu_or_statistics():
    inp = B.inputs(513, 64)
    z = torch.from_numpy(inp["z"]).double().requires_grad_(True)
    bn = torch.nn.BatchNorm1d(64, eps=B.EPS, affine=False, track_running_stats=False).double().train()
    (bn(z) * torch.from_numpy(inp["dy"]).double()).sum().backward()
    f = B.forward(inp["z"], relu=False)
    b = B.backward(inp["dy"], f)
    mag = B.magnitudes(inp["z"], f, b)
    assert f["running_mean"] is None and f["running_var"] is None and f["active"].all()
    assert B.worst_ratio(bn(z).detach().numpy(), f["y"], mag["y"]) <= PIN and B.worst_ratio(z.grad.numpy(), b["dz"], mag["dz"]) <= PIN


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("seed", [0, 1234, 2 ** 63 + 5, 2 ** 64 - 1])
def test_the_two_mask_restatements_agree(seed):
    m, n = 513, 65
    bits = B.keep_bits(seed, m, n)
    assert bits.min() >= 0 and bits.max() < 1 << 24
    idx = np.unique(np.concatenate([np.arange(100), np.arange(m * n - 100, m * n), np.floor(B.synth.uniform01(9, 200) * m * n).astype(np.int64)]))
    for p in (0.3, 0.5, 2.0 ** -24, 0.999):
        keep = B.keep_mask(seed, m, n, p).reshape(-1)
        assert all(bool(keep[i]) == B.keep_one(seed, i, p) for i in idx)
        share, sigma = keep.mean(), np.sqrt(p * (1 - p) / keep.size)
        assert abs(share - (1 - float(np.float32(p)))) <= 4 * sigma + 2.0 ** -24, (p, share)


def test_the_smallest_p_drops_exactly_the_zero_bits_and_the_mask_follows_the_seed():
    m, n = 2049, 4099   # 8.4e6 elements: about half a chance of a zero among 2^24 values, so plant the check on the bits
    bits = B.keep_bits(7, m, n)
    assert (B.keep_mask(7, m, n, 2.0 ** -24) == (bits != 0)).all()
    assert B.keep_mask(7, m, n, 0.0).all()
    assert (B.keep_mask(7, 16, 16, 0.999) == (B.keep_bits(7, 16, 16) >= np.float32(0.999) * 2.0 ** 24)).all()
    a, b = B.keep_mask(1, 513, 65, 0.5), B.keep_mask(2, 513, 65, 0.5)
    assert 0.4 < (a != b).mean() < 0.6
    assert (B.keep_mask(1, 513, 65, 0.5) == a).all()
    # idx = r n + c: the [m, n] mask is the flat sequence, row-major
    assert (B.keep_mask(1, 513 * 65, 1, 0.5).reshape(513, 65) == a).all()


def test_dropout_scale_is_formed_in_float32():
    """1 / (1 - p) from the float32 p in float32 operations (the entry points' ``1.f / (1.f - dropout_p)``); at p = 0.999 that is
    NOT float32(1 / (1 - 0.999)): 0.999 is not a float32"""
    for p in (0.3, 0.5, 2.0 ** -24, 0.999):
        assert B.scale32(p) == np.float32(1.0 / (1.0 - float(np.float32(p))))
    assert B.scale32(0.999) != np.float32(1.0 / (1.0 - 0.999))


# ------------------------------------------------------------------------------------------------ (c)
def test_knife_set_condition():
    counts = []
    for m, n in B.CASES:
        inp = B.inputs(m, n)
        f = B.forward(inp["z"], inp["gamma"], inp["beta"])
        k = B.knife_set(f, B.magnitudes(inp["z"], f, None, inp["gamma"], inp["beta"]))
        counts.append(int(k.sum()))
        assert k.sum() <= 1e-3 * k.size, (m, n, int(k.sum()))
    print("knife-set elements per case:", counts)
    assert counts == [0, 0, 0, 9, 14, 10, 38, 9]


def test_the_inputs_hold_what_the_kernels_branch_on():
    assert {m for m, _ in B.CASES} >= {511, 512, 513, 1025, 2049} and {n for _, n in B.CASES} >= {1, 63, 64, 65, 130}
    inp = B.inputs(513, 64)
    assert (inp["z"][:, 5] == 0.5).all() and inp["gamma"][6] == 0 and inp["gamma"][0] < 0 and inp["gamma"][7] < 0 and inp["gamma"][1] > 0
    assert abs(inp["z"][:, 2].mean() + 1000) < 1 and abs(inp["z"][:, 1].mean() - 10) < 1 and inp["z"][:, 3].std() < 2e-3 < 20 < inp["z"][:, 4].std()


# ------------------------------------------------------------------------------------------------ (d)
def case_reference(m, n, **kw):
    """float64 reference with its own decisions, the comparator with THOSE decisions, magnitudes"""
    inp = B.inputs(m, n)
    args = dict(gamma=inp["gamma"], beta=inp["beta"], running_mean=inp["running_mean"], running_var=inp["running_var"])
    act = B.forward(inp["z"], **dict(args, **kw))["active"]
    ref, cmp, mag, _ = B.reference(inp, FWD_KEYS + BWD_KEYS, active=act, **kw)
    return inp, args, act, ref, cmp, mag


@pytest.mark.parametrize("m,n", B.CASES, ids=IDS)
def test_sequential_float32_comparator(m, n):
    inp, args, act, ref, cmp, mag = case_reference(m, n)
    for k in FWD_KEYS + BWD_KEYS:
        r = B.worst_ratio(cmp[k], ref[k], mag[k])
        print("%dx%d %-12s float32 sequential %8.2f u (bound %.1f u)" % (m, n, k, r / U, B.bound(r) / U))
        assert np.isfinite(r)
        assert cmp[k].dtype == np.float32
    if n > 6:   # what the GPU test asserts bit for bit, of the comparator
        relu_beta = np.maximum(inp["beta"], 0)
        assert (cmp["mean"][5] == 0.5) and (cmp["y"][:, 5] == relu_beta[5]).all() and (cmp["y"][:, 6] == relu_beta[6]).all()
        assert not cmp["dz"][:, 6].any()


def mutant_ratio(got, ref, mag):
    """worst_ratio; a result that is not finite (a negative raw-moment variance) or not 0 where it must be is as wrong as can be"""
    with np.errstate(invalid="ignore"):
        try:
            return B.worst_ratio(got, ref, mag)
        except AssertionError:
            return np.inf


def violates(keys, got, ref, cmp, mag):
    return [k for k in keys if mutant_ratio(got[k], ref[k], mag[k]) > B.bound(B.worst_ratio(cmp[k], ref[k], mag[k]))]


@pytest.mark.parametrize("mutant,dtype,key", [("biased_running_var", np.float64, "running_var"), ("raw_moment_var", np.float32, "invstd"),
                                              ("no_xh_term", np.float64, "dz"), ("mean_over_m_minus_1", np.float64, "dz")])
def test_mutants_leave_the_bounds(mutant, dtype, key):
    """each wrong formula, evaluated with the reference's decisions, is outside the bound of ``key`` on some case; the raw-moment
    variance E[z^2] - mu^2 is wrong only in float32, and there on the columns shifted by -1000"""
    hit = []
    for m, n in B.CASES:
        inp, args, act, ref, cmp, mag = case_reference(m, n)
        f = B.forward(inp["z"], active=act, dtype=dtype, mutant=mutant, **args)
        got = dict(f, **B.backward(inp["dy"], f, mutant=mutant))
        bad = violates(FWD_KEYS + BWD_KEYS, got, ref, cmp, mag)
        print(mutant, (m, n), bad)
        if key in bad:
            hit.append((m, n))
            if mutant == "raw_moment_var":
                err = np.abs(got["invstd"] - ref["invstd"]) / ref["invstd"]
                assert np.argmax(np.where(np.isfinite(err), err, np.inf)) % 8 == 2
    assert hit, mutant
    if mutant in ("no_xh_term", "mean_over_m_minus_1"):
        assert (1025, 130) in hit and (513, 64) in hit


@pytest.mark.parametrize("m,n", [(513, 64), (1025, 130)])
def test_dropout_mutants_leave_the_bounds(m, n):
    """BatchNorm + ReLU + dropout at p = 0.3: the mask indexed c m + r, and the scale applied twice in the backward"""
    p, seed = 0.3, 1234
    keep = B.keep_mask(seed, m, n, p)
    inp, args, act, ref, cmp, mag = case_reference(m, n, p=p, keep=keep)
    assert not violates(FWD_KEYS + BWD_KEYS, cmp, ref, cmp, mag)
    wrong = B.keep_mask(seed, n, m, p).T   # keep[r, c] from idx = c m + r
    assert wrong.shape == keep.shape and (wrong != keep).mean() > 0.3
    f = B.forward(inp["z"], active=act, p=p, keep=wrong, **args)
    with pytest.raises(AssertionError, match="exactly 0"):   # a kept element where the reference drops
        B.worst_ratio(f["y"], ref["y"], mag["y"])
    assert "dz" in violates(BWD_KEYS, B.backward(inp["dy"], f), ref, cmp, mag)
    f = B.forward(inp["z"], active=act, p=p, keep=keep, **args)
    assert violates(BWD_KEYS, B.backward(inp["dy"], f, mutant="scale_twice"), ref, cmp, mag) == list(BWD_KEYS)


# ------------------------------------------------------------------------------------------------ (e)
def test_entry_points_argument_checks_without_gpu():
    """Everything below returns before a kernel is launched (the non-null pointers are host dummies that are never dereferenced)."""
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    big = 1 << 30
    need = l.mpnhip_bn_dropout_workspace_bytes(513, 64)
    assert need == (2 * 2 * 64 + 2 * 64) * 4 and l.mpnhip_bn_dropout_workspace_bytes(512, 64) == (2 * 64 + 2 * 64) * 4
    assert l.mpnhip_bn_dropout_workspace_bytes(0, 64) == 0 and l.mpnhip_bn_dropout_workspace_bytes(5, 0) == 0

    def fwd(m=513, n=64, use_bn=1, drop=0.3, z=p, y=p, mean=p, invstd=p, ws=p, nbytes=big):
        return l.mpnhip_bn_relu_dropout_forward(z, m, n, use_bn, p, p, p, p, 0.1, 1e-5, 1, drop, 7, y, mean, invstd, ws, nbytes, None)

    def bwd(m=513, n=64, use_bn=1, drop=0.3, dy=p, z=p, dz=p, mean=p, invstd=p, ws=p, nbytes=big):
        return l.mpnhip_bn_relu_dropout_backward(dy, z, m, n, use_bn, p, p, mean, invstd, 1, drop, 7, dz, p, p, ws, nbytes, None)

    for fn, name, nulls in ((fwd, b"bn_relu_dropout_forward", ("z", "y")), (bwd, b"bn_relu_dropout_backward", ("dy", "z", "dz"))):
        assert fn(m=0) == 0 and fn(m=0, use_bn=0, ws=None, nbytes=0, **{k: None for k in nulls}) == 0   # no rows: a successful no-op
        for bad in (dict(n=0), dict(n=-1), dict(m=-1), dict(drop=1.0), dict(drop=-0.25), dict(drop=float("nan"))) \
                + tuple({k: None} for k in nulls) + tuple({k: None, "use_bn": 0} for k in nulls) \
                + (dict(mean=None), dict(invstd=None), dict(ws=None), dict(nbytes=need - 1), dict(ws=None, nbytes=0)):
            assert fn(**bad) != 0, (name, bad)
            assert name in l.mpnhip_last_error(), (name, bad, l.mpnhip_last_error())
    for fn, name in ((fwd, b"bn_relu_dropout_forward"), (bwd, b"bn_relu_dropout_backward")):
        assert fn(m=1) != 0 and name in l.mpnhip_last_error() and b"more than one row" in l.mpnhip_last_error()
    assert fwd(drop=1.0) != 0 and b"[0, 1)" in l.mpnhip_last_error()
    assert fwd(nbytes=need - 1) != 0 and b"workspace" in l.mpnhip_last_error()
