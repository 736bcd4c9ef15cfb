"""The reference of csrc/bn_dropout.hip (training-mode BatchNorm1d -> ReLU -> Dropout behind one Linear, and its gradient) in numpy,
the case table of tests/test_gpu_bn_dropout.py and the bounds.  tests/test_bn_dropout_ref_cpu.py pins ``forward`` / ``backward``
in float64 against torch.nn.BatchNorm1d + ReLU under autograd and shows that the bounds bind.

  forward   mu = mean_r z, var = mean_r (z - mu)^2 (two passes), xh = (z - mu) / sqrt(var + eps), u = gamma xh + beta,
            y = [u > 0] u keep / (1 - p);  running_mean <- (1 - mom) running_mean + mom mu,
            running_var <- (1 - mom) running_var + mom var m / (m - 1)   (the UNBIASED variance)
  backward  du = dy keep / (1 - p) [u > 0];  dgamma = sum_r du xh, dbeta = sum_r du,
            dz = gamma invstd (du - mean_r du - xh mean_r(du xh))

``dtype`` chooses the arithmetic: float64 is the reference, float32 with ``sequential=True`` (column sums accumulated row by row)
the comparator of the bounds: an order no better than any the kernel may use.  ``active`` REPLACES the decision u > 0 (the GPU
tests pass the device's own decisions, so an u within rounding of 0 cannot make dz jump).  ``mutant`` names one deliberately
wrong formula (MUTANTS); the CPU test asserts that each of them leaves the bounds.

Errors are measured per element against the MAGNITUDES of ``magnitudes`` (sums of the absolute values of the terms: every formula
here cancels), in u = 2^-24, under max(16 u, 4 x the comparator's ratio of the same case)."""
import numpy as np

from mpntrackseg_amd import synth

U = 2.0 ** -24
FLOOR = 16 * U     # a short chain of float32 operations: a count of roundings, not a measurement
KNIFE = 32 * U     # |u_ref| <= KNIFE u_mag: where a float32 decision u > 0 may differ from the float64 one
EPS = 1e-5
SEED = 61
CASES = [(2, 1), (3, 5), (5, 64), (511, 65), (512, 63), (513, 64), (1025, 130), (2049, 7)]
MUTANTS = ("biased_running_var", "raw_moment_var", "no_xh_term", "mean_over_m_minus_1", "scale_twice")

_GOLDEN, _M1, _M2, _MASK64 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the dropout mask
def keep_bits(seed, m, n):
    """the 24 bits drop_keep compares against p, for idx = r n + c: splitmix64 of seed + (idx + 1) golden, top 24 bits -> [m, n]"""
    idx = np.arange(m * n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _MASK64) + (idx + np.uint64(1)) * np.uint64(_GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.int64).reshape(m, n)


def keep_mask(seed, m, n, p):
    """keep(r, c) of the kernels -> bool [m, n]: u = bits 2^-24 (exact in float32) >= float32(p)"""
    u = keep_bits(seed, m, n).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


def keep_one(seed, idx, p):
    """the same for ONE flat index in plain Python integers (no numpy wrap-around involved)"""
    z = ((int(seed) & _MASK64) + (int(idx) + 1) * _GOLDEN) & _MASK64
    z = ((z ^ (z >> 30)) * _M1) & _MASK64
    z = ((z ^ (z >> 27)) * _M2) & _MASK64
    z = z ^ (z >> 31)
    return (z >> 40) / 16777216.0 >= float(np.float32(p))


def scale32(p):
    """1 / (1 - p) as the entry points form it: in float32 from the float32 p"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


# ------------------------------------------------------------------------------------------------ inputs
def inputs(m, n):
    """-> dict(z [m, n], gamma [n], beta [n], dy [m, n], running_mean [n], running_var [n]) float32.  Columns by c % 8: 1 shifted
    by +10, 2 by -1000 (z - mu cancels), 3 scaled by 1e-3 (var of the order of eps), 4 by 30; column 5 constant 0.5 (var = 0);
    every 7th gamma negative, gamma[6] = 0."""
    z = synth.normal(SEED, (m, n), stream=1)
    c = np.arange(n) % 8
    z[:, c == 1] += np.float32(10.0)
    z[:, c == 2] -= np.float32(1000.0)
    z[:, c == 3] *= np.float32(1e-3)
    z[:, c == 4] *= np.float32(30.0)
    if n > 5:
        z[:, 5] = 0.5
    gamma = (0.5 + synth.uniform01(SEED, n, stream=2)).astype(np.float32)
    gamma[::7] *= -1
    if n > 6:
        gamma[6] = 0.0
    beta = synth.normal(SEED, (n,), stream=3, std=0.3)
    dy = synth.normal(SEED, (m, n), stream=4)
    rm = synth.normal(SEED, (n,), stream=5, std=0.3)
    rv = (0.5 + synth.uniform01(SEED, n, stream=6)).astype(np.float32)
    return dict(z=z, gamma=gamma, beta=beta, dy=dy, running_mean=rm, running_var=rv)


# ------------------------------------------------------------------------------------------------ forward / backward
def _colsum(a, sequential):
    if not sequential:
        return a.sum(0, dtype=a.dtype)
    s = np.zeros(a.shape[1], a.dtype)
    for r in range(a.shape[0]):
        s = s + a[r]
    return s


def forward(z, gamma=None, beta=None, running_mean=None, running_var=None, momentum=0.1, eps=EPS, use_bn=True, relu=True, p=0.0,
            keep=None, active=None, dtype=np.float64, sequential=False, mutant=None):
    """-> dict: y, u, xh, active (the decisions used) [m, n]; mean, invstd [n] (None without BatchNorm); running_mean, running_var
    (the updated copies, None where not given); and what ``backward`` needs.  ``keep`` bool [m, n] (None: nothing dropped)."""
    T = dtype
    z = np.asarray(z, T)
    m, n = z.shape
    g = None if gamma is None else np.asarray(gamma, T)
    b = None if beta is None else np.asarray(beta, T)
    out = dict(mean=None, invstd=None, running_mean=None, running_var=None)
    if use_bn:
        mu = _colsum(z, sequential) / T(m)
        d = z - mu
        ssq = _colsum(d * d, sequential)
        if mutant == "raw_moment_var":
            ssq = _colsum(z * z, sequential) - T(m) * mu * mu
        invstd = T(1) / np.sqrt(ssq / T(m) + T(eps))
        xh = d * invstd
        u = xh if g is None else g * xh
        u = u if b is None else u + b
        mom = T(momentum)
        if running_mean is not None:
            out["running_mean"] = (T(1) - mom) * np.asarray(running_mean, T) + mom * mu
        if running_var is not None:
            unbiased = ssq / T(m if mutant == "biased_running_var" else m - 1)
            out["running_var"] = (T(1) - mom) * np.asarray(running_var, T) + mom * unbiased
        out.update(mean=mu, invstd=invstd)
    else:
        xh, u = np.zeros_like(z), z
    if active is None:
        active = (u > 0) if relu else np.ones(z.shape, bool)
    scale = scale32(p) if T is np.float32 else 1.0 / (1.0 - float(np.float32(p)))
    factor = np.where(active, T(1), T(0))
    if keep is not None:
        factor = factor * np.where(keep, T(scale), T(0))
    out.update(y=u * factor, u=u, xh=xh, active=active, keep=keep, factor=factor, scale=T(scale), gamma=g, use_bn=use_bn, dtype=T,
               sequential=sequential)
    assert out["y"].dtype == T
    return out


def backward(dy, fwd, mutant=None):
    """-> dict(dz [m, n], dgamma, dbeta [n] (None without BatchNorm), du) in the dtype and summation order of ``fwd``"""
    T, seq = fwd["dtype"], fwd["sequential"]
    du = np.asarray(dy, T) * fwd["factor"]
    if mutant == "scale_twice":
        du = du * fwd["scale"]
    if not fwd["use_bn"]:
        return dict(dz=du, dgamma=None, dbeta=None, du=du)
    m = du.shape[0]
    xh, g = fwd["xh"], fwd["gamma"]
    sdu, sdx = _colsum(du, seq), _colsum(du * xh, seq)
    mdu = sdu / T(m - 1 if mutant == "mean_over_m_minus_1" else m)
    inner = du - mdu if mutant == "no_xh_term" else du - mdu - xh * (sdx / T(m))
    dz = (fwd["invstd"] if g is None else g * fwd["invstd"]) * inner
    assert dz.dtype == T
    return dict(dz=dz, dgamma=sdx, dbeta=sdu, du=du)


def magnitudes(z, fwd, bwd, gamma=None, beta=None, running_mean=None, running_var=None, momentum=0.1):
    """what the errors are measured against, from the float64 evaluation ``fwd`` / ``bwd`` (``bwd`` may be None): dict with the
    keys of the results.  y is 0 exactly where the mask drops (magnitude 0 there)."""
    z = np.asarray(z, np.float64)
    m, n = z.shape
    mag = {}
    kept = np.ones(z.shape, bool) if fwd["keep"] is None else fwd["keep"]   # (an element ReLU zeroes keeps its magnitude)
    if not fwd["use_bn"]:
        mag.update(u=np.abs(z), y=np.where(kept, np.abs(z) * fwd["scale"], 0.0))
        if bwd is not None:
            mag["dz"] = np.abs(bwd["du"])
        return mag
    g = np.ones(n) if gamma is None else np.abs(np.asarray(gamma, np.float64))
    b = np.zeros(n) if beta is None else np.abs(np.asarray(beta, np.float64))
    mu, invstd = fwd["mean"], fwd["invstd"]
    xh_mag = (np.abs(z) + np.abs(mu)) * invstd
    u_mag = g * xh_mag + b
    mag.update(u=u_mag, y=np.where(kept, u_mag * fwd["scale"], 0.0), mean=np.abs(z).mean(0), invstd=invstd)
    mom = float(momentum)
    if running_mean is not None:
        mag["running_mean"] = np.abs((1 - mom) * np.asarray(running_mean, np.float64)) + np.abs(mom * mu)
    if running_var is not None:
        unbiased = ((z - mu) ** 2).sum(0) / (m - 1)
        mag["running_var"] = np.abs((1 - mom) * np.asarray(running_var, np.float64)) + np.abs(mom * unbiased)
    if bwd is not None:
        adu = np.abs(bwd["du"])
        mag["dbeta"] = adu.sum(0)
        mag["dgamma"] = (adu * xh_mag).sum(0)
        mag["dz"] = g * invstd * (adu + adu.mean(0) + xh_mag * (adu * xh_mag).mean(0))
    return mag


# ------------------------------------------------------------------------------------------------ the bounds
def worst_ratio(got, ref, mag):
    """max |got - ref| / mag over the elements with mag > 0; where mag == 0 the reference is exactly 0 and so must ``got`` be"""
    got, ref, mag = (np.asarray(a, np.float64) for a in (got, ref, mag))
    zero = mag == 0
    assert not ref[zero].any()
    assert not got[zero].any(), "non-zero where the reference is exactly 0"
    assert np.isfinite(got).all()
    return float((np.abs(got - ref)[~zero] / mag[~zero]).max()) if not zero.all() else 0.0


def bound(cmp_ratio):
    """max(16 u, 4 x the comparator's ratio of the case)"""
    return max(FLOOR, 4.0 * cmp_ratio)


def knife_set(fwd, mag):
    """bool [m, n]: |u_ref| <= 32 u u_mag"""
    return np.abs(fwd["u"]) <= KNIFE * mag["u"]


def reference(inp, keys, **kw):
    """the float64 results and the sequential float32 comparator's of one case, and the magnitudes, for the result names ``keys``
    -> (ref, cmp, mag): dicts.  ``kw``: forward's arguments (gamma / beta / running statistics default to the inputs')."""
    args = dict(gamma=inp["gamma"], beta=inp["beta"], running_mean=inp["running_mean"], running_var=inp["running_var"])
    args.update(kw)
    out = []
    for T, seq in ((np.float64, False), (np.float32, True)):
        f = forward(inp["z"], dtype=T, sequential=seq, **args)
        b = backward(inp["dy"], f)
        out.append((f, b))
    (f, b) = out[0]
    mag = magnitudes(inp["z"], f, b, args["gamma"], args["beta"], args["running_mean"], args["running_var"], args.get("momentum", 0.1))
    merged = [dict((k, (fb[0] if k in fb[0] else fb[1])[k]) for k in keys) for fb in out]
    return merged[0], merged[1], mag, f


def check(label, got, ref, cmp, mag, keys):
    """every result ``keys`` of ``got`` against ``ref`` under max(16 u, 4 x comparator) of its magnitude; prints kernel ratio,
    comparator ratio and bound -> {key: (ratio, comparator ratio)} in u"""
    res, bad = {}, []
    for k in keys:
        r, c = worst_ratio(got[k], ref[k], mag[k]), worst_ratio(cmp[k], ref[k], mag[k])
        print("%s: %-12s kernel %7.2f u, float32 sequential %7.2f u (bound %.1f u)" % (label, k, r / U, c / U, bound(c) / U))
        res[k] = (r / U, c / U)
        if not r <= bound(c):
            bad.append((k, r / U, bound(c) / U))
    assert not bad, (label, bad)
    return res
