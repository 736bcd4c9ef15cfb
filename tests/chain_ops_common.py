"""What the operator tests of the fused chain kernels share (tests/test_gpu_chain_ops.py, _edge.py, _bf16.py): guarded device buffers, the
error report and its bound, the decision rule, the hand-built edge lists and the per-edge weights.  Test infrastructure only."""
import ctypes as C

import numpy as np
import torch

import segment_ref as SR
from mpntrackseg_amd import capi, synth

dev = lambda: torch.device("cuda:0")
GUARD = 3          # guard rows in front of and behind every output
FLOOR_TOL = 2e-6
MARGIN = 2e-5      # tests/test_gpu_pinned.py


class Guarded:
    """[GUARD + rows + GUARD, width] float32 on the device, all NaN (``fill``: the body holds these finite values instead -- a buffer
    the operator accumulates into or updates in place); the operator gets the address of row GUARD."""

    def __init__(self, rows, width, fill=None):
        self.rows, self.width = rows, width
        self.t = torch.full((rows + 2 * GUARD, width), float("nan"), dtype=torch.float32, device=dev())
        if fill is not None:
            self.t[GUARD:GUARD + rows] = torch.from_numpy(np.ascontiguousarray(fill, np.float32)).to(dev())

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 4 * GUARD * self.width)

    def result(self, name, nan_rows=None):
        """The body, after asserting that the guards are untouched, that the rows ``nan_rows`` (which the operator must not write)
        still hold their NaN prefill and that every other row is finite."""
        a = self.t.cpu().numpy()
        assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + self.rows:]).all(), (name, "guard rows written")
        body = a[GUARD:GUARD + self.rows]
        written = np.ones(self.rows, bool)
        if nan_rows is not None:
            written[nan_rows] = False
            assert np.isnan(body[~written]).all(), (name, "rows the operator must leave alone were written")
        assert np.isfinite(body[written]).all(), (name, "rows left unwritten or non-finite")
        return body


def with_nan_row(a):
    """``a`` with one NaN row appended, on the device: the operator is told about the rows of ``a`` only."""
    a = np.ascontiguousarray(a, np.float32)
    return torch.from_numpy(np.concatenate([a, np.full((1, a.shape[1]), np.nan, np.float32)])).to(dev())


def only_counter(name):
    c = {k: v for k, v in capi.path_counters(reset=True).items() if v}
    assert c == {name: 1}, c


def report(case, errs):
    for k, (e, e32) in errs.items():
        print("CHAIN_ERR %-34s %-7s kernel %.2e  float32-cpu %.2e" % (case, k, e, e32))
    for k, (e, e32) in errs.items():
        assert e <= max(FLOOR_TOL, 4.0 * e32), (case, k, e, e32)


def decision_exceptions(z64, got_positive):
    """Units whose decision differs from the float64 reference's; each must lie within MARGIN x rms of zero."""
    z = np.asarray(z64, np.float64)
    bad = (z > 0) != np.asarray(got_positive, bool)
    if bad.any():
        assert np.abs(z[bad]).max() <= MARGIN * np.sqrt((z ** 2).mean()), "a decision differs outside the margin"
    return int(bad.sum())


# ---- per-edge chain: widths, graphs with chosen direction groups, weights ----
WIDTHS = {"w128": (320, 64, 224, 128, 32), "w64": (160, 32, 112, 64, 16), "w32": (80, 16, 56, 32, 8), "p128": (304, 48, 208, 112, 24)}
# (edges with row < col, with row > col, self loops)
GROUPS = {"161-31-2": (161, 31, 2), "128-0-0": (128, 0, 0), "0-161-2": (0, 161, 2), "31-128-0": (31, 128, 0), "1-0-0": (1, 0, 0),
          "0-0-1": (0, 0, 1)}
N_NODES = 24
TAIL = 64          # pattern words behind the mask buffer
PATTERN = 0x5A5AA5A5


def edge_graph(n_out, n_in, n_self, seed):
    """[2, E] with exactly n_out edges row < col, n_in edges row > col and n_self self loops over N_NODES nodes, shuffled.  Node 3
    is the row of the first 70 edges of each group that has them; nodes 5 and 10 are never a row."""
    N = N_NODES
    u = synth.uniform01(seed, 4 * (n_out + n_in) + 16, stream=0)
    rows, cols, k = [], [], 0
    ok = [n for n in range(N) if n not in (5, 10)]
    for cnt, lo_side in ((n_out, False), (n_in, True)):
        for j in range(cnt):
            cand = [n for n in ok if (n >= 1 if lo_side else n <= N - 2)]
            r = 3 if j < 70 and cnt >= 100 else cand[int(u[k] * len(cand))]
            k += 1
            c = int(u[k] * r) if lo_side else r + 1 + int(u[k] * (N - 1 - r))
            k += 1
            rows.append(r)
            cols.append(c)
    for j in range(n_self):
        rows.append(7 + 9 * j)
        cols.append(7 + 9 * j)
    ei = np.array([rows, cols], np.int64).reshape(2, -1)
    ei = ei[:, np.argsort(synth.uniform01(seed, ei.shape[1], stream=1), kind="stable")]
    d = SR.directions(ei)
    assert ((d == 0).sum(), (d == 1).sum(), (d == 2).sum()) == (n_out, n_in, n_self)
    return ei


def make_weights(widths, reattach, seed):
    """The per-edge modules at these widths under the reference's state-dict names (kx = 2 dn: re-attached node features)."""
    he, de, hn, dn, hc = widths
    kx, ke = 2 * dn, (2 if reattach else 1) * de
    E, F, Cl = "MPNet.edge_model.edge_model.fc_layers.", "MPNet.node_model.flow_%s_model.fc_layers.", "classifier.edge_model.fc_layers."
    shapes = [(E + "0", he, 2 * kx + ke), (E + "2", de, he), (Cl + "0", hc, de), (Cl + "2", 1, hc)]
    for name in ("out", "in"):
        shapes += [(F % name + "0", hn, kx + de), (F % name + "2", dn, hn)]
    W = {}
    for i, (k, o, n) in enumerate(shapes):
        W[k + ".weight"] = synth.normal(seed, (o, n), stream=2 * i, std=(2.0 / n) ** 0.5)
        W[k + ".bias"] = synth.normal(seed, (o,), stream=2 * i + 1, std=0.1)
    return W
