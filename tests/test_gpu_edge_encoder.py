"""The edge encoder's MFMA kernel (csrc/edge_chain.hip: k_edge_encoder_mfma) at the widths launch_edge_encoder_mfma pads: every
combination of 32-column tiles other than (3, 3, 2) and (2, 2, 1) rides on the <3, 3, 2> instantiation with zero-padded tiles, and
synth only produces 36/36/32 and 72/72/64.  mpnhip_forward(save_for_backward = 1) on a model with such an encoder; both hidden
layers and the encoder output are read back (mpnhip_debug_saved, original edge order) and compared element by element with the float64
MLP of oracle/mpn_oracle.py on the same weights: |got - ref| <= 2e-6 max(1, max |ref|), the fp32-MFMA bound of tests/test_gpu_gemm.py.
Edge counts 1, 127, 128, 129 (the kernel's 128-row blocks) and 300.  The forward without saving (null hidden outputs) must give the
same logits."""
import numpy as np
import pytest
import torch

from mpntrackseg_amd import capi, synth
from mpntrackseg_amd.autograd import native_forward_saved
from mpntrackseg_amd.mpn import MOTMPNet
from oracle import mpn_oracle as O

pytestmark = pytest.mark.gpu
dev = lambda: torch.device("cuda:0")
TOL = 2e-6
N = 30


def graph(E, in_dim, seed):
    row = (synth.uniform01(seed, E, stream=1) * N).astype(np.int64)
    col = (row + 1 + (synth.uniform01(seed, E, stream=2) * (N - 1)).astype(np.int64)) % N      # no self loops
    return np.stack([row, col]), synth.normal(seed, (E, in_dim), stream=3), synth.normal(seed, (N, 64), stream=4)


def rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(1.0, float(np.abs(ref).max()))) if ref.size else 0.0


@pytest.mark.parametrize("in_dim,h1,h2,out", [(6, 40, 24, 20), (6, 96, 96, 64), (6, 4, 4, 4), (16, 72, 36, 32), (1, 36, 36, 32)])
def test_padded_edge_encoder_matches_float64(in_dim, h1, h2, out):
    params = synth.model_params(32, 1, node_in_dim=64, edge_in_dim=in_dim)
    params["encoder_feats_dict"].update(edge_dims=[h1, h2], edge_out_dim=out)
    params["edge_model_feats_dict"]["dims"] = [80, out]
    params["classifier_feats_dict"]["edge_in_dim"] = out
    W = synth.make_weights(params, seed=9)
    model = MOTMPNet(params)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    model = model.to(dev()).train()
    model.gemm_precision = "fp32"
    W64 = O.to_tensors(W, torch.float64)
    enc = {k: v for k, v in W64.items() if k.startswith("encoder.edge_model")}
    for E in (1, 127, 128, 129, 300):
        ei, ea, x = graph(E, in_dim, seed=E)
        # the reference: the oracle's MLP truncated after layer 0, after layer 1, whole
        ref = [O.mlp(torch.from_numpy(ea).double(), {k: v for k, v in enc.items() if int(k.split(".")[3]) <= 2 * i}, "encoder.edge_model").numpy()
               for i in range(3)]
        assert [r.shape[1] for r in ref] == [h1, h2, out]
        xd, eid, ead = torch.from_numpy(x).to(dev()), torch.from_numpy(ei).to(dev()), torch.from_numpy(ea).to(dev())
        pg = capi.PreparedGraph(eid, N, validate=True)
        logits = torch.full((1, E), float("nan"), dtype=torch.float32, device=dev())
        capi.path_counters(reset=True)
        ws = native_forward_saved(model, pg, xd, ead, logits)
        torch.cuda.synchronize()
        counts = capi.path_counters(reset=True)
        assert counts["edge_encoder"] == 1, counts
        got = [capi.saved_activation(model, pg, ws, "enc_edge", 0, 0), capi.saved_activation(model, pg, ws, "enc_edge", 0, 1),
               capi.saved_activation(model, pg, ws, "e", 0)]
        for i, (g, r) in enumerate(zip(got, ref)):
            g = g.cpu().numpy()
            assert g.shape == r.shape, (E, i, g.shape, r.shape)
            e = rel(g, r)
            print("EDGE_ENC_ERR %d->%d->%d->%d E=%d layer %d: %.2e" % (in_dim, h1, h2, out, E, i, e))
            assert np.isfinite(g).all() and e <= TOL, (E, i, e)
        # the whole forward against the oracle, and again without saving (the encoder's hidden outputs are null)
        with torch.no_grad():
            want = torch.stack([l.view(-1) for l in O.forward(params, W64, torch.from_numpy(x).double(), torch.from_numpy(ei),
                                                              torch.from_numpy(ea).double(), return_state=True)[1]]).numpy()
            capi.path_counters(reset=True)
            plain = model.eval().hot_path(xd, eid, ead, return_state=True)[0]
            torch.cuda.synchronize()
            counts = capi.path_counters(reset=True)
            model.train()
        assert counts["edge_encoder"] == 1, counts
        plain = plain.reshape(want.shape).cpu().numpy()
        assert rel(logits.cpu().numpy(), want) < 1e-4 and rel(plain, want) < 1e-4, (E, rel(logits.cpu().numpy(), want), rel(plain, want))
        assert rel(plain, logits.cpu().numpy().astype(np.float64)) < 1e-5, E
