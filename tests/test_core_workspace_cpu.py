"""The refusal path of the core operators, without a device: ``mpnhip_forward``, ``mpnhip_backward``, ``mpnhip_meta_layer_forward``
and ``mpnhip_mlp_forward`` plan their workspace and refuse a null or short one with MPNHIP_ERR_WORKSPACE and the two numbers in
``mpnhip_last_error()`` before any HIP call -- every pointer below is the address 256, which nothing may follow.  The sizes are
asked from the library, never pinned: tools/diag/workspace_sizes.py is how two builds' layouts are compared."""
import ctypes as C

import pytest

from mpntrackseg_amd import capi, synth

ERR_WORKSPACE = -3   # include/mpnhip.h
ONE = C.c_void_p(256)
N, E = 65, 301


def models():
    for d, L, agg, prec, deep in [(32, 3, "max", "fp32", False), (64, 4, "mean", "fp32_split", False), (64, 4, "sum", "bf16", False),
                                  (32, 0, "sum", "fp32", False), (32, 2, "mean", "fp32", True)]:
        p = synth.model_params(d, L, agg, node_in_dim=48)
        yield "d%d L%d %s %s%s" % (d, L, agg, prec, " deeper" if deep else ""), capi.dims_model(synth.deeper_params(p) if deep else p, prec, pointer=256)


def refused(status, message):
    assert status == ERR_WORKSPACE, (status, capi.load().mpnhip_last_error())
    assert capi.load().mpnhip_last_error() == message.encode()


@pytest.mark.parametrize("label,m", list(models()), ids=[k for k, _ in models()])
def test_forward_and_backward_refuse_a_short_workspace(label, m):
    lib = capi.load()
    for save in (0, 1):
        need = lib.mpnhip_forward_workspace_bytes(m, N, E, save)
        assert need > 0 and need % 256 == 0
        for ws, given in ((ONE, need - 1), (ONE, 0), (None, need)):
            refused(lib.mpnhip_forward(m, ONE, N, E, ONE, ONE, ONE, None, None, ws, given, save, None), "forward: workspace %d < %d" % (given, need))
    fneed, need = lib.mpnhip_forward_workspace_bytes(m, N, E, 1), lib.mpnhip_backward_workspace_bytes(m, N, E)
    assert need > 0 and need % 256 == 0
    for fn, flags in ((lib.mpnhip_backward, ()), (lib.mpnhip_backward_flags, (0,))):
        def backward(fws, fbytes, bws, bbytes):
            return fn(m, ONE, N, E, ONE, ONE, ONE, None, None, ONE, ONE, fws, fbytes, bws, bbytes, *flags, None)
        for fws, given in ((ONE, fneed - 1), (None, fneed)):   # (the forward workspace is looked at first)
            refused(backward(fws, given, None, 0), "backward: forward workspace %d < %d (must be the save_for_backward buffer)" % (given, fneed))
        for bws, given in ((ONE, need - 1), (ONE, 0), (None, need)):
            refused(backward(ONE, fneed, bws, given), "backward: workspace %d < %d" % (given, need))


@pytest.mark.parametrize("label,m", list(models()), ids=[k for k, _ in models()])
def test_meta_layer_refuses_a_short_workspace(label, m):
    lib = capi.load()
    need = lib.mpnhip_meta_layer_workspace_bytes(m, N, E)
    assert need > 0 and need % 256 == 0
    for ws, given in ((ONE, need - 1), (ONE, 0), (None, need)):
        refused(lib.mpnhip_meta_layer_forward(m, ONE, N, E, ONE, ONE, ONE, ONE, ws, given, None), "meta_layer: workspace %d < %d" % (given, need))


def test_mlp_forward_refuses_a_short_workspace():
    lib = capi.load()
    mlp = capi.fill_mlp_dims(capi.Mlp(), 6, [18, 18, 16], pointer=256)
    need = lib.mpnhip_mlp_workspace_bytes(mlp, N)
    assert need > 0 and need % 256 == 0
    for ws, given in ((ONE, need - 1), (ONE, 0), (None, need)):
        refused(lib.mpnhip_mlp_forward(mlp, ONE, ONE, N, ws, given, None), "mlp_forward: workspace %d < %d" % (given, need))
    assert lib.mpnhip_mlp_forward(mlp, None, None, 0, None, 0, None) == 0   # no rows: nothing to do, no workspace asked for


def test_size_queries_of_bad_models_are_zero():
    lib = capi.load()
    p = synth.model_params(32, 3, "sum", node_in_dim=48)
    bad = capi.dims_model(p)
    bad.classifier.in_dim += 1
    assert lib.mpnhip_forward_workspace_bytes(bad, N, E, 1) == 0 and lib.mpnhip_backward_workspace_bytes(bad, N, E) == 0
    assert lib.mpnhip_forward_workspace_bytes(None, N, E, 1) == 0 and lib.mpnhip_meta_layer_workspace_bytes(None, N, E) == 0
    assert lib.mpnhip_mlp_workspace_bytes(None, N) == 0
