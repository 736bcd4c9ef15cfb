"""The C-ABI library loads without a GPU and exports every function include/mpnhip.h declares;
the ctypes table in mpntrackseg_amd/capi.py covers the same set.  No compute calls here."""
import ctypes
import os
import re
import subprocess

import pytest

from mpntrackseg_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(REPO, "include", "mpnhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mpnhip_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.lib_path()):
        subprocess.check_call(["make", "-C", REPO, "-j4"], stdout=subprocess.DEVNULL)
    return ctypes.CDLL(capi.lib_path())


def test_header_functions_are_exported(lib):
    names = declared_functions()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mpnhip.h but not exported"


def test_ctypes_table_matches_header():
    assert sorted(capi.SIGNATURES) == declared_functions()


def test_version_and_sizes_without_gpu(lib):
    l = capi.load()
    assert l.mpnhip_version().decode().startswith("mpnhip")
    # pure host arithmetic: buffer sizes grow with the graph
    a, b = l.mpnhip_graph_bytes(10, 100), l.mpnhip_graph_bytes(1000, 100000)
    assert 0 < a < b


def test_struct_layout_matches_c():
    # sizeof(mpnhip_mlp) = 2 ints + 8 ints + 4 * 8 pointers, padded to 8
    assert ctypes.sizeof(capi.Mlp) == 8 + 32 + 4 * 8 * 8
    # 6 ints, 7 MLPs, then precision and weights_prepacked (two ints)
    assert ctypes.sizeof(capi.Model) == 24 + 7 * ctypes.sizeof(capi.Mlp) + 8
    assert capi.Model.precision.offset == 24 + 7 * ctypes.sizeof(capi.Mlp)
    assert capi.Model.weights_prepacked.offset == capi.Model.precision.offset + 4


def test_linear_bf16_args_layout_matches_c():
    # 15 pointers / int64 fields, int64 m, 7 ints, padded to 8
    assert ctypes.sizeof(capi.LinearBf16Args) == 15 * 8 + 8 + 7 * 4 + 4
    assert capi.LinearBf16Args.m.offset == 120 and capi.LinearBf16Args.n.offset == 128 and capi.LinearBf16Args.accumulate.offset == 152


def test_seg_job_layout_matches_c():
    # mpnhip_seg_job: 4 pointers / int64, 2 ints, pointer, int64, 5 ints (+ 4 bytes of padding), pointer, int64
    J = capi.SegJob
    assert ctypes.sizeof(J) == 4 * 8 + 2 * 4 + 2 * 8 + 5 * 4 + 4 + 2 * 8 == 96
    offsets = dict(src=0, lds=8, list=16, ptr=24, nseg=32, dim=36, out=40, ldo=48, nmod=56, off0=60, off1=64, runs=68,
                   run_stride=72, out16=80, ldo16=88)
    assert [f[0] for f in J._fields_] == list(offsets)
    for name, off in offsets.items():
        assert getattr(J, name).offset == off, name
    # the header declares the fields in the same order
    src = open(os.path.join(REPO, "include", "mpnhip.h")).read()
    body = re.search(r"typedef struct mpnhip_seg_job \{(.*?)\} mpnhip_seg_job;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == list(offsets)


def test_precision_codes_match_header():
    src = open(os.path.join(REPO, "include", "mpnhip.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define MPNHIP_PREC_([A-Z0-9_]+) (\d+)", src)}
    assert codes == capi.PRECISIONS


def test_new_entry_points_argument_checks_without_gpu():
    """Size queries and the argument checks of the f-3 / f-4 / optimizer entry points run on the host: no device work is
    reached for empty inputs, null pointers or undersized workspaces (error codes as include/mpnhip.h states)."""
    l = capi.load()
    assert l.mpnhip_knn_mask_workspace_bytes(1000, 0) > l.mpnhip_knn_mask_workspace_bytes(1000, 1) > 0
    assert l.mpnhip_time_valid_conn_workspace_bytes(500) >= 501 * 8
    assert l.mpnhip_compact_workspace_bytes(1000) > 0
    # empty inputs are successful no-ops
    assert l.mpnhip_knn_mask(None, None, 0, 0, 5, 1, 1, None, None, 0, None) == 0
    assert l.mpnhip_edge_features(None, 0, 0, None, ctypes.c_float(25.0), None, None, None, None, None, None) == 0
    assert l.mpnhip_pairwise_distance(None, 0, 0, None, 0, ctypes.c_float(1e-6), None, None) == 0
    assert l.mpnhip_gather_rows(None, 4, None, 0, 4, None, None) == 0
    assert l.mpnhip_average_preds(None, None, 0, None, None) == 0
    assert l.mpnhip_adam_step(None, None, None, None, 0, ctypes.c_float(1e-3), ctypes.c_float(0.9), ctypes.c_float(0.999),
                              ctypes.c_float(1e-8), ctypes.c_float(0.0), 1, None) == 0
    # null pointers / bad sizes are refused before anything is launched
    assert l.mpnhip_knn_mask(None, None, 10, 5, 5, 1, 1, None, None, 0, None) != 0
    assert b"knn_mask" in l.mpnhip_last_error()
    assert l.mpnhip_edge_features(None, 3, 2, None, ctypes.c_float(25.0), None, None, None, None, None, None) != 0
    assert l.mpnhip_adam_step(None, None, None, None, 5, ctypes.c_float(1e-3), ctypes.c_float(0.9), ctypes.c_float(0.999),
                              ctypes.c_float(1e-8), ctypes.c_float(0.0), 0, None) != 0
    assert l.mpnhip_window_accumulate(None, None, 3, None, 2, 0, None, None, None) != 0   # more kept than window edges
    # embedding-file selection (f-4): empty inputs succeed, null pointers are refused
    assert l.mpnhip_embedding_keep(None, 17, 0, None, 0, None, None) == 0
    assert l.mpnhip_embedding_keep(None, 17, 5, None, 0, None, None) != 0
    assert b"embedding_keep" in l.mpnhip_last_error()
    assert l.mpnhip_embedding_check(None, 17, None, 0, None, None, None) != 0   # the mismatch counter is always required


def test_attention_and_avgpool_argument_checks_without_gpu():
    """The host-side checks of the mask branch's entry points: everything below returns before a kernel is launched (the
    non-null pointers are host dummies that are never dereferenced)."""
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    # forward: feature size not a multiple of 4, null graph
    assert l.mpnhip_attention_aggregate(p, 3, 5, p, 6, p, p, p, p, None) != 0
    assert b"attention" in l.mpnhip_last_error()
    assert l.mpnhip_attention_aggregate(p, 3, 5, p, 0, p, p, p, p, None) != 0
    assert l.mpnhip_attention_aggregate(None, 3, 5, p, 8, p, p, p, p, None) != 0
    assert b"attention" in l.mpnhip_last_error()
    assert l.mpnhip_attention_aggregate(p, 3, 5, None, 8, p, p, p, p, None) != 0      # null x with nodes
    assert l.mpnhip_attention_aggregate(p, 3, 5, p, 8, None, p, p, p, None) != 0      # null logits with edges
    # no nodes: a successful no-op with a non-null graph buffer, whatever else is null
    assert l.mpnhip_attention_aggregate(p, 0, 0, None, 8, None, None, None, None, None) == 0
    assert l.mpnhip_attention_aggregate_backward(p, 0, 0, None, 8, None, None, None, None, 0, None, None, None) == 0
    # backward: the same two refusals ...
    assert l.mpnhip_attention_aggregate_backward(p, 3, 5, p, 6, p, p, p, p, 0, p, p, None) != 0
    assert b"attention" in l.mpnhip_last_error()
    assert l.mpnhip_attention_aggregate_backward(None, 3, 5, p, 8, p, p, p, p, 0, p, p, None) != 0
    # ... and null weights with edges are refused whichever gradient is requested (k_attention_dx reads them as well)
    for gx, gl in ((p, None), (None, p), (p, p)):
        assert l.mpnhip_attention_aggregate_backward(p, 3, 5, p, 8, None, p, p, gx, 0, gl, p, None) != 0
        assert b"null weights" in l.mpnhip_last_error()
    assert l.mpnhip_attention_aggregate_backward(p, 3, 5, p, 8, p, p, p, None, 0, p, None, None) != 0   # grad_logits without workspace
    assert b"null workspace" in l.mpnhip_last_error()
    # avgpool: hw = 0 and negative rows are refused, rows = 0 is a no-op, null pointers with rows are refused
    assert l.mpnhip_avgpool(p, 4, 0, p, None) != 0
    assert b"avgpool" in l.mpnhip_last_error()
    assert l.mpnhip_avgpool(p, -1, 4, p, None) != 0
    assert l.mpnhip_avgpool(None, 0, 4, None, None) == 0
    assert l.mpnhip_avgpool(None, 4, 4, p, None) != 0


def test_segment_debug_entries_argument_checks_without_gpu():
    """mpnhip_debug_aggregate and mpnhip_debug_segment_reduce3 check their arguments on the host: everything below returns
    before a kernel is launched (the non-null pointers are host dummies that are never dereferenced)."""
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    # aggregate: null graph, bad sizes, unknown aggregation, null pointers with nodes; no nodes is a no-op
    assert l.mpnhip_debug_aggregate(None, 3, 5, p, 8, 0, p, None, None) != 0
    assert b"debug_aggregate" in l.mpnhip_last_error()
    assert l.mpnhip_debug_aggregate(p, -1, 5, p, 8, 0, p, None, None) != 0
    assert l.mpnhip_debug_aggregate(p, 3, 5, p, 0, 0, p, None, None) != 0
    assert l.mpnhip_debug_aggregate(p, 3, 5, p, 8, 3, p, None, None) != 0
    assert l.mpnhip_debug_aggregate(p, 3, 5, None, 8, 0, p, None, None) != 0
    assert l.mpnhip_debug_aggregate(p, 3, 5, p, 8, 0, None, None, None) != 0
    assert l.mpnhip_debug_aggregate(p, 0, 0, None, 8, 0, None, None, None) == 0

    def jobs(**kw):
        arr = (capi.SegJob * 3)()
        for j in arr:
            j.src, j.ptr, j.out, j.lds, j.ldo, j.nseg, j.dim, j.nmod = p.value, p.value, p.value, 8, 8, 4, 8, 4
        for k, v in kw.items():
            setattr(arr[1], k, v)
        return arr
    for fp16 in (0, 1):
        assert l.mpnhip_debug_segment_reduce3(None, 10, fp16, None) != 0
        assert b"null jobs" in l.mpnhip_last_error()
        for bad in (dict(nseg=-1), dict(dim=-4), dict(src=None), dict(ptr=None), dict(out=None), dict(runs=3, list=p.value),
                    dict(nmod=0), dict(nmod=-2)):
            assert l.mpnhip_debug_segment_reduce3(jobs(**bad), 10, fp16, None) == -1, bad
            assert b"debug_segment_reduce3: job 1" in l.mpnhip_last_error(), bad
    assert l.mpnhip_debug_segment_reduce3(jobs(), -1, 0, None) == -1
    # nothing to do: three empty jobs, null pointers allowed
    empty = jobs()
    for j in empty:
        j.src, j.ptr, j.out, j.nseg, j.nmod = None, None, None, 0, 0
    assert l.mpnhip_debug_segment_reduce3(empty, 0, 0, None) == 0
    assert l.mpnhip_debug_segment_reduce3(empty, 0, 1, None) == 0
    # bf16 rows: a width that is no multiple of 4 is refused by the alignment check, before any launch
    assert l.mpnhip_debug_segment_reduce3(jobs(dim=82), 10, 1, None) == -1
    assert b"alignment" in l.mpnhip_last_error()
