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


def test_debug_gemm_layout_matches_c():
    # mpnhip_debug_gemm_group: 14 pointers, 8 int64; mpnhip_debug_gemm_args: two groups, 6 ints, int64, 3 ints (+ 4 bytes of padding)
    G, A = capi.DebugGemmGroup, capi.DebugGemmArgs
    g_fields = ["A", "A2", "a_idx", "B", "bias", "G1", "g1_idx", "G2", "g2_idx", "mask", "C", "c_idx", "row_begin", "row_end",
                "lda", "lda2", "ldb", "ldg1", "ldg2", "ldmask", "ldc", "m_static"]
    assert ctypes.sizeof(G) == 22 * 8 == 176
    assert [f[0] for f in G._fields_] == g_fields
    for i, name in enumerate(g_fields):
        assert getattr(G, name).offset == 8 * i, name
    offsets = dict(g=0, ngroups=352, N=356, K=360, ksplit=364, relu=368, accumulate=372, m_upper=376, small_tiles=384, b_layout=388,
                   precision=392)
    assert ctypes.sizeof(A) == 2 * 176 + 6 * 4 + 8 + 3 * 4 + 4 == 400
    assert [f[0] for f in A._fields_] == list(offsets)
    for name, off in offsets.items():
        assert getattr(A, name).offset == off, name
    # the header declares the fields in the same order
    src = open(os.path.join(REPO, "include", "mpnhip.h")).read()
    body = re.search(r"typedef struct mpnhip_debug_gemm_group \{(.*?)\} mpnhip_debug_gemm_group;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == g_fields
    body = re.search(r"typedef struct mpnhip_debug_gemm_args \{(.*?)\} mpnhip_debug_gemm_args;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[2\])?;", body) == list(offsets)
    layouts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define MPNHIP_GEMM_B_([A-Z]+) (\d+)", src)}
    assert layouts == {"KCONTIG": 0, "NCONTIG": 1}


def test_gemm_debug_entries_argument_checks_without_gpu():
    """mpnhip_debug_gemm and mpnhip_debug_linear_splitk check their arguments on the host: everything below returns before a kernel
    is launched (the non-null pointers are host dummies that are never dereferenced)."""
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p).value

    def args(**kw):
        a = capi.DebugGemmArgs()
        a.ngroups, a.N, a.K, a.ksplit, a.m_upper = 1, 8, 8, 8, 16
        for g in a.g:
            g.A, g.B, g.C, g.lda, g.ldb, g.ldc, g.m_static = p, p, p, 8, 8, 8, 16
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    chosen = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    assert l.mpnhip_debug_gemm(None, chosen, None) == -1
    assert b"debug_gemm: null args" in l.mpnhip_last_error()
    for bad, msg in ((dict(ngroups=0), b"ngroups"), (dict(ngroups=3), b"ngroups"), (dict(ngroups=-1), b"ngroups"),
                     (dict(b_layout=2), b"b_layout"), (dict(b_layout=-1), b"b_layout"),
                     (dict(precision=3), b"precision"), (dict(precision=-1), b"precision"),
                     (dict(b_layout=1, precision=1), b"fp32 operands only"), (dict(b_layout=1, precision=2), b"fp32 operands only")):
        assert l.mpnhip_debug_gemm(ctypes.byref(args(**bad)), chosen, None) == -1, bad
        err = l.mpnhip_last_error()
        assert b"debug_gemm" in err and msg in err, (bad, err)
    assert list(chosen) == [7, 7, 7, 7]     # a refusal of the entry itself leaves `chosen` alone
    # launch_gemm's own checks follow: ksplit beyond K, ksplit without A2, a null operand
    assert l.mpnhip_debug_gemm(ctypes.byref(args(ksplit=12)), None, None) == -1
    assert b"gemm: bad N/K/ksplit" in l.mpnhip_last_error()
    assert l.mpnhip_debug_gemm(ctypes.byref(args(ksplit=4)), None, None) == -1
    assert b"second A segment" in l.mpnhip_last_error()
    a = args()
    a.g[0].B = None
    assert l.mpnhip_debug_gemm(ctypes.byref(a), None, None) == -1
    assert b"null operand" in l.mpnhip_last_error()
    # no rows: a successful no-op in every layout / precision, nothing chosen
    for bl, prec in ((0, 0), (0, 1), (0, 2), (1, 0)):
        for ng in (1, 2):
            assert l.mpnhip_debug_gemm(ctypes.byref(args(m_upper=0, b_layout=bl, precision=prec, ngroups=ng)), chosen, None) == 0
            assert list(chosen) == [-1, 0, 0, 0]

    # split-K scratch: 0 for k < 512, more than 8192 rows, 320 or more 64 x 64 tiles; positive otherwise
    sf = l.mpnhip_debug_linear_splitk_scratch_floats
    assert sf(140, 128, 508) == 0 and sf(140, 128, 512) > 0
    assert sf(8193, 64, 2048) == 0 and sf(8192, 64, 2048) > 0
    assert sf(64 * 319, 64, 2048) == 0              # more than 8192 rows
    assert sf(64 * 20, 64 * 16, 2048) == 0          # 20 x 16 = 320 tiles
    assert sf(64 * 20 + 1, 64 * 16, 2048) == 0      # 336 tiles
    assert sf(64 * 20, 64 * 16 - 1, 2048) == 0      # still 320 tiles
    assert sf(64 * 20, 64 * 15 + 63, 2048) == 0
    assert sf(64 * 19 + 63, 64 * 16, 2048) == 0
    assert sf(64 * 29, 64 * 11, 2048) > 0           # 319 tiles
    assert sf(0, 64, 2048) == 0
    for m, n, k in ((1, 36, 512), (65, 100, 704), (140, 128, 2048), (5000, 128, 2048)):
        assert sf(m, n, k) >= 2 * m * n, (m, n, k)
    # the entry: refusals, and shapes that are not this path's return MPNHIP_OK with taken = 0 before any launch
    tf = (ctypes.c_int32 * 2)(5, 5)
    assert l.mpnhip_debug_linear_splitk(None, 512, p, None, p, 8, 4, 8, 512, 0, 0, None, None, 0, 0, None, 0, p, 1 << 20, tf, None) == -1
    assert b"debug_linear_splitk" in l.mpnhip_last_error() and list(tf) == [0, 0]
    assert l.mpnhip_debug_linear_splitk(p, 512, p, None, p, 8, 4, 8, 512, 0, 3, None, None, 0, 0, None, 0, p, 1 << 20, tf, None) == -1
    assert l.mpnhip_debug_linear_splitk(p, 512, p, None, p, 8, 4, 8, 512, 0, 0, p, None, 4, 0, None, 0, p, 1 << 20, tf, None) == -1
    for kw in (dict(k=508), dict(prec=1), dict(scratch=None), dict(floats=7), dict(m=0), dict(m=8193), dict(ldx=514), dict(k=514, ldx=516)):
        m, k, prec, floats = kw.get("m", 4), kw.get("k", 512), kw.get("prec", 0), kw.get("floats", 1 << 20)
        tf[0] = tf[1] = 5
        assert l.mpnhip_debug_linear_splitk(p, kw.get("ldx", k), p, None, p, 8, m, 8, k, 0, prec, None, None, 0, 0, None, 0,
                                            kw.get("scratch", p), floats, tf, None) == 0, kw
        assert list(tf) == [0, 0], kw


def test_wgrad_product_layout_matches_c():
    # mpnhip_wgrad_group: 4 pointers; mpnhip_wgrad_product: 13 pointers / int64, 5 ints (+ 4 bytes of padding), two groups
    G, P = capi.WgradGroup, capi.WgradProduct
    assert ctypes.sizeof(G) == 32 and [f[0] for f in G._fields_] == ["grad_w", "grad_b", "row_begin", "row_end"]
    offsets = dict(dZ=0, ldz=8, z_bstride=16, dz_idx=24, H=32, ldh=40, h_bstride=48, h_idx=56, H2=64, ldh2=72, h2_bstride=80, ldw=88,
                   rows=96, csplit=104, n_out=108, k_in=112, nbatch=116, src16=120, g=128)
    assert ctypes.sizeof(P) == 13 * 8 + 5 * 4 + 4 + 2 * 32 == 192
    assert [f[0] for f in P._fields_] == list(offsets)
    for name, off in offsets.items():
        assert getattr(P, name).offset == off, name
    src = open(os.path.join(REPO, "include", "mpnhip.h")).read()
    body = re.search(r"typedef struct mpnhip_wgrad_group \{(.*?)\} mpnhip_wgrad_group;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in G._fields_]
    body = re.search(r"typedef struct mpnhip_wgrad_product \{(.*?)\} mpnhip_wgrad_product;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[2\])?;", body) == list(offsets)
    assert len(capi.WG_CHOSEN_FIELDS) == 10 and sorted(capi.WG_PATHS) == [-1, 0, 1, 2, 3, 4, 5]


def test_weight_grad_batch_debug_entry_argument_checks_without_gpu():
    """mpnhip_debug_weight_grad_batch checks its arguments on the host: everything below returns before a kernel is launched (the
    non-null pointers are host dummies that are never dereferenced)."""
    l = capi.load()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.cast(dummy, ctypes.c_void_p).value
    big = 1 << 30        # a workspace size that is never too small (the dummy is not touched before the checks have passed)

    def prod(**kw):
        a = capi.WgradProduct()
        a.dZ, a.ldz, a.z_bstride, a.H, a.ldh, a.h_bstride = p, 8, 0, p, 8, 0
        a.ldw, a.rows, a.n_out, a.k_in, a.nbatch = 8, 100, 8, 8, 1
        a.g[0].grad_w = p
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(products, n=None, prec=2, ws=p, ws_bytes=big, chosen=None):
        arr = (capi.WgradProduct * max(len(products), 1))(*products)
        n = len(products) if n is None else n
        return l.mpnhip_debug_weight_grad_batch(arr if products else None, n, prec, 0, 1, 0, ws, ws_bytes, chosen, None)
    chosen = (ctypes.c_int32 * 20)(*([7] * 20))
    assert call([], n=1, chosen=chosen) == -1
    assert b"debug_weight_grad_batch: null products" in l.mpnhip_last_error()
    for n in (0, -1, 17):
        assert call([prod()] * 17, n=n, chosen=chosen) == -1, n
        assert b"products (1 .. 16)" in l.mpnhip_last_error()
    for prec in (-1, 3, 4):
        assert call([prod()], prec=prec, chosen=chosen) == -1, prec
        assert b"unknown precision" in l.mpnhip_last_error()
    for prec in (0, 2):
        assert call([prod(src16=1)], prec=prec, chosen=chosen) == -1, prec
        assert b"src16 needs the bf16 precision" in l.mpnhip_last_error()
    for cs in (0, 8, 9, -4):
        assert call([prod(), prod(H2=p, ldh2=8, csplit=cs)], chosen=chosen) == -1, cs
        assert b"product 1: csplit" in l.mpnhip_last_error()
    for bad in (dict(n_out=0), dict(k_in=0), dict(rows=-1), dict(nbatch=0), dict(ldw=7), dict(dZ=None), dict(H=None)):
        assert call([prod(**bad)], chosen=chosen) == -1, bad
        assert b"debug_weight_grad_batch: product 0" in l.mpnhip_last_error()
    # the workspace: null, or smaller than the size query says, through the common refusal (MPNHIP_ERR_WORKSPACE)
    for prec in (0, 1, 2):
        arr = (capi.WgradProduct * 2)(prod(), prod(rows=5000, n_out=64, k_in=64, ldz=64, ldh=64, ldw=64))
        need = l.mpnhip_debug_weight_grad_batch_workspace_bytes(arr, 2, prec, 0, 0)
        assert need > 256
        assert l.mpnhip_debug_weight_grad_batch(arr, 2, prec, 0, 1, 0, p, need - 1, chosen, None) == -3
        assert b"debug_weight_grad_batch: workspace" in l.mpnhip_last_error()
        assert l.mpnhip_debug_weight_grad_batch(arr, 2, prec, 0, 1, 0, None, need, chosen, None) == -3
        # more rows, more batches, a batched plan with fewer chunks: the size follows the chunk plans
        assert l.mpnhip_debug_weight_grad_batch_workspace_bytes(arr, 1, prec, 0, 0) < need
    assert list(chosen) == [7] * 20      # a refusal leaves `chosen` alone
    # the size query refuses the same descriptions with 0
    assert l.mpnhip_debug_weight_grad_batch_workspace_bytes(None, 1, 2, 0, 0) == 0
    assert l.mpnhip_debug_weight_grad_batch_workspace_bytes((capi.WgradProduct * 1)(prod(src16=1)), 1, 2, 0, 0) == 0
    # no rows: a successful no-op, nothing chosen
    for prec in (0, 1, 2):
        assert call([prod(rows=0)], prec=prec, chosen=chosen) == 0
        assert list(chosen)[:10] == [-1] + [0] * 9


def test_chain_debug_entries_argument_checks_without_gpu():
    """mpnhip_debug_edge_chain_forward / _backward and mpnhip_debug_node_chain / _backward check their arguments on the host:
    everything below returns before a kernel is launched (the non-null pointers are host dummies that are never dereferenced)."""
    from mpntrackseg_amd import synth
    l = capi.load()
    dummy = ctypes.create_string_buffer(512)
    addr = (ctypes.addressof(dummy) + 255) & ~255
    p = ctypes.c_void_p(addr)
    capi.path_counters(reset=True)

    def model(d=128, prec="fp32", **change):
        params = synth.model_params(d, 2)
        for k, v in change.items():
            params[k] = v
        return capi.dims_model(params, prec, addr)

    def fwd_io(**kw):
        io = capi.DebugEdgeChainFwd()
        for n in ("P", "e0", "e_prev", "e_new", "msg", "logits", "h1", "hc", "hf", "mask"):
            setattr(io, n, addr)
        for k, v in kw.items():
            setattr(io, k, v)
        return io

    def bwd_io(**kw):
        io = capi.DebugEdgeChainBwd()
        for n in ("dAGG", "ARG", "dlog", "mask", "dE_io", "dZM", "dZF", "dZc", "dZ1", "dE0", "dEprev", "dZ2"):
            setattr(io, n, addr)
        for k, v in kw.items():
            setattr(io, k, v)
        return io

    fwd = lambda m, io, n=3, e=5, ws=p, nbytes=1 << 40, graph=p: l.mpnhip_debug_edge_chain_forward(
        ctypes.byref(m) if m is not None else None, graph, n, e, ctypes.byref(io) if io is not None else None, ws, nbytes, None)
    bwd = lambda m, io, n=3, e=5, ws=p, nbytes=1 << 40, graph=p: l.mpnhip_debug_edge_chain_backward(
        ctypes.byref(m) if m is not None else None, graph, n, e, ctypes.byref(io) if io is not None else None, ws, nbytes, None)
    m = model()
    # sizes grow with the edge count; the mask buffer is the chain's own formula: ((E + 127) / 128 + 3) blocks x 4 waves x 64 lanes x 14 words
    assert l.mpnhip_debug_edge_chain_mask_ints(ctypes.byref(m), 161) == (2 + 3) * 4 * 64 * (5 + 1 + 1 + 4 + 2)
    assert 0 < l.mpnhip_debug_edge_chain_forward_workspace_bytes(ctypes.byref(m), 10) < l.mpnhip_debug_edge_chain_forward_workspace_bytes(ctypes.byref(m), 1000)
    assert l.mpnhip_debug_edge_chain_backward_workspace_bytes(ctypes.byref(m)) > 0
    for call, io in ((fwd, fwd_io()), (bwd, bwd_io())):
        assert call(None, io) == -1 and call(m, None) == -1 and call(m, io, graph=None) == -1
        assert b"debug_edge_chain" in l.mpnhip_last_error()
        assert call(m, io, n=-1) == -1 and call(m, io, e=-1) == -1
        assert call(m, io, n=0, e=5) == -1                       # edges without nodes
        assert call(m, io, e=0) == 0                             # no edges: a successful no-op
        assert call(m, io, ws=None) == -3 and call(m, io, nbytes=16) == -3
        assert call(m, io, ws=ctypes.c_void_p(addr + 4)) == -1   # misaligned workspace
        # refused widths and modes: MPNHIP_ERR_UNSUPPORTED, and the size queries say 0
        for bad in (model(96), model(256), model(128, "fp32_wgsplit")):
            assert call(bad, io) == -4
            assert l.mpnhip_debug_edge_chain_forward_workspace_bytes(ctypes.byref(bad), 10) == 0
            assert l.mpnhip_debug_edge_chain_mask_ints(ctypes.byref(bad), 10) == 0
            assert l.mpnhip_debug_edge_chain_backward_workspace_bytes(ctypes.byref(bad)) == 0
        deep = model()
        deep.classifier.n_layers, deep.classifier.out_dims[1], deep.classifier.out_dims[2] = 3, 8, 1
        deep.classifier.weight[2] = deep.classifier.bias[2] = addr
        assert call(deep, io) == -4
        wrong = model()
        wrong.flow_in.in_dim += 4
        assert call(wrong, io) == -1
    for name in ("P", "e_prev", "e0", "e_new", "msg", "logits"):
        assert fwd(m, fwd_io(**{name: None})) == -1, name
    assert fwd(m, fwd_io(save=1, mask=None)) == -1 and fwd(m, fwd_io(save=1, h1=None)) == -1
    assert fwd(m, fwd_io(P=addr + 4)) == -1
    # hoist_e0: MPNHIP_PREC_FP32 with re-attached edge features only
    assert fwd(model(128, "fp32_split"), fwd_io(hoist_e0=1)) == -1
    assert fwd(model(128, reattach_initial_edges=False), fwd_io(hoist_e0=1, e0=None)) == -1
    assert fwd(model(128, reattach_initial_edges=False), fwd_io(e0=None), e=0) == 0
    for name in ("dAGG", "dlog", "mask", "dE_io", "dZM", "dZF", "dZc", "dZ1", "dE0", "dEprev"):
        assert bwd(m, bwd_io(**{name: None})) == -1, name
    assert bwd(m, bwd_io(dEprev=None, first_step=1), e=0) == 0
    mx = model()
    mx.agg = capi.AGG_CODE["max"]
    assert bwd(mx, bwd_io(ARG=None)) == -1
    # the fp32 forward entry does not take MPNHIP_PREC_BF16 (mpnhip_debug_edge_chain_bf16_forward does); the backward entry does, at the
    # widths the bf16 backward kernel takes: multiples of 8, re-attached edge features -- with dZ2 a buffer of its own
    assert fwd(model(128, "bf16"), fwd_io()) == -4 and l.mpnhip_debug_edge_chain_mask_ints(ctypes.byref(model(128, "bf16")), 10) == 0
    mb16 = model(128, "bf16")
    assert l.mpnhip_debug_edge_chain_backward_workspace_bytes(ctypes.byref(mb16)) > 0
    assert l.mpnhip_debug_edge_chain_backward_workspace_bytes(ctypes.byref(model(256, "bf16"))) > \
        l.mpnhip_debug_edge_chain_backward_workspace_bytes(ctypes.byref(mb16))
    assert bwd(mb16, bwd_io(), e=0) == 0 and bwd(mb16, bwd_io(), ws=None) == -3 and bwd(mb16, bwd_io(skip_e0=1), ws=None) == -3
    assert bwd(mb16, bwd_io(dZ2=None)) == -1 and bwd(m, bwd_io(dZ2=None), ws=None) == -3
    assert bwd(model(128, "bf16", reattach_initial_edges=False), bwd_io()) == -4 and bwd(model(96, "bf16"), bwd_io()) == -4
    odd16 = model(128, "bf16")
    odd16.classifier.out_dims[0] = 28
    assert bwd(odd16, bwd_io()) == -4 and l.mpnhip_debug_edge_chain_backward_workspace_bytes(ctypes.byref(odd16)) == 0
    # hoist_e0 only where the forward takes that form: de >= 32
    assert fwd(model(32), fwd_io(hoist_e0=1)) == -1 and fwd(model(64), fwd_io(hoist_e0=1), ws=None) == -3
    # skip_e0: two column passes only (re-attachment, 32 < de <= 64)
    assert bwd(model(64), bwd_io(skip_e0=1)) == -1 and bwd(model(128, reattach_initial_edges=False), bwd_io(skip_e0=1)) == -1

    # the bf16-operand forward chain: its own precision, re-attached edge features, save / rows16 only at widths they take
    def bf_io(**kw):
        io = capi.DebugEdgeChainBf16Fwd()
        for n, t in io._fields_:
            if t is ctypes.c_void_p:
                setattr(io, n, addr)
        for k, v in kw.items():
            setattr(io, k, v)
        return io

    bf = lambda m, io, n=3, e=5, ws=p, nbytes=1 << 40, graph=p: l.mpnhip_debug_edge_chain_bf16_forward(
        ctypes.byref(m) if m is not None else None, graph, n, e, ctypes.byref(io) if io is not None else None, ws, nbytes, None)
    mb = model(128, "bf16")
    epb, nw = ctypes.c_int32(-1), ctypes.c_int32(-1)
    l.mpnhip_debug_edge_chain_bf16_geometry(ctypes.byref(mb), ctypes.byref(epb), ctypes.byref(nw))
    assert (epb.value, nw.value) == (256, 8)
    l.mpnhip_debug_edge_chain_bf16_geometry(ctypes.byref(model(256, "bf16")), ctypes.byref(epb), ctypes.byref(nw))
    assert (epb.value, nw.value) == (128, 4)
    l.mpnhip_debug_edge_chain_bf16_geometry(ctypes.byref(model(96, "bf16")), ctypes.byref(epb), ctypes.byref(nw))
    assert (epb.value, nw.value) == (0, 0)
    # ((E + 255) / 256 + 4) blocks x 8 waves x 64 lanes x (5 + 1 + 1 + 4 + 2) words
    assert l.mpnhip_debug_edge_chain_bf16_mask_ints(ctypes.byref(mb), 300) == (2 + 4) * 8 * 64 * 13
    assert 0 < l.mpnhip_debug_edge_chain_bf16_forward_workspace_bytes(ctypes.byref(mb), 10) < \
        l.mpnhip_debug_edge_chain_bf16_forward_workspace_bytes(ctypes.byref(mb), 5000)
    assert bf(None, bf_io()) == -1 and bf(mb, None) == -1 and bf(mb, bf_io(), graph=None) == -1 and bf(mb, bf_io(), e=-1) == -1
    assert bf(mb, bf_io(), e=0) == 0 and bf(mb, bf_io(), n=0) == -1
    for bad in (model(128, "fp32"), model(128, "fp32_split"), model(96, "bf16"), model(128, "bf16", reattach_initial_edges=False)):
        assert bf(bad, bf_io()) == -4
        assert l.mpnhip_debug_edge_chain_bf16_mask_ints(ctypes.byref(bad), 10) == 0
        assert l.mpnhip_debug_edge_chain_bf16_forward_workspace_bytes(ctypes.byref(bad), 10) == 0
    odd = model(128, "bf16")               # hc = 28: the inference variant takes it, the SAVE variant (hc % 8) does not
    odd.classifier.out_dims[0] = 28
    assert bf(odd, bf_io(save=1)) == -4 and bf(odd, bf_io(), ws=None) == -3
    d44 = model(128, "bf16")               # de = 44: two tiles like 64, but no bf16 rows of 8
    d44.de = d44.edge.out_dims[1] = d44.classifier.in_dim = 44
    d44.edge.in_dim, d44.flow_in.in_dim, d44.flow_out.in_dim = 4 * 128 + 2 * 44, 2 * 128 + 44, 2 * 128 + 44
    assert l.mpnhip_debug_edge_chain_bf16_forward_workspace_bytes(ctypes.byref(d44), 10) > 0
    assert bf(d44, bf_io(rows16=1)) == -4 and bf(d44, bf_io(save=1)) == -4 and bf(d44, bf_io(), ws=None) == -3
    for name in ("P", "e0", "e_prev", "e_new", "msg", "logits"):
        assert bf(mb, bf_io(**{name: None})) == -1, name
    assert bf(mb, bf_io(fused_agg=1, agg_out=None)) == -1 and bf(mb, bf_io(fused_agg=1, msg=None), ws=None) == -3
    assert bf(mb, bf_io(save=1, dec_m=None)) == -1 and bf(mb, bf_io(rows16=1, e16=None)) == -1
    assert bf(mb, bf_io(), ws=None) == -3 and bf(mb, bf_io(), nbytes=64) == -3 and bf(mb, bf_io(P=addr + 4)) == -1

    # node chain: widths, then pointers
    nc = lambda dn=64, pw=544, n=4, e=9, agg=0, graph=p, M=p, Wu=p, bu=p, Wn=p, P0=p, x=p, Pn=p, ao=p, ws=p, nbytes=1 << 40: \
        l.mpnhip_debug_node_chain(graph, n, e, M, dn, pw, agg, Wu, bu, Wn, P0, x, Pn, ao, ws, nbytes, None)
    ncb = lambda dn=64, pw=544, n=4, dP=p, xp=p, Wn=p, Wu=p, dZ=p, dA=p, ws=p, nbytes=1 << 40: \
        l.mpnhip_debug_node_chain_backward(n, dP, dn, pw, xp, Wn, Wu, dZ, dA, ws, nbytes, None)
    assert l.mpnhip_debug_node_chain_workspace_bytes(64, 544) > 0 and l.mpnhip_debug_node_chain_backward_workspace_bytes(128, 1088) > 0
    for dn, pw in ((32, 272), (96, 816), (64, 540), (256, 2176)):
        assert l.mpnhip_debug_node_chain_workspace_bytes(dn, pw) == 0 and l.mpnhip_debug_node_chain_backward_workspace_bytes(dn, pw) == 0
        assert nc(dn=dn, pw=pw) == -4 and ncb(dn=dn, pw=pw) == -4
        assert b"debug_node_chain" in l.mpnhip_last_error()
    assert nc(n=-1) == -1 and nc(e=-1) == -1 and nc(agg=3) == -1 and nc(graph=None) == -1 and nc(dn=0) == -1
    assert nc(n=0) == 0 and ncb(n=0) == 0
    for bad in (dict(M=None), dict(Wu=None), dict(bu=None), dict(Wn=None), dict(x=None), dict(P0=None), dict(x=ctypes.c_void_p(addr + 4))):
        assert nc(**bad) == -1, bad
    assert nc(P0=None, Pn=None, ws=None) == -3                    # (no P_next: P0 is not needed -- reaches the workspace check)
    assert nc(ws=None) == -3 and nc(nbytes=8) == -3 and ncb(ws=None) == -3 and ncb(nbytes=8) == -3
    assert ncb(n=-1) == -1
    for bad in (dict(dP=None), dict(xp=None), dict(Wn=None), dict(Wu=None), dict(dZ=None), dict(dA=None), dict(dP=ctypes.c_void_p(addr + 4))):
        assert ncb(**bad) == -1, bad
    assert not any(capi.path_counters(reset=True).values()), "an argument check let a launch through"
