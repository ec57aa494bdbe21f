"""Tensor-level wrappers over the C-ABI of libesvit_hip.so.

Each function takes/returns torch CUDA tensors, allocates outputs with torch (the library never
allocates) and enqueues on torch's current stream.  There is no CPU or eager fallback: a
non-CUDA tensor is an error.  Shapes and semantics are documented in include/esvit_hip.h.
"""
import ctypes as C
import os

import numpy as np
import torch

from ._lib import BF16, EPI_GELU, EPI_GELU_BWD, EPI_NONE, EPI_QGELU, EPI_QGELU_BWD, F32, GEMM_AUTO, GEMM_DMA8, GEMM_P8, GemmDesc, GemmTopk, GridGroup, MAX_GRID_GROUPS, PATCH_EMBED_BWD, PATCH_EMBED_FWD, PATCH_EMBED_MAX_CROPS, PATCH_EMBED_REDUCE, PatchEmbed, check, lib

_ACT_DTYPE = torch.bfloat16


def set_act_dtype(dt):
    """Storage type of activations: torch.bfloat16 (benchmark mode) or torch.float32 (exact-parity mode)."""
    global _ACT_DTYPE
    assert dt in (torch.bfloat16, torch.float32)
    _ACT_DTYPE = dt


def act_dtype():
    return _ACT_DTYPE


def _code(dt):
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float32:
        return F32
    raise TypeError("unsupported activation dtype %s" % dt)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("esvit_amd.ops: tensor is not on the GPU (no CPU fallback exists)")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


def _actc(t):
    assert t.dtype in (torch.float32, torch.bfloat16) and t.is_contiguous()
    return t


# ------------------------------------------------------------------------------------------------
# shared scratch (split-K partials, column-sum partials, LN partials); stream-ordered reuse
# ------------------------------------------------------------------------------------------------
_WS = {}


def workspace(nfloats, device, slot=0):
    # stream-ordered reuse: one scratch per (device, slot, stream) -- work enqueued on different streams never shares it
    key = (device, slot, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nfloats:
        buf = torch.empty(max(int(nfloats), 1 << 20), dtype=torch.float32, device=device)
        _WS[key] = buf
    return buf


# ------------------------------------------------------------------------------------------------
# host-side integer index maps
# ------------------------------------------------------------------------------------------------
def relative_position_index(ws):
    out = np.empty((ws * ws, ws * ws), dtype=np.int64)
    check(lib.esvit_relative_position_index(ws, out.ctypes.data_as(C.c_void_p)), "relative_position_index")
    return out


# esvit_query questions (include/esvit_hip.h)
(Q_ATTN_FRAG_ELEMS, Q_ATTN_LSE_ELEMS, Q_ATTN_BWD_PARTS, Q_ATTN_BWD_PAD_ROWS, Q_LN_BWD_BLOCKS, Q_COLSUM_BLOCKS, Q_COL_REDUCE_BLOCKS,
 Q_UPDATE_CHUNK_ELEMS, Q_MLP_FUSED, Q_AUG_MAX_BOX, Q_JPEG_WORKSPACE, Q_RESIZE_FITS, Q_CHUNK_ATTN_WS, Q_TOPK_WS, Q_PROBE_CE_REG_ROW,
 Q_GLOBAL_ATTN_WS, Q_MLP_DW_WS, Q_ATTN_BWD_FUSED_GRID, Q_PATCH_EMBED_WS, Q_DIST_STATS, Q_ATTN_TAIL_WS) = range(1, 22)
MLP_DW_PARTIAL_FLOATS = 74208  # ESVIT_MLP_DW_PARTIAL_FLOATS
ATTN_BWD_PARTIAL_FLOATS = 37440  # ESVIT_ATTN_BWD_PARTIAL_FLOATS
ATTN_TAIL_PARTIAL_FLOATS = 28128  # ESVIT_ATTN_TAIL_PARTIAL_FLOATS
LN_BWD_QKV_TAIL = -1  # ESVIT_LN_BWD_QKV_TAIL


def query(what, a=0, b=0, c=0):
    """scratch sizes / capabilities of the library (esvit_query)"""
    return int(lib.esvit_query(int(what), int(a), int(b), int(c)))


def window_maps(H, W, ws, shift):
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    win2tok = np.empty((Hp // ws) * (Wp // ws) * ws * ws, dtype=np.int32)
    tok2win = np.empty(H * W, dtype=np.int32)
    check(lib.esvit_window_maps(H, W, ws, shift, win2tok.ctypes.data_as(C.c_void_p), tok2win.ctypes.data_as(C.c_void_p), None),
          "window_maps")
    return win2tok, tok2win


def shift_mask(H, W, ws, shift):
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    nW, N = (Hp // ws) * (Wp // ws), ws * ws
    mask = np.empty((nW, N, N), dtype=np.float32)
    n = C.c_int(0)
    check(lib.esvit_shift_mask(H, W, ws, shift, mask.ctypes.data_as(C.c_void_p), C.byref(n)), "shift_mask")
    assert n.value == nW
    return mask


def shift_region_ids(H, W, ws, shift):
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    ids = np.empty((Hp // ws) * (Wp // ws) * ws * ws, dtype=np.int32)
    check(lib.esvit_window_maps(H, W, ws, shift, None, None, ids.ctypes.data_as(C.c_void_p)), "window_maps(region ids)")
    return ids


# ------------------------------------------------------------------------------------------------
# GEMM family
# ------------------------------------------------------------------------------------------------
# optional launch timing for bench.py's roofline leg: list of (flops, start_event, end_event) or None
GEMM_PROFILE = None
_EVENT_POOL = []


def _event():
    return _EVENT_POOL.pop() if _EVENT_POOL else torch.cuda.Event(enable_timing=True)


def _gemm(dt, **kw):
    if GEMM_PROFILE is not None:
        e0, e1 = _event(), _event()
        e0.record()
        _gemm_launch(dt, **kw)
        e1.record()
        GEMM_PROFILE.append((2.0 * kw["M"] * kw["N"] * kw["K"] * kw.get("batch", 1), e0, e1,
                             (kw["M"], kw["N"], kw["K"], kw.get("a_kstrided", 0), kw.get("b_kstrided", 0), kw.get("splitk", 0)),
                             gemm_algorithmic_bytes(dt, kw)))
        return
    _gemm_launch(dt, **kw)


def gemm_algorithmic_bytes(dt, kw):
    """HBM bytes one esvit_gemm call has to move when every operand is read once and every output written once:
    A + B + C (+ the GELU pre-activation / derivative side tensor, + the fp32 residual).  Split-K partials are NOT
    algorithmic (they are this implementation's overhead and show up in the PMC traffic instead)."""
    es = 2 if dt == torch.bfloat16 else 4
    M, N, K, batch = kw["M"], kw["N"], kw["K"], kw.get("batch", 1)
    b = batch * (M * K + N * K) * es + batch * M * N * (4 if kw.get("out_f32", 0) else es)
    if kw.get("aux") is not None:
        b += M * N * es
    if kw.get("residual") is not None:
        b += M * N * 4
    return float(b)


# main loop forced on every esvit_gemm call issued through this module (GEMM_AUTO = the library's own choice); the
# descriptor carries it, the library keeps no state.  Tests sweep it to run every main loop on every shape.
FORCE_GEMM_KERNEL = GEMM_AUTO


def _gemm_desc(kw):
    d = GemmDesc()
    for k in ("A", "B", "C", "bias", "residual", "rowmap", "rowscale", "aux", "partial", "colsum", "colsum_partial", "rowstat", "rowstat_center", "colstat"):
        setattr(d, k, _p(kw.get(k)))
    d.rowstat_scale = float(kw.get("rowstat_scale", 0.0))
    for k in ("M", "N", "K", "lda", "ldb", "ldc", "a_kstrided", "b_kstrided", "strideA", "strideB", "strideC", "ldr",
              "rowmap_period", "rowmap_tokens", "rows_per_sample", "ldaux", "epilogue", "out_f32", "splitk", "accumulate"):
        setattr(d, k, int(kw.get(k, 0)))
    d.batch = int(kw.get("batch", 1))
    d.alpha = float(kw.get("alpha", 1.0))
    d.kernel = int(kw.get("kernel", FORCE_GEMM_KERNEL))
    if d.kernel == GEMM_DMA8 and d.a_kstrided and "kernel" not in kw:
        d.kernel = GEMM_AUTO  # FORCE_GEMM_KERNEL is a test / bench hook: the 8-wave tile has no weight-gradient instantiation
    if d.kernel == GEMM_P8 and "kernel" not in kw:
        # (same hook) the eight-phase loops run whole 64-deep k-tiles, have no row map / statistics, and the 256 x 128 one its own list
        # of epilogue kinds: ask the library whether the forced loop takes this descriptor
        tm, tn, slots = C.c_int(0), C.c_int(0), C.c_int(0)
        if lib.esvit_gemm_select(BF16, C.byref(d), C.byref(tm), C.byref(tn), C.byref(slots)) <= 0:
            d.kernel = GEMM_AUTO
    return d


def _gemm_launch(dt, **kw):
    d = _gemm_desc(kw)
    if dt != torch.bfloat16:
        d.kernel = GEMM_AUTO  # the exact-fp32 mode has one main loop
    check(lib.esvit_gemm(_code(dt), C.byref(d), _stream()), "esvit_gemm")


def gemm_select(dt, **kw):
    """-> (kernel id, tile_m, tile_n, resident workgroup slots) the library would use for this problem (no pointers needed)"""
    d = _gemm_desc(kw)
    if dt != torch.bfloat16:
        d.kernel = GEMM_AUTO
    tm, tn, slots = C.c_int(0), C.c_int(0), C.c_int(0)
    k = lib.esvit_gemm_select(_code(dt), C.byref(d), C.byref(tm), C.byref(tn), C.byref(slots))
    if k <= 0:
        raise RuntimeError("esvit_gemm_select failed (%d): %s" % (k, lib.esvit_last_error().decode()))
    return k, tm.value, tn.value, slots.value


LOG2E = 1.4426950408889634


def row_stats_supported(dt, M, N):
    """can the GEMM that writes logits [M, N] also emit their softmax row statistics (esvit_gemm_desc::rowstat)?"""
    return dt == torch.bfloat16 and M > 0 and M % 128 == 0 and N % 128 == 0


def linear_fwd(x, w, bias=None, *, gelu=False, want_preact=False, residual=None, rowmap=None, rowmap_tokens=0,
               out_rows=None, rowscale=None, rows_per_sample=0, out_f32=False, quick=False, row_stats=None):
    """y = x @ w^T (+bias) with the fused epilogue of the GEMM kernel.  gelu: exact erf-GELU, or (quick=True) the
    QuickGELU x*sigmoid(1.702x) of the CvT feed-forward.

    x [M, K] act; w [N, K] act (cached cast of the fp32 parameter); bias fp32 [N].
    rowmap (int32 [period]) scatters window rows to token rows (out_rows rows, tokens per image =
    rowmap_tokens); residual fp32 [out_rows, N] is added at the destination row.
    row_stats = (inv_temp, center fp32 [N] or None[, want_col_sums]): also return the softmax statistics of z = (y - center) * inv_temp,
    the outputs of teacher_row_stats -> (y, row_max, row_lse); the shape must pass row_stats_supported.  With want_col_sums the batch
    sum of the stored logits per column (what the centre update reads, main_esvit.py:752-770) rides along as the attribute
    `esvit_col_sums` of row_max (fp32 [N]; absent when the main loop in use has no such epilogue)."""
    x, w = _actc(x), _actc(w)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.dtype == w.dtype
    if row_stats is not None:
        inv_temp, cen = row_stats[:2]
        want_cs = len(row_stats) > 2 and bool(row_stats[2])
        assert row_stats_supported(x.dtype, M, N) and bias is None and not gelu and residual is None and rowmap is None and not out_f32
        y = torch.empty((M, N), dtype=x.dtype, device=x.device)
        cen = None if cen is None else _f32c(cen)
        # the statistics come in blocks of 64 columns from the 128-row loop, of 32 columns from the 256 x 256 eight-phase loop
        kern = gemm_select(x.dtype, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, rowstat=y)[0]
        nb = N // (32 if kern == GEMM_P8 else 64)
        st = torch.empty((M, nb, 2), dtype=torch.float32, device=x.device)
        # column sums of the stored logits per 64-row wave tile (the statistics epilogue of the 128 x 128 tile only)
        cst = torch.empty((M // 64, N), dtype=torch.float32, device=x.device) if (want_cs and kern != GEMM_P8) else None
        _gemm(x.dtype, A=x, B=w, C=y, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, rowstat=st, rowstat_center=cen, rowstat_scale=float(inv_temp) * LOG2E,
              colstat=cst, kernel=kern)
        mx, lse = rowstat_combine(st)
        if cst is not None:
            mx.esvit_col_sums = colsum(cst)
        return y, mx, lse
    rows = M if out_rows is None else out_rows
    y = torch.empty((rows, N), dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    pre = torch.empty((M, N), dtype=x.dtype, device=x.device) if (gelu and want_preact) else None
    _gemm(x.dtype, A=x, B=w, C=y, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, residual=residual, ldr=N,
          rowmap=rowmap, rowmap_period=0 if rowmap is None else rowmap.numel(), rowmap_tokens=rowmap_tokens,
          rowscale=rowscale, rows_per_sample=rows_per_sample, aux=pre, ldaux=N,
          epilogue=(EPI_QGELU if quick else EPI_GELU) if gelu else EPI_NONE, out_f32=out_f32)
    return (y, pre) if gelu and want_preact else y


KNN_MAX_K = 256  # the largest k of esvit_gemm_desc::topk


def knn_topk_supported(test, train):
    """does the fused k-NN scan take these feature matrices (fp32 rows of a multiple of 4 features on the GPU)?"""
    return (test.is_cuda and train.is_cuda and test.dtype == torch.float32 and train.dtype == torch.float32 and test.dim() == 2 and train.dim() == 2 and
            test.shape[1] == train.shape[1] and test.shape[1] % 4 == 0 and test.shape[0] > 0 and train.shape[0] > 0)


def knn_topk(test, train, k, *, out=None, idx_base=0, return_similarity=False):
    """The k most similar train rows of every test row in one pass (esvit_gemm_desc::topk): test [Nt, C], train [Ntr, C], fp32.
    -> (vals fp32 [Nt, k], idx int32 [Nt, k]) sorted by larger similarity first, on equal similarities the smaller row number first;
    the [Nt, Ntr] similarities are never stored unless return_similarity asks for them (-> (vals, idx, similarity), tests / small sets).
    out = (vals, idx) of an earlier call: this call's rows (numbered from idx_base) are merged into those lists in place, so a train
    matrix scored piece by piece ends with the lists of the whole."""
    test, train = _f32c(test), _f32c(train)
    Nt, Cc = test.shape
    Ntr = train.shape[0]
    k = int(k)
    assert train.shape[1] == Cc
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError("knn_topk: k=%d outside 1 .. %d" % (k, KNN_MAX_K))
    if out is None and k > Ntr:
        raise ValueError("knn_topk: k=%d exceeds the %d train rows" % (k, Ntr))
    if out is None:
        vals = torch.empty((Nt, k), dtype=torch.float32, device=test.device)
        idx = torch.empty((Nt, k), dtype=torch.int32, device=test.device)
    else:
        vals, idx = out
        assert vals.shape == (Nt, k) and idx.shape == (Nt, k) and vals.dtype == torch.float32 and idx.dtype == torch.int32
        assert vals.is_contiguous() and idx.is_contiguous()
    sim = torch.empty((Nt, Ntr), dtype=torch.float32, device=test.device) if return_similarity else None
    nbytes = query(Q_TOPK_WS, Nt, Ntr, k)
    if nbytes <= 0:
        raise RuntimeError("esvit_query(Q_TOPK_WS) failed (%d): %s" % (nbytes, lib.esvit_last_error().decode()))
    ws = workspace((nbytes + 3) // 4, test.device, slot="knn_topk")
    t = GemmTopk(k=k, merge=0 if out is None else 1, vals=_p(vals), idx=_p(idx), idx_base=int(idx_base), workspace=_p(ws), workspace_bytes=ws.numel() * 4)
    d = _gemm_desc(dict(A=test, B=train, C=sim, M=Nt, N=Ntr, K=Cc, lda=Cc, ldb=Cc, ldc=Ntr, out_f32=0, kernel=GEMM_AUTO))
    d.topk = C.pointer(t)
    check(lib.esvit_gemm(F32, C.byref(d), _stream()), "esvit_gemm(topk)")
    return (vals, idx, sim) if return_similarity else (vals, idx)


def linear_dgrad(dy, w, *, gelu_preact=None, out_f32=False, quick=False):
    """dx = dy @ w  (w [Nout, Kin] act, read k-strided); optional fused GELU': dx *= gelu'(preact) (quick: QuickGELU')."""
    dy, w = _actc(dy), _actc(w)
    M, Nout = dy.shape
    Kin = w.shape[1]
    assert w.shape[0] == Nout and dy.dtype == w.dtype
    dx = torch.empty((M, Kin), dtype=torch.float32 if out_f32 else dy.dtype, device=dy.device)
    if gelu_preact is None and Nout >= 4096:
        # a very long reduction (DINOHead last layer: K = out_dim) over few output tiles: the wide-tile loop, split-K to fill the chip
        kern = FORCE_GEMM_KERNEL
        if FORCE_GEMM_KERNEL == GEMM_AUTO and dy.dtype == torch.bfloat16 and Kin >= 192:
            # (the eight-phase loop addresses its operands with 32-bit DMA offsets: d(logits) below 4 GiB)
            kern = GEMM_P8 if (Nout % 64 == 0 and Kin % 256 == 0 and dy.numel() * 2 < 0xfff00000 and not os.environ.get("ESVIT_NO_P8_ROUTING")) else GEMM_DMA8
        _, tm, tn, slots = gemm_select(dy.dtype, M=M, N=Kin, K=Nout, lda=Nout, ldb=Kin, ldc=Kin, b_kstrided=1, kernel=kern)
        tiles = (-(-M // tm)) * (-(-Kin // tn))
        if tiles <= slots // 2:
            splitk = int(min(16, max(2, slots // tiles)))
            part = workspace(splitk * M * Kin, dy.device)
            _gemm(dy.dtype, A=dy, B=w, C=dx, M=M, N=Kin, K=Nout, lda=Nout, ldb=Kin, ldc=Kin, b_kstrided=1, out_f32=out_f32,
                  splitk=splitk, partial=part, kernel=kern)
            return dx
        _gemm(dy.dtype, A=dy, B=w, C=dx, M=M, N=Kin, K=Nout, lda=Nout, ldb=Kin, ldc=Kin, b_kstrided=1, out_f32=out_f32, kernel=kern)
        return dx
    _gemm(dy.dtype, A=dy, B=w, C=dx, M=M, N=Kin, K=Nout, lda=Nout, ldb=Kin, ldc=Kin, b_kstrided=1, aux=gelu_preact,
          ldaux=Kin, epilogue=(EPI_QGELU_BWD if quick else EPI_GELU_BWD) if gelu_preact is not None else EPI_NONE, out_f32=out_f32)
    return dx


def _pick_splitk(rows, Nout, Kin, tiles, slots=512):
    """split-K factor for wgrad: as many workgroups as fit the chip AT ONCE (`slots` resident workgroups: 256 CUs x 2
    64-KiB workgroups of the 4-wave loop, x 1 of the 8-wave loop) and never one more -- every workgroup runs for the whole
    kernel, so one extra doubles its duration --, >= 512 reduction rows per split, and partial slabs (written + re-read)
    no larger than the operand traffic"""
    want = max(1, slots // max(tiles, 1))
    by_rows = max(1, rows // 512)
    by_bytes = max(1, (rows * (Nout + Kin) * 2) // (Nout * Kin * 8))
    return int(max(1, min(want, by_rows, by_bytes, 512)))


def linear_wgrad(dy, x, *, out=None, accumulate=False, want_bias=False, db_out=None):
    """dw[Nout, Kin] = dy^T @ x (fp32), both operands read k-strided, split-K over the rows.
    want_bias: also return db[Nout] = column sums of dy, fused into the same kernel (all-ones MFMA fragment); db_out: the
    fp32 [Nout] tensor to write it to (e.g. the parameter's slot of a gradient bucket)."""
    dy, x = _actc(dy), _actc(x)
    rows, Nout = dy.shape
    Kin = x.shape[1]
    assert x.shape[0] == rows and dy.dtype == x.dtype
    if out is None:
        out = torch.empty((Nout, Kin), dtype=torch.float32, device=dy.device)
        accumulate = False
    db = None
    if want_bias:
        db = db_out if db_out is not None else torch.empty((Nout,), dtype=torch.float32, device=dy.device)
        assert db.shape == (Nout,) and db.dtype == torch.float32 and db.is_contiguous()
    _, tm, tn, slots = gemm_select(dy.dtype, M=Nout, N=Kin, K=rows, lda=Nout, ldb=Kin, ldc=Kin, a_kstrided=1, b_kstrided=1, colsum=db)
    tiles = (-(-Nout // tm)) * (-(-Kin // tn))
    splitk = _pick_splitk(rows, Nout, Kin, tiles, slots)
    if splitk > 1:
        part = workspace(splitk * Nout * (Kin + 1), dy.device)
        cpart = part[splitk * Nout * Kin:] if want_bias else None
        _gemm(dy.dtype, A=dy, B=x, C=out, M=Nout, N=Kin, K=rows, lda=Nout, ldb=Kin, ldc=Kin, a_kstrided=1, b_kstrided=1,
              out_f32=1, splitk=splitk, partial=part, accumulate=int(accumulate), colsum=db, colsum_partial=cpart)
    else:
        # accumulate through the residual input (each element is read and written by the same lane)
        _gemm(dy.dtype, A=dy, B=x, C=out, M=Nout, N=Kin, K=rows, lda=Nout, ldb=Kin, ldc=Kin, a_kstrided=1, b_kstrided=1,
              out_f32=1, residual=out if accumulate else None, ldr=Kin, colsum=db)
    return (out, db) if want_bias else out


def batched_nt(a, b, out_ld):
    """out[p] = a[p] @ b[p]^T in fp32: a [P, M, K], b [P, N, K] fp32 -> out [P, M, out_ld] (cols >= N undefined)."""
    a, b = _f32c(a), _f32c(b)
    P, M, K = a.shape
    N = b.shape[1]
    out = torch.empty((P, M, out_ld), dtype=torch.float32, device=a.device)
    _gemm(torch.float32, A=a, B=b, C=out, M=M, N=N, K=K, lda=K, ldb=K, ldc=out_ld, batch=P, strideA=M * K, strideB=N * K,
          strideC=M * out_ld, out_f32=1)
    return out


def colsum(x, *, out=None, accumulate=False):
    x = _actc(x)
    rows, N = x.shape
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=x.device)
        accumulate = False
    ws = workspace(query(Q_COLSUM_BLOCKS, rows) * N, x.device, slot=1)
    check(lib.esvit_colsum(_code(x.dtype), _p(x), rows, N, N, _p(out), _p(ws), int(accumulate), _stream()), "colsum")
    return out


# ------------------------------------------------------------------------------------------------
# fused MLP forward
# ------------------------------------------------------------------------------------------------
def mlp_fused_supported(dt, Cc, backward=False):
    """the fused MLP forward exists for this width (inference passes); backward=True: the training pair exists"""
    return bool(query(Q_MLP_FUSED, _code(dt), int(Cc)) & (2 if backward else 1))


def mlp_fused_fwd(x, gamma, beta, eps, W1, b1, W2, b2, *, rowscale=None, next_norm=None):
    """x fp32 [M, C] -> y fp32 [M, C] = x + rowscale * (GELU(LN(x) W1^T + b1) W2^T + b2); nothing hidden-sized is written.
    next_norm = (gamma_next, beta_next): also return (xw_next act [M, C], mean_next, rstd_next) = LayerNorm(y) with the next
    block's norm1 parameters -> (y, (xw, mean, rstd))"""
    x, W1, W2 = _f32c(x), _actc(W1), _actc(W2)
    M, Cc = x.shape
    assert W1.shape == (4 * Cc, Cc) and W2.shape == (Cc, 4 * Cc) and W1.dtype == W2.dtype
    y = torch.empty_like(x)
    gn = bn = xw = mn = rn = None
    if next_norm is not None:
        gn, bn = _f32c(next_norm[0]), _f32c(next_norm[1])
        xw = torch.empty((M, Cc), dtype=W1.dtype, device=x.device)
        mn = torch.empty((M,), dtype=torch.float32, device=x.device)
        rn = torch.empty_like(mn)
    check(lib.esvit_mlp_fused_fwd(_code(W1.dtype), _p(x), _p(_f32c(gamma)), _p(_f32c(beta)), eps, _p(W1), _p(_f32c(b1)), _p(W2), _p(_f32c(b2)),
                                  _p(rowscale), M, Cc, _p(y), _p(gn), _p(bn), _p(xw), _p(mn), _p(rn), _stream()), "mlp_fused_fwd")
    return y if next_norm is None else (y, (xw, mn, rn))


def mlp_fused_fwd_train(x, gamma, beta, eps, W1, b1, W2, b2, *, rowscale=None):
    """the wide-stage (C = 384) training pass: y as mlp_fused_fwd plus what the UNFUSED backward reads, written by the same kernel:
    -> (y fp32 [M, C], a1 act [M, 4C] pre-activation, a1g act [M, 4C] GELU(a1), h act [M, C] LayerNorm(x), mean fp32 [M], rstd fp32 [M])"""
    x, W1, W2 = _f32c(x), _actc(W1), _actc(W2)
    M, Cc = x.shape
    assert W1.shape == (4 * Cc, Cc) and W2.shape == (Cc, 4 * Cc) and W1.dtype == W2.dtype
    y = torch.empty_like(x)
    a1 = torch.empty((M, 4 * Cc), dtype=W1.dtype, device=x.device)
    a1g = torch.empty_like(a1)
    h = torch.empty((M, Cc), dtype=W1.dtype, device=x.device)
    mean = torch.empty((M,), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    check(lib.esvit_mlp_fused_fwd_train(_code(W1.dtype), _p(x), _p(_f32c(gamma)), _p(_f32c(beta)), eps, _p(W1), _p(_f32c(b1)), _p(W2), _p(_f32c(b2)),
                                        _p(rowscale), M, Cc, _p(y), _p(a1), _p(a1g), _p(h), _p(mean), _p(rstd), _stream()), "mlp_fused_fwd_train")
    return y, a1, a1g, h, mean, rstd


def mlp_fused_train_supported(dt, Cc, rows=0):
    """esvit_mlp_fused_fwd_train exists for this width (bf16, C = 384: forward fused, backward through the GEMMs) and row count (its side outputs
    are addressed through 32-bit offsets: [rows, 4C] bf16 below 2 GiB)"""
    return dt == torch.bfloat16 and int(Cc) == 384 and mlp_fused_supported(dt, Cc) and rows * 4 * Cc * 2 < 0x7ff00000


def cast_weight(w, transpose=False, perm32=False):
    """fp32 [R, S] -> bf16 ([S, R] if transpose), rows optionally in the 32-block channel order of the 16-token kernels"""
    w = _f32c(w)
    R, S = w.shape
    out = torch.empty((S, R) if transpose else (R, S), dtype=torch.bfloat16, device=w.device)
    check(lib.esvit_cast_weight(_p(w), _p(out), R, S, int(transpose), int(perm32), _stream()), "cast_weight")
    return out


MLP_W1_FWD, MLP_W1_BWD, MLP_W1T_BWD, MLP_W2T_BWD = range(4)  # ESVIT_MLP_* of include/esvit_hip.h


def mlp_fused_weight(kind, w):
    """the weight copy the fused MLP kernels stream, from the fp32 master: kind MLP_W1_FWD / MLP_W1_BWD (fc1.weight [4C, C] for
    esvit_mlp_fused_fwd / _bwd), MLP_W1T_BWD (its transpose), MLP_W2T_BWD (the transpose of fc2.weight [C, 4C]).  fc2.weight itself
    is used as the plain activation-dtype cast.  The channel order of a copy is private to the library."""
    w = _f32c(w)
    Cc = min(w.shape)
    out = torch.empty((w.shape[1], w.shape[0]) if kind in (MLP_W1T_BWD, MLP_W2T_BWD) else tuple(w.shape), dtype=torch.bfloat16, device=w.device)
    check(lib.esvit_mlp_fused_weight(int(kind), _p(w), _p(out), Cc, _stream()), "mlp_fused_weight")
    return out


def mlp_fused_bwd(x, gy, gamma, beta, eps, W1, W2T, W1T, b1, *, rowscale_mlp=None, rowscale_out=None):
    """data-gradient path of the fused MLP branch: x (branch input) fp32 [M, C], gy = dL/dy fp32 [M, C] ->
    (gx fp32 [M, C], gx_act act [M, C] = cast(rowscale_out * gx), xhat act [M, C], a1g act [M, 4C], da1 act [M, 4C])"""
    x, gy, W1, W2T, W1T = _f32c(x), _f32c(gy), _actc(W1), _actc(W2T), _actc(W1T)
    M, Cc = x.shape
    assert gy.shape == x.shape and W1.shape == (4 * Cc, Cc) and W2T.shape == (4 * Cc, Cc) and W1T.shape == (Cc, 4 * Cc)
    dt = W1.dtype
    gx = torch.empty_like(x)
    gxa = torch.empty((M, Cc), dtype=dt, device=x.device)
    xhat = torch.empty((M, Cc), dtype=dt, device=x.device)
    a1g = torch.empty((M, 4 * Cc), dtype=dt, device=x.device)
    da1 = torch.empty((M, 4 * Cc), dtype=dt, device=x.device)
    check(lib.esvit_mlp_fused_bwd(_code(dt), _p(x), _p(gy), _p(rowscale_mlp), _p(rowscale_out), _p(_f32c(gamma)), _p(_f32c(beta)), eps, _p(W1),
                                  _p(W2T), _p(W1T), _p(_f32c(b1)), M, Cc, _p(gx), _p(gxa), _p(xhat), _p(a1g), _p(da1), _stream(),
                                  None, None, None, None, None), "mlp_fused_bwd")
    return gx, gxa, xhat, a1g, da1


def mlp_fused_dw_supported(dt, Cc):
    """esvit_mlp_fused_bwd can accumulate the branch's weight gradients on the chip at this dtype and width (bf16, C = 96)"""
    return query(Q_MLP_DW_WS, _code(dt), int(Cc), 1) > 0


def mlp_fused_dw_grid(dt, Cc, M):
    """workgroups (= partials, = the summation order) of the on-chip weight-gradient mode for M rows on the current device"""
    return query(Q_MLP_DW_WS, _code(dt), int(Cc), int(M)) // (4 * MLP_DW_PARTIAL_FLOATS)


def mlp_fused_bwd_dw(x, gy, gamma, beta, eps, W1, W2T, W1T, b1, *, rowscale_mlp=None, rowscale_out=None, out=None, db_out=None):
    """mlp_fused_bwd with the weight gradients accumulated on the chip: nothing hidden-sized is written ->
    (gx fp32 [M, C], gx_act act [M, C], dW2 fp32 [C, 4C], db2 fp32 [C], G fp32 [4C, C] = dA^T xhat, db1 fp32 [4C]); G and db1 go on to
    ln_fold_finish.  out = (dW2, G), db_out = (db2, db1): the fp32 tensors to write them to (gradient-bucket slots), each or any None"""
    x, gy, W1, W2T, W1T = _f32c(x), _f32c(gy), _actc(W1), _actc(W2T), _actc(W1T)
    M, Cc = x.shape
    assert gy.shape == x.shape and W1.shape == (4 * Cc, Cc) and W2T.shape == (4 * Cc, Cc) and W1T.shape == (Cc, 4 * Cc)
    dt = W1.dtype
    dev = x.device
    dW2, G = out if out is not None else (None, None)
    db2, db1 = db_out if db_out is not None else (None, None)
    dW2 = dW2 if dW2 is not None else torch.empty((Cc, 4 * Cc), dtype=torch.float32, device=dev)
    G = G if G is not None else torch.empty((4 * Cc, Cc), dtype=torch.float32, device=dev)
    db2 = db2 if db2 is not None else torch.empty((Cc,), dtype=torch.float32, device=dev)
    db1 = db1 if db1 is not None else torch.empty((4 * Cc,), dtype=torch.float32, device=dev)
    assert dW2.shape == (Cc, 4 * Cc) and G.shape == (4 * Cc, Cc) and db2.shape == (Cc,) and db1.shape == (4 * Cc,)
    for t in (dW2, G, db2, db1):
        _f32c(t)
    nbytes = query(Q_MLP_DW_WS, _code(dt), Cc, M)
    if nbytes <= 0:
        raise RuntimeError("mlp_fused_bwd_dw: no on-chip weight-gradient mode at dtype %s, C = %d" % (dt, Cc))
    ws = workspace(nbytes // 4, dev)
    gx = torch.empty_like(x)
    gxa = torch.empty((M, Cc), dtype=dt, device=dev)
    check(lib.esvit_mlp_fused_bwd(_code(dt), _p(x), _p(gy), _p(rowscale_mlp), _p(rowscale_out), _p(_f32c(gamma)), _p(_f32c(beta)), eps, _p(W1),
                                  _p(W2T), _p(W1T), _p(_f32c(b1)), M, Cc, _p(gx), _p(gxa), None, None, None, _stream(),
                                  _p(dW2), _p(G), _p(db1), _p(db2), _p(ws)), "mlp_fused_bwd(dw)")
    return gx, gxa, dW2, db2, G, db1


def ln_fold_finish(G, db, W, gamma, beta, *, gb_out=None):
    """LayerNorm folded out of a weight gradient: G = dY^T xhat [J, C] (overwritten by dW = G o gamma + db (x) beta), db = colsum(dY),
    W the fp32 master -> (dW, dgamma, dbeta)"""
    G, db, W = _f32c(G), _f32c(db), _f32c(W)
    J, Cc = G.shape
    assert W.shape == (J, Cc) and db.shape == (J,)
    dgamma, dbeta = _ln_grad_outs(Cc, G.device, gb_out)
    check(lib.esvit_ln_fold_finish(_p(G), _p(db), _p(W), _p(_f32c(gamma)), _p(_f32c(beta)), J, Cc, _p(dgamma), _p(dbeta), 0, _stream()), "ln_fold_finish")
    return G, dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# normalisation
# ------------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, *, rowmap=None, period_out=0, out_rows=None, want_f32=False, dtype=None):
    """x fp32 [nB, T, C] or [rows, C] -> (y act, y_f32 or None, mean, rstd).  With rowmap (int32 [T], token ->
    window slot) y has out_rows rows, zero at the pad slots."""
    x = _f32c(x)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    dt = dtype or _ACT_DTYPE
    tokens = 0
    if rowmap is not None:
        tokens = rowmap.numel()
        y = torch.zeros((out_rows, Cc), dtype=dt, device=x.device)
    else:
        y = torch.empty((rows, Cc), dtype=dt, device=x.device)
    yf = torch.empty((rows, Cc), dtype=torch.float32, device=x.device) if want_f32 else None
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    check(lib.esvit_layernorm_fwd(_code(dt), _p(x), _p(gamma), _p(beta), eps, rows, Cc, _p(y), _p(yf), _p(mean), _p(rstd),
                                  _p(rowmap), tokens, period_out, _stream()), "layernorm_fwd")
    return y, yf, mean, rstd


def _ln_grad_outs(Cc, device, gb_out):
    """(dgamma, dbeta) destinations: the caller's pair of fp32 [C] tensors (gradient-bucket slots) or a fresh [2, C]"""
    if gb_out is not None and gb_out[0] is not None and gb_out[1] is not None:
        for t in gb_out:
            assert t.numel() == Cc and t.dtype == torch.float32 and t.is_contiguous()
        return gb_out[0].view(Cc), gb_out[1].view(Cc)
    gb = torch.empty((2, Cc), dtype=torch.float32, device=device)
    return gb[0], gb[1]


def layernorm_bwd(dy, x, mean, rstd, gamma, *, g_in=None, rowmap=None, period_in=0, gb_out=None):
    """-> (dx fp32 like x, dgamma, dbeta).  dy act, read through rowmap (token -> window slot) if given."""
    x, dy = _f32c(x), _actc(dy)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    dx = torch.empty_like(x)
    dgamma, dbeta = _ln_grad_outs(Cc, x.device, gb_out)
    ws = workspace(query(Q_LN_BWD_BLOCKS, rows, Cc) * 2 * Cc, x.device, slot=1)
    check(lib.esvit_layernorm_bwd(_code(dy.dtype), _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(g_in), rows, Cc, _p(dx),
                                  _p(dgamma), _p(dbeta), _p(ws), _p(rowmap), 0 if rowmap is None else rowmap.numel(),
                                  period_in, None, 0, None, 0, _stream()), "layernorm_bwd")
    return dx, dgamma, dbeta


def layernorm_bwd_cast(dy, x, mean, rstd, gamma, *, g_in=None, rowscale=None, rows_per_sample=0, gb_out=None):
    """-> (dx fp32, dx_act = cast(rowscale * dx) in dy's dtype, dgamma, dbeta): layernorm_bwd + gather_cast in one pass"""
    x, dy = _f32c(x), _actc(dy)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    dx = torch.empty_like(x)
    dxa = torch.empty((rows, Cc), dtype=dy.dtype, device=x.device)
    dgamma, dbeta = _ln_grad_outs(Cc, x.device, gb_out)
    ws = workspace(query(Q_LN_BWD_BLOCKS, rows, Cc) * 2 * Cc, x.device, slot=1)
    check(lib.esvit_layernorm_bwd(_code(dy.dtype), _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(g_in), rows, Cc, _p(dx), _p(dgamma),
                                  _p(dbeta), _p(ws), None, 0, 0, _p(dxa), _code(dxa.dtype), _p(rowscale), rows_per_sample, _stream()), "layernorm_bwd(cast)")
    return dx, dxa, dgamma, dbeta


def layernorm_bwd_to_act(dy, x, mean, rstd, gamma, *, gb_out=None):
    """-> (cast(dx) in the activation dtype, dgamma, dbeta) from an fp32 upstream gradient `dy`, read as it is: the LayerNorm of the patch
    embedding, whose dL/dy is the fp32 residual-stream gradient and whose dL/dx is only ever read as the operand of the projection's
    weight gradient -- no fp32 dx is written and no cast pass follows"""
    x, dy = _f32c(x), _f32c(dy)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    dxa = torch.empty((rows, Cc), dtype=_ACT_DTYPE, device=x.device)
    dgamma, dbeta = _ln_grad_outs(Cc, x.device, gb_out)
    ws = workspace(query(Q_LN_BWD_BLOCKS, rows, Cc) * 2 * Cc, x.device, slot=1)
    check(lib.esvit_layernorm_bwd(_code(dy.dtype), _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), None, rows, Cc, None, _p(dgamma),
                                  _p(dbeta), _p(ws), None, 0, 0, _p(dxa), _code(dxa.dtype), None, 0, _stream()), "layernorm_bwd(to act)")
    return dxa, dgamma, dbeta


class LnQkvTail(C.Structure):
    """esvit_ln_qkv_tail (include/esvit_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("Wqkv", "beta", "dWqkv", "dbqkv")]


def attn_tail_bwd_supported(dt, Cc):
    """the qkv-tail mode of esvit_layernorm_bwd exists at this dtype and width (bf16, C = 96)"""
    return dt in (torch.float32, torch.bfloat16) and query(Q_ATTN_TAIL_WS, _code(dt), int(Cc), 1) > 0


def attn_tail_bwd_grid(dt, Cc, M):
    """workgroups (= partials, = the summation order) of attn_tail_bwd for M rows on the current device"""
    return query(Q_ATTN_TAIL_WS, _code(dt), int(Cc), int(M)) // (4 * ATTN_TAIL_PARTIAL_FLOATS)


def attn_tail_bwd(dqkv, x, mean, rstd, gamma, beta, Wqkv, g_in, *, rowscale=None, rows_per_sample=0, want_act=False, out=None, db_out=None,
                  gb_out=None):
    """the tail of a Swin block's attention-branch backward in one pass over the rows: qkv data gradient, qkv weight and bias gradient and
    norm1's backward.  dqkv act [M, 3C], x fp32 [M, C] (the block input), mean / rstd of norm1, Wqkv act [3C, C] (the plain cast),
    g_in fp32 [M, C] = dL/dx1 -> (gx fp32 [M, C], gx_act = cast(rowscale * gx) or None, dWqkv fp32 [3C, C], dbqkv fp32 [3C], dgamma,
    dbeta).  out / db_out / gb_out: the fp32 tensors to write dWqkv / dbqkv / (dgamma, dbeta) to (gradient-bucket slots)"""
    dqkv, x, g_in, Wqkv = _actc(dqkv), _f32c(x), _f32c(g_in), _actc(Wqkv)
    M, Cc = x.shape
    dt, dev = dqkv.dtype, x.device
    assert dqkv.shape == (M, 3 * Cc) and Wqkv.shape == (3 * Cc, Cc) and Wqkv.dtype == dt and g_in.shape == x.shape
    assert mean.shape == (M,) and rstd.shape == (M,)
    nbytes = query(Q_ATTN_TAIL_WS, _code(dt), Cc, M)
    if nbytes <= 0:
        raise RuntimeError("attn_tail_bwd: no qkv-tail mode at dtype %s, C = %d" % (dt, Cc))
    dW = out if out is not None else torch.empty((3 * Cc, Cc), dtype=torch.float32, device=dev)
    db = db_out if db_out is not None else torch.empty((3 * Cc,), dtype=torch.float32, device=dev)
    assert dW.shape == (3 * Cc, Cc) and db.shape == (3 * Cc,)
    dgamma, dbeta = _ln_grad_outs(Cc, dev, gb_out)
    gx = torch.empty_like(x)
    gxa = torch.empty((M, Cc), dtype=dt, device=dev) if want_act else None
    assert rowscale is None or want_act
    # (a tensor of its own, not the shared scratch: the partials are larger than the scratch's floor, and growing that for good would
    # change what every later caller of the slot finds)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
    rec = LnQkvTail(_p(Wqkv).value, _p(_f32c(beta)).value, _p(_f32c(dW)).value, _p(_f32c(db)).value)
    check(lib.esvit_layernorm_bwd(_code(dt), _p(dqkv), _p(x), _p(_f32c(mean)), _p(_f32c(rstd)), _p(_f32c(gamma)), _p(g_in), M, Cc, _p(gx), _p(dgamma),
                                  _p(dbeta), _p(ws), C.cast(C.pointer(rec), C.c_void_p), 0, LN_BWD_QKV_TAIL, _p(gxa), _code(dt) if want_act else 0,
                                  _p(rowscale), rows_per_sample, _stream()), "layernorm_bwd(qkv tail)")
    return gx, gxa, dW, db, dgamma, dbeta


MERGE_LN_PAD = True  # merge_ln_fwd / merge_ln_bwd take pad=True: odd grids padded inside the kernel (ESVIT_MERGE_PAD, include/esvit_hip.h)
MERGE_PAD_FLAG = 0x40000000  # ESVIT_MERGE_PAD: OR'd into H, selects the pad mode of esvit_merge_ln_fwd / _bwd


def _merge_grid(H, W, pad):
    """-> (the H argument of the library call, merged rows per sample)"""
    if pad:
        return min(max(H, 0), 0xffff) | MERGE_PAD_FLAG, ((H + 1) // 2) * ((W + 1) // 2)  # (a side the low 16 bits cannot hold: one the library refuses)
    return H, (H // 2) * (W // 2)


def merge_ln_fwd(x, gamma, beta, eps, H, W, dtype=None, out=None, pad=False):
    """x fp32 [nB, H*W, C] -> (y act [nB*H/2*W/2, 4C], mean, rstd).  out: optional preallocated (y, mean, rstd) -- e.g.
    row slices of buffers shared by several resolution groups.  pad: H x W of any parity, the missing bottom row / right column
    read as zeros inside the kernel -> ceil(H/2)*ceil(W/2) rows per sample (F.pad + merge, swin_transformer.py:406-414)."""
    x = _f32c(x)
    nB, L, Cc = x.shape
    assert L == H * W
    Harg, rps = _merge_grid(H, W, pad)
    rows = nB * rps
    dt = dtype or _ACT_DTYPE
    if out is not None:
        y, mean, rstd = out
        assert y.shape == (rows, 4 * Cc) and y.dtype == dt and y.is_contiguous() and mean.is_contiguous() and rstd.is_contiguous()
    else:
        y = torch.empty((rows, 4 * Cc), dtype=dt, device=x.device)
        mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
    check(lib.esvit_merge_ln_fwd(_code(dt), _p(x), _p(gamma), _p(beta), eps, nB, Harg, W, Cc, _p(y), _p(mean), _p(rstd), _stream()),
          "merge_ln_fwd")
    return y, mean, rstd


def merge_ln_bwd(dy, x, mean, rstd, gamma, H, W, dx_out=None, gb_out=None, accumulate=False, act_out=None, rowscale=None, pad=False):
    """pad: as in merge_ln_fwd; dx / act_out keep the true [nB, H*W, C] grid, pad positions receive nothing.  gb_out: optional fp32 [2, 4C] receiving (dgamma | dbeta); accumulate: add to it instead of overwriting (further
    resolution groups sharing the parameters).  act_out: optional activation-dtype [nB*H*W, C] receiving cast(rowscale * dx)
    (rowscale: per token row, or None) -- the MLP-branch operand of the block whose dL/dy this dx is (SwinBlockMultiFn's shadow)"""
    x, dy = _f32c(x), _actc(dy)
    nB, L, Cc = x.shape
    if dx_out is not None:
        assert dx_out.numel() == x.numel() and dx_out.dtype == torch.float32 and dx_out.is_contiguous()
        dx = dx_out
    else:
        dx = torch.empty_like(x)
    if act_out is not None:
        assert act_out.numel() == x.numel() and act_out.dtype == dy.dtype and act_out.is_contiguous()
        assert rowscale is None or (rowscale.numel() == nB * L and rowscale.dtype == torch.float32 and rowscale.is_contiguous())
    else:
        assert rowscale is None
    acc = bool(accumulate) and gb_out is not None
    gb = gb_out if gb_out is not None else torch.empty((2, 4 * Cc), dtype=torch.float32, device=x.device)
    assert gb.shape == (2, 4 * Cc) and gb.is_contiguous()
    dgamma, dbeta = gb[0], gb[1]
    Harg, rps = _merge_grid(H, W, pad)
    rows = nB * rps
    assert not pad or (L == H * W and dy.numel() == rows * 4 * Cc and mean.numel() == rows and rstd.numel() == rows)
    ws = workspace(query(Q_LN_BWD_BLOCKS, rows, 4 * Cc) * 8 * Cc, x.device, slot=1)
    check(lib.esvit_merge_ln_bwd(_code(dy.dtype), _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), nB, Harg, W, Cc, _p(dx), _p(dgamma),
                                 _p(dbeta), _p(ws), _p(act_out), _p(rowscale), 1, int(acc), _stream()), "merge_ln_bwd")
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# data movement
# ------------------------------------------------------------------------------------------------
def gather_cast(src, rows, *, rowmap=None, tokens=0, rowscale=None, rows_per_sample=0, dtype=None):
    """dst[r] = cast(scale * src[map(r)]); src fp32 [*, C] -> dst act [rows, C]."""
    src = _f32c(src)
    Cc = src.shape[-1]
    dt = dtype or _ACT_DTYPE
    dst = torch.empty((rows, Cc), dtype=dt, device=src.device)
    check(lib.esvit_gather_cast(_code(dt), _p(src), _p(dst), rows, Cc, _p(rowmap), 0 if rowmap is None else rowmap.numel(),
                                tokens, _p(rowscale), rows_per_sample, _stream()), "gather_cast")
    return dst


def cast_to_act(x, dtype=None, out=None):
    x = _f32c(x)
    dt = dtype or _ACT_DTYPE
    if out is None:
        out = torch.empty(x.shape, dtype=dt, device=x.device)
    assert out.dtype == dt and out.numel() == x.numel() and out.is_contiguous()
    check(lib.esvit_cast_f32_to(_code(dt), _p(x), _p(out), x.numel(), _stream()), "cast_f32_to")
    return out






PATCH_IM2COL_RECT = True  # patch_im2col takes [nB, 3, H, W] with H != W (esvit_patch_im2col's packed form of S)


def patch_im2col(img, P, Kpad, dtype=None, out=None):
    """img fp32 [nB, 3, H, W] -> cols [nB * (H/P) * (W/P), Kpad], column order (c, ph, pw).  A square image goes in the library's plain
    form (S = the side), a rectangle as S = H | W << 16 (include/esvit_hip.h)."""
    img = _f32c(img)
    nB, ch, H, W = img.shape
    assert ch == 3 and 0 < H < 65536 and 0 < W < 32768, tuple(img.shape)
    dt = dtype or _ACT_DTYPE
    rows = nB * (H // P) * (W // P)
    if out is not None:
        assert out.shape == (rows, Kpad) and out.dtype == dt and out.is_contiguous()
        cols = out
    else:
        cols = torch.empty((rows, Kpad), dtype=dt, device=img.device)
    check(lib.esvit_patch_im2col(_code(dt), _p(img), _p(cols), nB, H if H == W else (H | (W << 16)), P, Kpad, _stream()), "patch_im2col")
    return cols


# ---- fused patch embedding (the fused mode of esvit_patch_im2col): image -> LayerNorm(conv 4x4/4) tokens in one kernel each way
PATCH_EMBED_FWD_TILE, PATCH_EMBED_BWD_TILE = 64, 128  # token rows per workgroup tile of the two kernels
PATCH_EMBED_K = 48


def patch_embed_supported(dt, E, patch=4, in_ch=3):
    """the fused patch embedding exists at this activation dtype and geometry (bf16, 4 x 4 patches of 3 channels, E in {96, 128, 192})"""
    return patch == 4 and in_ch == 3 and dt in (torch.bfloat16, torch.float32) and query(Q_PATCH_EMBED_WS, _code(dt), int(E), 1) > 0


def patch_embed_rows(imgs):
    return [im.shape[0] * (im.shape[2] // 4) * (im.shape[3] // 4) for im in imgs]


def _patch_embed_call(d, ncrops, what):
    check(lib.esvit_patch_im2col(BF16, C.cast(C.pointer(d), C.c_void_p), None, -ncrops, 0, 4, PATCH_EMBED_K, _stream()), what)


def _patch_embed_chunks(imgs, row0=0):
    """(first crop, crops, first row, rows) of every launch: at most PATCH_EMBED_MAX_CROPS crop tensors each"""
    rows = patch_embed_rows(imgs)
    out, r = [], row0
    for i in range(0, len(imgs), PATCH_EMBED_MAX_CROPS):
        n = sum(rows[i:i + PATCH_EMBED_MAX_CROPS])
        out.append((i, imgs[i:i + PATCH_EMBED_MAX_CROPS], r, n))
        r += n
    return out


def _patch_embed_desc(mode, W, bias, gamma, crops, row0):
    d = PatchEmbed()
    d.mode, d.E = mode, W.shape[0]
    d.W, d.bias, d.gamma = _p(_actc(W)), _p(_f32c(bias)), _p(_f32c(gamma))
    r = row0
    for i, im in enumerate(crops):
        im = _f32c(im)
        if im.dim() != 4 or im.shape[1] != 3:
            raise ValueError("patch embedding: images are [nB, 3, H, W], not %s" % (tuple(im.shape),))
        cr = d.crops[i]
        cr.img, cr.nB, cr.H, cr.W, cr.row0 = _p(im), im.shape[0], im.shape[2], im.shape[3], r
        r += im.shape[0] * (im.shape[2] // 4) * (im.shape[3] // 4)
    return d


def patch_embed_fwd(imgs, W, bias, gamma, beta, eps, *, stats=True, out=None):
    """imgs: fp32 [nB_i, 3, H_i, W_i] (sides multiples of 4), W act [E, 48] -> (x fp32 [sum rows, E], mean, rstd fp32 [rows] or None, None
    without stats): LayerNorm(patch projection), crops in order, rows (image, patch row, patch column).  out: preallocated (x, mean, rstd)"""
    E = W.shape[0]
    assert W.shape == (E, PATCH_EMBED_K) and len(imgs) > 0
    M = sum(patch_embed_rows(imgs))
    dev = imgs[0].device
    if out is not None:
        x, mean, rstd = out
        assert x.shape == (M, E) and (mean is None) == (rstd is None) and (mean is None or (mean.shape == (M,) and rstd.shape == (M,)))
    else:
        x = torch.empty((M, E), dtype=torch.float32, device=dev)
        mean = torch.empty((M,), dtype=torch.float32, device=dev) if stats else None
        rstd = torch.empty((M,), dtype=torch.float32, device=dev) if stats else None
    for _, crops, r0, _ in _patch_embed_chunks(imgs):
        d = _patch_embed_desc(PATCH_EMBED_FWD, W, bias, gamma, crops, r0)
        d.beta, d.eps = _p(_f32c(beta)), eps
        d.x, d.mean, d.rstd = _p(_f32c(x)), _p(None if mean is None else _f32c(mean)), _p(None if rstd is None else _f32c(rstd))
        _patch_embed_call(d, len(crops), "patch_embed_fwd")
    return x, mean, rstd


def patch_embed_parts(E, imgs):
    """partial records the backward over these crop tensors writes (one launch per PATCH_EMBED_MAX_CROPS of them) on the current device"""
    return sum(query(Q_PATCH_EMBED_WS, BF16, E, n) // (4 * E * (PATCH_EMBED_K + 3)) for _, _, _, n in _patch_embed_chunks(imgs))


def patch_embed_bwd(imgs, W, bias, gamma, gx, mean, rstd, *, partials=None):
    """the backward of patch_embed_fwd up to its partial sums: gx fp32 [rows, E] -> (partials fp32 [records, 51 E], records); every record is
    [dW E x 48 | dbias | dgamma | dbeta] of one workgroup.  patch_embed_reduce finishes.  partials: a preallocated buffer"""
    E = W.shape[0]
    gx, mean, rstd = _f32c(gx), _f32c(mean), _f32c(rstd)
    M = sum(patch_embed_rows(imgs))
    assert gx.shape == (M, E) and mean.shape == (M,) and rstd.shape == (M,)
    nparts = patch_embed_parts(E, imgs)
    if nparts <= 0:
        raise RuntimeError("patch_embed_bwd: no fused patch embedding at E = %d" % E)
    rec = E * (PATCH_EMBED_K + 3)
    if partials is None:
        partials = torch.empty((nparts, rec), dtype=torch.float32, device=gx.device)
    assert partials.numel() >= nparts * rec and partials.dtype == torch.float32 and partials.is_contiguous()
    first = 0
    for _, crops, r0, n in _patch_embed_chunks(imgs):
        d = _patch_embed_desc(PATCH_EMBED_BWD, W, bias, gamma, crops, r0)
        d.gx, d.mean, d.rstd, d.partials, d.first_partial = _p(gx), _p(mean), _p(rstd), _p(partials), first
        _patch_embed_call(d, len(crops), "patch_embed_bwd")
        first += query(Q_PATCH_EMBED_WS, BF16, E, n) // (4 * rec)
    return partials, nparts


def patch_embed_reduce(partials, nparts, E, *, out=None):
    """-> (dW fp32 [E, 48], dbias, dgamma, dbeta fp32 [E]) = the first nparts records of `partials` summed in a fixed order.
    out: the four fp32 tensors to write (gradient-bucket slots), each or any None"""
    dev = partials.device
    outs = list(out) if out is not None else [None] * 4
    shapes = [(E, PATCH_EMBED_K), (E,), (E,), (E,)]
    for i, shp in enumerate(shapes):
        if outs[i] is None:
            outs[i] = torch.empty(shp, dtype=torch.float32, device=dev)
        assert outs[i].numel() == E * (PATCH_EMBED_K if i == 0 else 1)
        _f32c(outs[i])
    d = PatchEmbed()
    d.mode, d.E, d.first_partial, d.partials = PATCH_EMBED_REDUCE, E, int(nparts), _p(_f32c(partials))
    d.dW, d.dbp, d.dgamma, d.dbeta = [_p(t) for t in outs]
    _patch_embed_call(d, 1, "patch_embed_reduce")
    return tuple(outs)


def token_mean_fwd(x, dtype=None):
    """x fp32 [nB, T, C] -> (mean fp32 [nB, C], mean act [nB, C])."""
    x = _f32c(x)
    nB, T, Cc = x.shape
    dt = dtype or _ACT_DTYPE
    out = torch.empty((nB, Cc), dtype=torch.float32, device=x.device)
    out_act = torch.empty((nB, Cc), dtype=dt, device=x.device)
    check(lib.esvit_token_mean_fwd(_code(dt), _p(x), nB, T, Cc, _p(out), _p(out_act), _stream()), "token_mean_fwd")
    return out, out_act


def token_mean_bwd(g_mean, g_tok, T):
    g_mean = _f32c(g_mean)
    nB, Cc = g_mean.shape
    dx = torch.empty((nB, T, Cc), dtype=torch.float32, device=g_mean.device)
    check(lib.esvit_token_mean_bwd(_p(g_mean), _p(g_tok), nB, T, Cc, _p(dx), _stream()), "token_mean_bwd")
    return dx


# ------------------------------------------------------------------------------------------------
# window attention
# ------------------------------------------------------------------------------------------------
def attn_frag_elems(N):
    n = query(Q_ATTN_FRAG_ELEMS, N)
    if n < 0:
        raise RuntimeError("window size with %d tokens is not supported by the HIP attention kernel yet" % N)
    return n






def new_bias_frag(nH, N, device):
    """scratch for the fragment-order relative-position bias of one block (filled by the first attention call that gets it
    together with the table; later calls of the step -- the other resolution group, the backward -- pass it with table None)"""
    return torch.empty(2 * nH * attn_frag_elems(N), dtype=torch.float32, device=device)


def window_attn_fwd(qkv, qkv_bias, win2tok, L, rel_table, ws, region_ids, nW, N, nH, scale, want_attn=False, out=None, bias_frag=None):
    """token-ordered qkv [nB*L, 3C] -> (out [nB*L, C], lse or None[, attn]); win2tok int32 [nW*N] slot -> token (-1 = zero-pad slot).
    lse (per-query log-sum-exp) is produced for 14x14 windows, whose blocked backward needs it."""
    qkv = _actc(qkv)
    rows, C3 = qkv.shape
    Cc = C3 // 3
    nB = rows // L
    if out is None:
        out = torch.empty((rows, Cc), dtype=qkv.dtype, device=qkv.device)
    assert out.shape == (rows, Cc) and out.dtype == qkv.dtype and out.is_contiguous()  # may be a row slice of a larger matrix
    attn = torch.empty((nB * nW, nH, N, N), dtype=torch.float32, device=qkv.device) if want_attn else None
    nl = query(Q_ATTN_LSE_ELEMS, N)
    lse = torch.empty((nB * nW * nH, nl), dtype=torch.float32, device=qkv.device) if nl else None
    # frag-layout relative-position bias of every head: the caller's per-block buffer, or shared scratch refilled by this call
    bias_ws = bias_frag if bias_frag is not None else workspace(2 * nH * attn_frag_elems(N), qkv.device, slot=2)
    assert rel_table is not None or bias_frag is not None
    check(lib.esvit_window_attn_fwd(_code(qkv.dtype), _p(qkv), _p(_f32c(qkv_bias)), _p(win2tok), L, _p(None if rel_table is None else _f32c(rel_table)), ws, _p(bias_ws),
                                    _p(region_ids), nW, nB, N, nH, Cc // nH, scale, _p(out), _p(lse), _p(attn), _stream()),
          "window_attn_fwd")
    return (out, lse, attn) if want_attn else (out, lse)


# ---- statistics of the window softmax (csrc/window_attn.hip, window_attn_big.hip): entropy of every row and a few rows of P, without P --
ATTN_WINDOW_STATS = 0x04000000  # ESVIT_ATTN_WINDOW_STATS: OR'd into a real window side, selects the statistics mode of esvit_window_attn_fwd


def window_attn_stats_supported(dtype, N, hd):
    """the statistics kernels exist for this shape: every instance the probability variant of window_attn_fwd has"""
    if dtype not in (torch.bfloat16, torch.float32) or hd not in (32, 64) or not 0 < N <= 224:
        return False
    return N <= 64 or hd == 32 or dtype == torch.bfloat16


def _stats_slots(slots, nslots, device):
    """a list / range / int tensor of window slots w * N + i -> int32 device tensor, every index checked against [0, nW * N) here: the
    library cannot read the array"""
    if torch.is_tensor(slots):
        s = slots.reshape(-1)
        assert not s.dtype.is_floating_point and s.dtype != torch.bool, "slots: integer slot indices"
        if s.numel():
            lo, hi = int(s.min()), int(s.max())
            if lo < 0 or hi >= nslots:
                raise ValueError("window_attn_stats: slot indices must lie in [0, %d), got %d .. %d" % (nslots, lo, hi))
        return s.to(device=device, dtype=torch.int32).contiguous()
    idx = [int(i) for i in slots]
    bad = [i for i in idx if not 0 <= i < nslots]
    if bad:
        raise ValueError("window_attn_stats: slot indices must lie in [0, %d), got %r" % (nslots, bad[:8]))
    return torch.tensor(idx, dtype=torch.int32, device=device)


def window_attn_stats(qkv, qkv_bias, win2tok, L, rel_table, ws, region_ids, nW, N, nH, scale, slots=None, bias_frag=None, ent_out=None,
                      rows_out=None):
    """what an attention analysis reads of the softmax window_attn_fwd computes, without the maps: token-ordered qkv [nB*L, 3C] ->
    (entropy fp32 [nB*nW, nH, N] in nats, window-slot order, pad query slots included; rows fp32 [nB, nH, nq, N] or None: the
    probability row, over the N slots of its own window, of every listed slot w * N + i in [0, nW * N) -- the same list for every image
    and head, duplicates allowed).  ent_out / rows_out: optional contiguous fp32 destinations of those shapes."""
    qkv = _actc(qkv)
    rows_, C3 = qkv.shape
    Cc = C3 // 3
    nB = rows_ // L
    sidx = None if slots is None else _stats_slots(slots, nW * N, qkv.device)
    nq = 0 if sidx is None else sidx.numel()
    if nq >= 1 << 15:
        raise ValueError("window_attn_stats: at most %d listed slots, got %d" % ((1 << 15) - 1, nq))
    ent = torch.empty((nB * nW, nH, N), dtype=torch.float32, device=qkv.device) if ent_out is None else ent_out
    rows = None
    if slots is not None:
        rows = torch.empty((nB, nH, nq, N), dtype=torch.float32, device=qkv.device) if rows_out is None else rows_out
    for t, shape in ((ent, (nB * nW, nH, N)), (rows, (nB, nH, nq, N))):
        assert t is None or (t.shape == shape and t.dtype == torch.float32 and t.is_contiguous()), (shape, t.shape)
    bias_ws = bias_frag if bias_frag is not None else workspace(2 * nH * attn_frag_elems(N), qkv.device, slot=2)
    assert rel_table is not None or bias_frag is not None
    check(lib.esvit_window_attn_fwd(_code(qkv.dtype), _p(qkv), _p(_f32c(qkv_bias)), _p(win2tok), L, _p(None if rel_table is None else _f32c(rel_table)),
                                    ws | ATTN_WINDOW_STATS, _p(bias_ws), _p(region_ids), nW, nB, N | (nq << 16), nH, Cc // nH, scale,
                                    _p(sidx) if nq else None, _p(rows) if nq else None, _p(ent), _stream()), "window_attn_fwd(window stats)")
    return ent, rows


def attn_branch_supported(dt, Cc, nH, N, rows=0, windows=0):
    """the fused attention branch (esvit_attn_branch_fwd) exists for this shape: bf16, head_dim 32, C in {96, 192}, <= 64-token windows,
    and -- when given -- a call of `rows` token rows / `windows` windows stays inside the kernel's 2 GiB buffer ranges and 2^22-window
    limit (esvit_hip.h), so that an oversized per-GPU batch takes the four-kernel sequence instead of raising"""
    return (dt == torch.bfloat16 and Cc in (96, 192) and Cc == 32 * nH and N <= 64
            and rows * 3 * Cc * 2 < 0x7fff0000 and rows * Cc * 4 < 0x7fff0000 and windows < (1 << 22))


def attn_branch_fwd(x, gamma, beta, eps, Wqkv_p, bqkv, Wproj_p, bproj, win2tok, L, rel_table, ws, region_ids, nW, N, nH, scale, *,
                    rowscale=None, out=None, bias_frag=None, save=False):
    """x fp32 [nB*L, C] token rows of one resolution group -> y fp32 = x + rowscale * (proj(window_attention(qkv(LayerNorm(x)))) + b_proj)
    in one kernel.  Wqkv_p / Wproj_p: cast_weight(W, perm32=True) of qkv.weight / proj.weight.  save=True also returns what the
    unfused backward reads: (y, (xw, mean, rstd, qkv, ao)); save=(xw, mean, rstd, qkv, ao) writes them into the given tensors (row
    slices of a stage's matrices).  bias_frag / rel_table as for window_attn_fwd."""
    x = _f32c(x)
    rows, Cc = x.shape
    nB = rows // L
    assert rows == nB * L and Wqkv_p.shape == (3 * Cc, Cc) and Wproj_p.shape == (Cc, Cc) and Wqkv_p.dtype == torch.bfloat16
    y = torch.empty_like(x) if out is None else out
    assert y.shape == x.shape and y.dtype == torch.float32 and y.is_contiguous()
    xw = qkv = ao = mean = rstd = None
    if save is True:
        xw = torch.empty((rows, Cc), dtype=torch.bfloat16, device=x.device)
        qkv = torch.empty((rows, 3 * Cc), dtype=torch.bfloat16, device=x.device)
        ao = torch.empty((rows, Cc), dtype=torch.bfloat16, device=x.device)
        mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
    elif save:
        xw, mean, rstd, qkv, ao = save
        assert xw.shape == (rows, Cc) and qkv.shape == (rows, 3 * Cc) and ao.shape == (rows, Cc) and mean.shape == (rows,) and rstd.shape == (rows,)
        assert all(t.is_contiguous() for t in save) and xw.dtype == qkv.dtype == ao.dtype == torch.bfloat16 and mean.dtype == rstd.dtype == torch.float32
    if rowscale is not None:
        assert rowscale.shape == (rows,) and rowscale.dtype == torch.float32 and rowscale.is_contiguous()
    bias_ws = bias_frag if bias_frag is not None else workspace(2 * nH * attn_frag_elems(N), x.device, slot=2)
    assert rel_table is not None or bias_frag is not None
    check(lib.esvit_attn_branch_fwd(BF16, _p(x), _p(_f32c(gamma)), _p(_f32c(beta)), eps, _p(Wqkv_p), _p(_f32c(bqkv)), _p(Wproj_p), _p(_f32c(bproj)),
                                    _p(win2tok), L, _p(None if rel_table is None else _f32c(rel_table)), ws, _p(bias_ws), _p(region_ids), nW, nB, N, nH,
                                    scale, _p(rowscale), _p(y), _p(xw), _p(qkv), _p(ao), _p(mean), _p(rstd), _stream(), None), "attn_branch_fwd")
    return (y, (xw, mean, rstd, qkv, ao)) if save else y


class AttnBwdDesc(C.Structure):
    """esvit_attn_bwd_desc (include/esvit_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("gin", "rowscale_out", "gx", "gx_act", "WqkvT", "dWqkv", "dbqkv", "dWproj", "dbproj", "dgamma", "dbeta",
                                         "dbias_ws", "partials_ws")] + [("first_partial", C.c_int32), ("finish", C.c_int32), ("index", C.c_void_p),
                                                                        ("dtable", C.c_void_p), ("table_rows", C.c_int32)]


def attn_branch_bwd_grid(dt, Cc, windows):
    """workgroups (= partials, = bias-gradient slabs, = the summation order) of one attn_branch_bwd call over `windows` windows on the
    current device; 0 where the mode does not exist"""
    return query(Q_ATTN_BWD_FUSED_GRID, _code(dt) if dt in (torch.float32, torch.bfloat16) else -1, int(Cc), int(windows))


def attn_branch_bwd_supported(dt, Cc, nH, N, rows=0, windows=1):
    """the backward mode of the fused attention branch exists for this call: bf16, C = 96 = 3 heads of 32, 7x7 windows, inside the
    forward's buffer-range and window-count limits"""
    return (dt == torch.bfloat16 and int(Cc) == 96 and int(nH) == 3 and int(N) == 49 and attn_branch_supported(dt, Cc, nH, N, rows, windows)
            and attn_branch_bwd_grid(dt, Cc, max(int(windows), 1)) > 0)


def attn_branch_bwd_weights(Wqkv, Wproj):
    """the three bf16 copies the backward mode reads, from the fp32 masters: (qkv.weight [3C, C], its transpose [C, 3C], the transpose of
    proj.weight [C, C])"""
    return cast_weight(Wqkv), cast_weight(Wqkv, transpose=True), cast_weight(Wproj, transpose=True)


def attn_branch_bwd_workspaces(windows, nH, device):
    """partials and bias-gradient slabs for the calls of one block (its resolution groups, `windows` = their window counts), stacked so
    that the LAST call's finish (partial reduce, slab fold, table gather) serves them all -> (partials_ws [n, ATTN_BWD_PARTIAL_FLOATS], dbias_ws [n, nH, frag], firsts)"""
    grids = [attn_branch_bwd_grid(torch.bfloat16, 32 * nH, w) for w in windows]
    assert all(g_ > 0 for g_ in grids)
    n = sum(grids)
    firsts = [sum(grids[:i]) for i in range(len(grids))]
    return (torch.empty((n, ATTN_BWD_PARTIAL_FLOATS), dtype=torch.float32, device=device),
            torch.empty((n, nH, attn_frag_elems(49)), dtype=torch.float32, device=device), firsts)


def attn_branch_bwd(x, gin, gamma, beta, eps, weights, bqkv, win2tok, L, ws, region_ids, nW, N, nH, scale, *, bias_frag, rowscale=None,
                    rowscale_out=None, out=None, workspaces=None, first_partial=0, finish=True, gx_out=None, gx_act_out=None,
                    index=None, dtable=None, table_rows=0):
    """backward of attn_branch_fwd for one resolution group in one kernel: x fp32 [nB*L, C] (the branch input), gin = dL/dx1 fp32 ->
    (gx fp32, gx_act bf16 = cast(rowscale_out * gx) or None, (dWqkv, dbqkv, dWproj, dbproj, dgamma, dbeta), dbias_ws, dtable or None).
    weights = attn_branch_bwd_weights(...); bias_frag: the block's filled fragment-order bias.  out: the six fp32 tensors to write the
    gradients to (each or any None).  workspaces = (partials_ws, dbias_ws) of attn_branch_bwd_workspaces with this call's first_partial;
    finish=False leaves the reduce to a later call of the same block (the gradients are then not yet written), finish=True sums every
    partial up to and including this call's.  index (the relative-position index) with table_rows, or a dtable fp32 [table_rows, nH] to write
    to: the finishing call also sums the slabs and gathers the table's gradient, without atomics (bit-reproducible, unlike relpos_bias_bwd without ordered=True,
    which the slabs may go to instead).  gx_out / gx_act_out: row slices of a block's matrices
    to write gx / gx_act to."""
    x, gin = _f32c(x), _f32c(gin)
    rows, Cc = x.shape
    nB = rows // L
    Wq, WqT, WpT = weights
    dev = x.device
    assert gin.shape == x.shape and rows == nB * L and Wq.shape == (3 * Cc, Cc) and WqT.shape == (Cc, 3 * Cc) and WpT.shape == (Cc, Cc)
    assert Wq.dtype == WqT.dtype == WpT.dtype == torch.bfloat16 and Wq.is_contiguous() and WqT.is_contiguous() and WpT.is_contiguous()
    grid = attn_branch_bwd_grid(torch.bfloat16, Cc, nB * nW)
    if grid <= 0:
        raise RuntimeError("attn_branch_bwd: no backward mode of the fused attention branch at C = %d" % Cc)
    shapes = ((3 * Cc, Cc), (3 * Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,))
    outs = list(out) if out is not None else [None] * 6
    for i, sh in enumerate(shapes):
        if outs[i] is None:
            outs[i] = torch.empty(sh, dtype=torch.float32, device=dev)
        assert tuple(outs[i].shape) == sh
        _f32c(outs[i])
    if workspaces is None:
        part, dbias, _ = attn_branch_bwd_workspaces([nB * nW], nH, dev)
        first_partial = 0
    else:
        part, dbias = workspaces
    assert part.shape[0] >= first_partial + grid and dbias.shape[0] == part.shape[0] and part.shape[1] == ATTN_BWD_PARTIAL_FLOATS
    for r_ in (rowscale, rowscale_out):
        assert r_ is None or (r_.shape == (rows,) and r_.dtype == torch.float32 and r_.is_contiguous())
    gx = torch.empty_like(x) if gx_out is None else _f32c(gx_out)
    gxa = gx_act_out
    assert gx.shape == x.shape and (gxa is None or (gxa.shape == x.shape and gxa.dtype == torch.bfloat16 and gxa.is_contiguous()))
    if finish and index is not None:
        if dtable is None:
            dtable = torch.empty((int(table_rows), nH), dtype=torch.float32, device=dev)
        assert index.dtype == torch.int64 and index.is_contiguous() and index.numel() == N * N and dtable.shape[1] == nH
        _f32c(dtable)
    else:
        dtable = None
    a = lambda t: None if t is None else _p(t).value  # noqa: E731
    d = AttnBwdDesc(a(gin), a(rowscale_out), a(gx), a(gxa), a(WqT), a(outs[0]), a(outs[1]), a(outs[2]), a(outs[3]), a(outs[4]), a(outs[5]),
                    a(_f32c(dbias)), a(_f32c(part)), int(first_partial), int(first_partial + grid) if finish else 0, a(index if dtable is not None else None),
                    a(dtable), 0 if dtable is None else int(dtable.shape[0]))
    check(lib.esvit_attn_branch_fwd(BF16, _p(x), _p(_f32c(gamma)), _p(_f32c(beta)), eps, _p(Wq), _p(_f32c(bqkv)), _p(WpT), None, _p(win2tok), L, None, ws,
                                    _p(_f32c(bias_frag)), _p(region_ids), nW, nB, N, nH, scale, _p(rowscale), None, None, None, None, None, None,
                                    _stream(), C.byref(d)), "attn_branch_bwd")
    return gx, gxa, tuple(outs), dbias, dtable


def attn_dbias_slabs(N, windows, nH, device):
    """One buffer for the bias-gradient slabs of several window_attn_bwd calls over the same window size (the resolution groups of a
    ragged block), so that ONE relpos_bias_bwd folds and scatters them all: -> (buffer [sum of parts, nH, frag], its per-call slices).
    windows: the calls' window counts (nB * nW)"""
    parts = [query(Q_ATTN_BWD_PARTS, N, w, nH) for w in windows]
    buf = torch.empty((sum(parts), nH, attn_frag_elems(N)), dtype=torch.float32, device=device)
    out, at = [], 0
    for p_ in parts:
        out.append(buf[at:at + p_])
        at += p_
    return buf, out


ATTN_BWD_OPTIONAL_DBIAS = True  # window_attn_bwd takes want_dbias (functional._no_dbias)
ATTN_SPLIT_DBIAS = 0x10000000  # ESVIT_ATTN_SPLIT_DBIAS: OR'd into ws of esvit_window_attn_bwd, the separate bias-gradient kernel at head_dim 32 too


def window_attn_bwd(qkv, qkv_bias, win2tok, L, dout, fwd_out, lse, rel_table, ws, region_ids, nW, N, nH, scale, dqkv_out=None, bias_frag=None,
                    dbias_out=None, want_dbias=True):
    """-> (dqkv act [nB*L, 3C], dbias_ws fp32 [parts, nH, frag], dpad_ws fp32 [rows, 2C]).  dbias_out: this call's slice of attn_dbias_slabs.
    want_dbias=False (a caller without a table; windows of more than 64 tokens at head_dim 64 only, where the bias gradient is a kernel
    of its own -- the library refuses it elsewhere): no slabs, None in their place.  ws may carry ATTN_SPLIT_DBIAS"""
    qkv, dout = _actc(qkv), _actc(dout)
    rows, C3 = qkv.shape
    Cc = C3 // 3
    nB = rows // L
    code = _code(qkv.dtype)
    dqkv = torch.empty_like(qkv) if dqkv_out is None else dqkv_out
    assert dqkv.shape == qkv.shape and dqkv.dtype == qkv.dtype and dqkv.is_contiguous()
    parts = query(Q_ATTN_BWD_PARTS, N, nB * nW, nH)
    if not want_dbias:
        assert dbias_out is None
        dbias_ws = None
    elif dbias_out is None:
        dbias_ws = torch.empty((parts, nH, attn_frag_elems(N)), dtype=torch.float32, device=qkv.device)
    else:
        dbias_ws = _f32c(dbias_out)
        assert tuple(dbias_ws.shape) == (parts, nH, attn_frag_elems(N)), (dbias_ws.shape, parts, nH)
    # the <= 64-token kernel writes every element of its pad-row slab itself; the 14x14 kernels fill one head's slice per row
    alloc = torch.empty if N <= 64 else torch.zeros
    pad = alloc((query(Q_ATTN_BWD_PAD_ROWS, N, nB * nW, nH | (code << 32)), 2 * Cc), dtype=torch.float32, device=qkv.device)
    bias_ws = bias_frag if bias_frag is not None else workspace(2 * nH * attn_frag_elems(N), qkv.device, slot=2)
    assert rel_table is not None or bias_frag is not None
    check(lib.esvit_window_attn_bwd(code, _p(qkv), _p(_f32c(qkv_bias)), _p(win2tok), L, _p(dout), _p(fwd_out), _p(lse), _p(None if rel_table is None else _f32c(rel_table)),
                                    ws, _p(bias_ws), _p(region_ids), nW, nB, N, nH, Cc // nH, scale, _p(dqkv), _p(dbias_ws), _p(pad),
                                    _stream()), "window_attn_bwd")
    return dqkv, dbias_ws, pad


RELPOS_ORDERED = 0x100  # ESVIT_RELPOS_ORDERED: OR'd into accumulate of esvit_relpos_bias_bwd
RELPOS_BWD_ORDERED = True  # relpos_bias_bwd takes ordered (functional._relpos_kw)


def relpos_bias_bwd(dbias_ws, index, N, table_rows, out=None, accumulate=None, ordered=False):
    """out: optional fp32 [table_rows, nH]; accumulate (default: True when out is given -- the second resolution group of a
    ragged block) adds to it, False overwrites it (a gradient-bucket slot written for the first time).
    ordered: the fixed-order form without atomics (bit-reproducible); it leaves the slabs' sum in dbias_ws[0]"""
    parts, nH, _ = dbias_ws.shape
    if index.shape[-1] != N:  # N < ws^2 (a ViT crop on the first N positions of the grid): the kernel reads index[q * N + key]
        index = index[:N, :N].contiguous()
    assert index.dtype == torch.int64 and index.is_contiguous() and tuple(index.shape) == (N, N), (index.dtype, index.shape, N)
    dtable = torch.empty((table_rows, nH), dtype=torch.float32, device=dbias_ws.device) if out is None else _f32c(out)
    acc = (out is not None) if accumulate is None else (bool(accumulate) and out is not None)
    if ordered:
        _f32c(dbias_ws)
    check(lib.esvit_relpos_bias_bwd(_p(dbias_ws), parts, _p(index), N, nH, table_rows, _p(dtable), int(acc) | (RELPOS_ORDERED if ordered else 0),
                                    _stream()), "relpos_bias_bwd")
    return dtable


# ------------------------------------------------------------------------------------------------
# DINOHead pieces
# ------------------------------------------------------------------------------------------------
def l2norm_fwd(x):
    x = _actc(x)
    R, D = x.shape
    z = torch.empty_like(x)
    inv = torch.empty((R,), dtype=torch.float32, device=x.device)
    check(lib.esvit_l2norm_fwd(_code(x.dtype), _p(x), R, D, _p(z), _p(inv), _stream()), "l2norm_fwd")
    return z, inv


def l2norm_bwd(dz, z, inv):
    dz, z = _actc(dz), _actc(z)
    R, D = z.shape
    dx = torch.empty_like(z)
    check(lib.esvit_l2norm_bwd(_code(z.dtype), _p(dz), _p(z), _p(inv), R, D, _p(dx), _stream()), "l2norm_bwd")
    return dx


def weightnorm_fwd(v, g, dtype=None):
    """v fp32 [K, D], g fp32 [K, 1] -> (w act [K, D], inv_norm fp32 [K])."""
    v, g = _f32c(v), _f32c(g)
    K, D = v.shape
    dt = dtype or _ACT_DTYPE
    w = torch.empty((K, D), dtype=dt, device=v.device)
    inv = torch.empty((K,), dtype=torch.float32, device=v.device)
    check(lib.esvit_weightnorm_fwd(_code(dt), _p(v), _p(g), K, D, _p(w), None, _p(inv), _stream()), "weightnorm_fwd")
    return w, inv


def weightnorm_bwd(dw, v, g, inv, need_dg, dv_out=None):
    dw, v, g = _f32c(dw), _f32c(v), _f32c(g)
    K, D = v.shape
    dv = torch.empty_like(v) if dv_out is None else _f32c(dv_out)
    assert dv.shape == v.shape
    dg = torch.empty((K, 1), dtype=torch.float32, device=v.device) if need_dg else None
    check(lib.esvit_weightnorm_bwd(_p(dw), _p(v), _p(g), _p(inv), K, D, _p(dv), _p(dg), _stream()), "weightnorm_bwd")
    return dv, dg


# ------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------
def teacher_row_stats(t, center, inv_temp):
    t = _actc(t)
    R, K = t.shape
    mx = torch.empty((R,), dtype=torch.float32, device=t.device)
    lse = torch.empty_like(mx)
    check(lib.esvit_teacher_row_stats(_code(t.dtype), _p(t), _p(center), inv_temp, R, K, _p(mx), _p(lse), _stream()),
          "teacher_row_stats")
    return mx, lse


def rowstat_combine(st):
    """fold the block statistics the last-layer GEMM leaves behind (esvit_gemm_desc::rowstat: fp32 [R, nb, 2] pairs of a block's
    maximum in base-2 units and its sum of 2^(z - max)) into the natural-log (row_max, row_lse) of teacher_row_stats"""
    st = _f32c(st)
    R, nb, two = st.shape
    assert two == 2
    mx = torch.empty((R,), dtype=torch.float32, device=st.device)
    lse = torch.empty_like(mx)
    check(lib.esvit_rowstat_combine(_p(st), R, nb, _p(mx), _p(lse), _stream()), "rowstat_combine")
    return mx, lse


def region_match(sim, Tt, crop_id, cm_row, tmatch):
    """sim fp32 [B, S, ld]; writes tmatch (int32 [rows, 2]) in place."""
    sim = _f32c(sim)
    B, S, ld = sim.shape
    check(lib.esvit_region_match(_p(sim), B, S, Tt, ld, _p(crop_id), _p(cm_row), _p(tmatch), _stream()), "region_match")
    return tmatch


def dino_ce(s, t, center, t_max, t_lse, tmatch, row_w, inv_student_temp, inv_teacher_temp, row_loss=None, term_w=None, row_order=None,
            s_stats=None):
    """-> (row_loss fp32 [Rs], ds act [Rs, K]).  tmatch int32 [Rs, 2] with one weight row_w[r] for both terms, or (mixup
    targets) tmatch [Rs, 4] with term_w fp32 [Rs, 4], one weight per term.  s_stats = (row_max, row_lse) of s * inv_student_temp
    (linear_fwd(row_stats=(inv_student_temp, None))) spares the kernel its first pass over the student rows."""
    s, t = _actc(s), _actc(t)
    Rs, K = s.shape
    assert t.shape[1] == K and s.dtype == t.dtype and tmatch.dtype == torch.int32
    if row_loss is None:
        row_loss = torch.empty((Rs,), dtype=torch.float32, device=s.device)
    assert row_loss.numel() == Rs and row_loss.is_contiguous()
    ds = torch.empty_like(s)
    terms = 2 if term_w is None else 4
    assert row_order is None or (row_order.dtype == torch.int32 and row_order.numel() == Rs and row_order.is_contiguous())
    assert tmatch.numel() == Rs * terms and tmatch.is_contiguous() and (term_w is None or (term_w.numel() == Rs * 4 and term_w.is_contiguous()))
    s_mx, s_lse = (None, None) if s_stats is None else s_stats
    assert s_stats is None or (term_w is None and s_mx.numel() == Rs and s_lse.numel() == Rs and s_mx.dtype == s_lse.dtype == torch.float32)
    check(lib.esvit_dino_ce_fwd_bwd(_code(s.dtype), _p(s), _p(t), _p(center), _p(t_max), _p(t_lse), _p(tmatch), _p(row_w), terms,
                                    _p(term_w), inv_student_temp, inv_teacher_temp, Rs, K, _p(row_loss), _p(ds), _p(row_order), _p(s_mx),
                                    _p(s_lse), _stream()),
          "dino_ce_fwd_bwd")
    return row_loss, ds


def probe_ce(logits, targets, row_w, row_loss=None, want_grad=True, inplace=True):
    """class-index cross-entropy of G classifiers sharing a batch (esvit_dino_ce_fwd_bwd, terms = 0).  logits fp32 [Rs, C] (the
    [B, G * C] GEMM output viewed as Rs = B * G rows), targets int32 [Rs], row_w fp32 [Rs] (the gradient scale of each row).
    -> (row_loss fp32 [Rs, 2] = (lse - z_t, rank of the target), dlogits): dlogits is `logits` itself overwritten (inplace), a new
    tensor, or None with want_grad=False (validation: the logits are left as they are)."""
    logits = _f32c(logits)
    Rs, C = logits.shape
    assert targets.dtype == torch.int32 and targets.numel() == Rs and targets.is_contiguous()
    if row_loss is None:
        row_loss = torch.empty((Rs, 2), dtype=torch.float32, device=logits.device)
    assert row_loss.numel() == 2 * Rs and row_loss.is_contiguous() and row_loss.dtype == torch.float32
    ds = None
    if want_grad:
        assert row_w is not None and row_w.numel() == Rs
        row_w = _f32c(row_w)
        ds = logits if inplace else torch.empty_like(logits)
    check(lib.esvit_dino_ce_fwd_bwd(_code(logits.dtype), _p(logits), None, None, None, None, _p(targets), _p(row_w), 0, None, 1.0, 1.0, Rs, C,
                                    _p(row_loss), _p(ds), None, None, None, _stream()),
          "dino_ce_fwd_bwd(class index)")
    return row_loss, ds


def dist_stats_slab():
    """rows one workgroup of dist_stats owns (its column-sum partials: one per slab)"""
    return query(Q_DIST_STATS, 0)


def dist_stats(x, center, inv_temp, stats, buf=None):
    """distribution statistics of the softmax rows p = softmax((x - center) * inv_temp) (esvit_dino_ce_fwd_bwd, terms = -1): x act
    [R, K] read once, center fp32 [K] or None, stats = (row_max, row_lse) of the rows (teacher_row_stats / rowstat_combine)
    -> (ent fp32 [R] in nats, amax int32 [R]: lowest index of the maximum, -1 for a row with NaN / inf in it, psum fp32 [K] = sum_r p_rk).
    buf: an fp32 tensor of query(Q_DIST_STATS, R, K) floats to work in (psum is its head), else one is allocated."""
    x = _actc(x)
    R, K = x.shape
    mx, lse = stats
    assert mx.numel() == R and lse.numel() == R and mx.dtype == lse.dtype == torch.float32 and mx.is_contiguous() and lse.is_contiguous()
    if center is not None:
        center = _f32c(center)
        assert center.numel() == K
    n = query(Q_DIST_STATS, R, K)
    if n <= 0:
        raise RuntimeError("esvit_query(Q_DIST_STATS) failed (%d): %s" % (n, lib.esvit_last_error().decode()))
    if buf is None:
        buf = torch.empty((n,), dtype=torch.float32, device=x.device)
    assert buf.dtype == torch.float32 and buf.numel() >= n and buf.is_contiguous()
    out = torch.empty((R, 2), dtype=torch.float32, device=x.device)
    check(lib.esvit_dino_ce_fwd_bwd(_code(x.dtype), _p(x), None, _p(center), None, None, None, None, -1, None, float(inv_temp), 1.0, R, K,
                                    _p(out), _p(buf), None, _p(mx), _p(lse), _stream()),
          "dino_ce_fwd_bwd(row statistics)")
    return out[:, 0], out[:, 1].to(torch.int32), buf[:K]


def probe_ce_reg_row():
    """longest row the class-index CE keeps in registers; longer rows take the workgroup-per-row kernel"""
    return query(Q_PROBE_CE_REG_ROW)


def sum_f32(x):
    x = _f32c(x)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    check(lib.esvit_sum_f32(_p(x), x.numel(), _p(out), _stream()), "sum_f32")
    return out


def scale_inplace(x, scale):
    x = _actc(x)
    check(lib.esvit_scale_inplace(_code(x.dtype), _p(x), x.numel(), _p(_f32c(scale)), _stream()), "scale_inplace")
    return x


def center_ema(center, colsum_, momentum, denom):
    check(lib.esvit_center_ema(_p(_f32c(center)), _p(_f32c(colsum_)), momentum, float(denom), center.numel(), _stream()),
          "center_ema")
    return center


# ------------------------------------------------------------------------------------------------
# fused update
# ------------------------------------------------------------------------------------------------
def update_chunk_elems():
    return query(Q_UPDATE_CHUNK_ELEMS)


RULE_ADAMW, RULE_SGD, RULE_LARS, RULE_SGD_MEMBERS = 0, 1, 2, 3


SQNORM_ORDERED = 0x100  # ESVIT_SQNORM_ORDERED: OR'd into stats of esvit_grad_sqnorm


def grad_sqnorm(tensors, ntensors, chunks, nchunks, sqnorms, stats=1, ordered=False):
    """ordered: the fixed-order form without atomics (bit-reproducible); sqnorms is then fp32 [ntensors * stats + nchunks * stats],
    the statistics in its head, per-chunk partials behind them"""
    if ordered:
        assert sqnorms.dtype == torch.float32 and sqnorms.is_contiguous() and sqnorms.numel() >= (ntensors + nchunks) * int(stats), sqnorms.shape
    check(lib.esvit_grad_sqnorm(_p(tensors), ntensors, _p(chunks), nchunks, int(stats) | (SQNORM_ORDERED if ordered else 0), _p(sqnorms), _stream()),
          "grad_sqnorm")


def fused_clip_update_ema(rule, tensors, ntensors, chunks, nchunks, sqnorms, clip, lr, wd, beta1, beta2, eps, ema_m, skipped=None):
    """rule AdamW: (beta1, beta2, eps); SGD: beta1 = momentum; LARS: beta1 = momentum, beta2 = eta; SGD_MEMBERS: beta1 = momentum, lr and
    wd per tensor in the table's slot 9, the member id in the upper half of the flags slot, `skipped` int32 [members] required"""
    check(lib.esvit_fused_clip_update_ema(int(rule), _p(tensors), ntensors, _p(chunks), nchunks, _p(sqnorms), clip, lr, wd, beta1, beta2,
                                          eps, ema_m, _p(skipped), _stream()), "fused_clip_update_ema")


# ------------------------------------------------------------------------------------------------
# CvT backbone pieces (cvt_v4_transformer.py): ConvEmbed im2col, depthwise 3x3, BatchNorm reductions
# ------------------------------------------------------------------------------------------------
def conv_out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


IM2COL_OUT = True  # conv_im2col / conv_col2im take `out=` (a row slice of a larger matrix: the ragged multi-crop ConvEmbed)


def conv_im2col(src, nchw, nB, H, W, Cin, k, stride, pad, dtype=None, out=None):
    """-> cols [nB*Ho*Wo, Kpad] (Kpad = k*k*Cin rounded up to 8), column order (ky, kx, c).
    src: fp32 NCHW images (nchw=True) or activation-dtype NHWC tokens [nB*H*W, Cin]."""
    dt = dtype or (_ACT_DTYPE if nchw else src.dtype)
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    Kpad = -(-(k * k * Cin) // 8) * 8
    assert src.is_contiguous() and (src.dtype == torch.float32 if nchw else src.dtype == dt)
    cols = torch.empty((nB * Ho * Wo, Kpad), dtype=dt, device=src.device) if out is None else out
    assert cols.shape == (nB * Ho * Wo, Kpad) and cols.dtype == dt and cols.is_contiguous()
    check(lib.esvit_conv_im2col(_code(dt), _p(src), int(bool(nchw)), nB, H, W, Cin, k, stride, pad, Ho, Wo, Kpad, _p(cols), _stream()),
          "conv_im2col")
    return cols


def conv_col2im(dcols, nB, H, W, Cin, k, stride, pad, out=None):
    """adjoint of conv_im2col for NHWC sources: dcols act [nB*Ho*Wo, Kpad] -> dsrc fp32 [nB*H*W, Cin]."""
    dcols = _actc(dcols)
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    dsrc = torch.empty((nB * H * W, Cin), dtype=torch.float32, device=dcols.device) if out is None else _f32c(out)
    assert dsrc.shape == (nB * H * W, Cin)
    check(lib.esvit_conv_col2im(_code(dcols.dtype), _p(dcols), nB, H, W, Cin, k, stride, pad, Ho, Wo, dcols.shape[1], _p(dsrc), _stream()),
          "conv_col2im")
    return dsrc


def dwconv3x3(x, w, nB, H, W, flip=False):
    """depthwise 3x3, stride 1, zero pad 1 on NHWC tokens x [nB*H*W, C] (act); w fp32 [C, 9]; flip: mirrored taps."""
    x = _actc(x)
    Cc = x.shape[1]
    assert x.shape[0] == nB * H * W and w.numel() == 9 * Cc
    y = torch.empty_like(x)
    check(lib.esvit_dwconv3x3(_code(x.dtype), _p(x), _p(_f32c(w)), int(bool(flip)), nB, H, W, Cc, _p(y), _stream()), "dwconv3x3")
    return y


def dwconv3x3_wgrad(x, dy, nB, H, W):
    """-> dw fp32 [C, 9]"""
    x, dy = _actc(x), _actc(dy)
    Cc = x.shape[1]
    assert x.dtype == dy.dtype and x.shape == dy.shape
    dw = torch.empty((Cc, 9), dtype=torch.float32, device=x.device)
    ws = workspace(query(Q_COL_REDUCE_BLOCKS, nB * H * W) * 9 * Cc, x.device, slot=1)
    check(lib.esvit_dwconv3x3_wgrad(_code(x.dtype), _p(x), _p(dy), nB, H, W, Cc, _p(dw), _p(ws), _stream()), "dwconv3x3_wgrad")
    return dw


def col_sums2(a, b):
    """-> fp32 [2, C]: sum_r a[r, c]  and  sum_r a[r, c] * b[r, c]"""
    a, b = _actc(a), _actc(b)
    rows, Cc = a.shape
    assert a.dtype == b.dtype and a.shape == b.shape
    out = torch.empty((2, Cc), dtype=torch.float32, device=a.device)
    ws = workspace(query(Q_COL_REDUCE_BLOCKS, rows) * 2 * Cc, a.device, slot=1)
    check(lib.esvit_col_sums2(_code(a.dtype), _p(a), _p(b), rows, Cc, _p(out), _p(ws), _stream()), "col_sums2")
    return out


def col_affine2(x1, a1, a3, x2=None, a2=None, act=0):
    """act 0: y = a1[c] * x1 + a2[c] * x2 + a3[c];  1: y = GELU(a1[c] * x1 + a3[c]);  2: y = x2 * GELU'(a1[c] * x1 + a3[c]);
    3: y = max(a1[c] * x1 + a3[c], 0);  4: y = x2 where a1[c] * x1 + a3[c] > 0 else 0  (act dtype in / out, fp32 coefficients)"""
    x1 = _actc(x1)
    rows, Cc = x1.shape
    assert a1.numel() == Cc and a3.numel() == Cc, (a1.shape, a3.shape, Cc)
    if x2 is not None:
        assert x2.dtype == x1.dtype and x2.shape == x1.shape and x2.is_contiguous(), (x2.dtype, tuple(x2.shape), x2.is_contiguous())
    if a2 is not None:
        assert _f32c(a2).numel() == Cc, (a2.shape, Cc)
    y = torch.empty_like(x1)
    check(lib.esvit_col_affine2(_code(x1.dtype), _p(x1), _p(x2), rows, Cc, _p(_f32c(a1)), _p(a2), _p(_f32c(a3)), int(act), _p(y), _stream()),
          "col_affine2")
    return y


def bn_fwd_coeffs(sums, n, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """sums fp32 [2, C] (sum d, sum d^2; already summed over the ranks) -> coef fp32 [4, C] = (a, shift, mean, rstd)"""
    Cc = gamma.numel()
    coef = torch.empty((4, Cc), dtype=torch.float32, device=sums.device)
    check(lib.esvit_bn_fwd_coeffs(_p(_f32c(sums)), float(n), _p(_f32c(gamma)), _p(_f32c(beta)), float(eps), float(momentum),
                                  _p(running_mean), _p(running_var), Cc, _p(coef), _stream()), "bn_fwd_coeffs")
    return coef


def bn_eval_coeffs(running_mean, running_var, gamma, beta, eps):
    Cc = gamma.numel()
    coef = torch.empty((4, Cc), dtype=torch.float32, device=gamma.device)
    check(lib.esvit_bn_eval_coeffs(_p(_f32c(running_mean)), _p(_f32c(running_var)), _p(_f32c(gamma)), _p(_f32c(beta)), float(eps), Cc,
                                   _p(coef), _stream()), "bn_eval_coeffs")
    return coef


def bn_bwd_local(sums, coef):
    """sums fp32 [2, C] (sum dy, sum dy*d) -> red fp32 [2, C] (sum dy, sum dy*xhat)"""
    Cc = coef.shape[1]
    red = torch.empty((2, Cc), dtype=torch.float32, device=sums.device)
    check(lib.esvit_bn_bwd_local(_p(_f32c(sums)), _p(_f32c(coef)), Cc, _p(red), _stream()), "bn_bwd_local")
    return red


def bn_bwd_coeffs(red, n, gamma, coef):
    """-> abc fp32 [3, C]: d(d) = A*dy + B*d + C (red=None: fixed / eval statistics)"""
    Cc = coef.shape[1]
    abc = torch.empty((3, Cc), dtype=torch.float32, device=coef.device)
    check(lib.esvit_bn_bwd_coeffs(_p(red), float(n), _p(_f32c(gamma)), _p(_f32c(coef)), Cc, _p(abc), _stream()), "bn_bwd_coeffs")
    return abc


def pad_crop_tokens(src, nB, Hs, Ws, Hd, Wd):
    """[nB*Hs*Ws, C] -> [nB*Hd*Wd, C]: zero-pad at the bottom / right, or crop"""
    src = _actc(src)
    Cc = src.shape[1]
    dst = torch.empty((nB * Hd * Wd, Cc), dtype=src.dtype, device=src.device)
    check(lib.esvit_pad_crop_tokens(_code(src.dtype), _p(src), nB, Hs, Ws, Hd, Wd, Cc, _p(dst), _stream()), "pad_crop_tokens")
    return dst


# ---- grouped mode of the four spatial kernels (include/esvit_hip.h): the resolution groups of a ragged multi-crop step in one launch ----
def _grid_groups(recs):
    """recs: list of dicts of esvit_grid_group fields (tensors for the pointers) -> (host record array, -G)"""
    assert 1 <= len(recs) <= MAX_GRID_GROUPS, len(recs)
    arr = (GridGroup * len(recs))()
    for r, d in zip(arr, recs):
        for k, v in d.items():
            setattr(r, k, _p(v) if k in ("p0", "p1", "out", "a1", "a2", "a3") else int(v))
    return arr, -len(recs)


def _group_outs(outs, shapes, dt, device):
    """outs: None (allocate) or one tensor per group -- e.g. row slices of one matrix"""
    if outs is None:
        return [torch.empty(sh, dtype=dt, device=device) for sh in shapes]
    assert len(outs) == len(shapes) and all(t.shape == tuple(sh) and t.dtype == dt and t.is_contiguous() for t, sh in zip(outs, shapes))
    return list(outs)


def pad_crop_tokens_grouped(srcs, geos, outs=None):
    """pad_crop_tokens of every group in one launch; geos: (nB, Hs, Ws, Hd, Wd) per group -> list of [nB*Hd*Wd, C]"""
    srcs = [_actc(t) for t in srcs]
    Cc, dt = srcs[0].shape[1], srcs[0].dtype
    assert all(t.shape[1] == Cc and t.dtype == dt for t in srcs)
    assert all(t.shape[0] == nB * Hs * Ws for t, (nB, Hs, Ws, Hd, Wd) in zip(srcs, geos))
    dsts = _group_outs(outs, [(nB * Hd * Wd, Cc) for (nB, Hs, Ws, Hd, Wd) in geos], dt, srcs[0].device)
    arr, negG = _grid_groups([dict(p0=t, out=d, nB=nB, H=Hs, W=Ws, Hd=Hd, Wd=Wd, C=Cc, dtype=_code(dt))
                              for t, d, (nB, Hs, Ws, Hd, Wd) in zip(srcs, dsts, geos)])
    check(lib.esvit_pad_crop_tokens(_code(dt), C.c_void_p(C.addressof(arr)), negG, 0, 0, 0, 0, Cc, None, _stream()), "pad_crop_tokens(grouped)")
    return dsts


def dwconv3x3_grouped(xs, w, geos, flip=False, outs=None):
    """dwconv3x3 of every group in one launch; geos: (nB, H, W) per group -> list of y"""
    xs = [_actc(t) for t in xs]
    Cc, dt = xs[0].shape[1], xs[0].dtype
    assert all(t.shape == (nB * H * W, Cc) and t.dtype == dt for t, (nB, H, W) in zip(xs, geos)) and w.numel() == 9 * Cc
    ys = _group_outs(outs, [t.shape for t in xs], dt, xs[0].device)
    arr, negG = _grid_groups([dict(p0=t, out=y, nB=nB, H=H, W=W, C=Cc, dtype=_code(dt)) for t, y, (nB, H, W) in zip(xs, ys, geos)])
    check(lib.esvit_dwconv3x3(_code(dt), C.c_void_p(C.addressof(arr)), _p(_f32c(w)), int(bool(flip)), negG, 0, 0, Cc, None, _stream()), "dwconv3x3(grouped)")
    return ys


def col_sums2_grouped(a_list, b_list):
    """col_sums2 of every group in one launch -> fp32 [G, 2, C]; row g has the bits of col_sums2(a_list[g], b_list[g])"""
    a_list, b_list = [_actc(t) for t in a_list], [_actc(t) for t in b_list]
    Cc, dt = a_list[0].shape[1], a_list[0].dtype
    assert all(a.shape == b.shape and a.dtype == dt and b.dtype == dt and a.shape[1] == Cc for a, b in zip(a_list, b_list))
    out = torch.empty((len(a_list), 2, Cc), dtype=torch.float32, device=a_list[0].device)
    ws = workspace(sum(query(Q_COL_REDUCE_BLOCKS, a.shape[0]) for a in a_list) * 2 * Cc, a_list[0].device, slot=1)
    arr, negG = _grid_groups([dict(p0=a, p1=b, nB=a.shape[0], H=1, W=1, C=Cc, dtype=_code(dt)) for a, b in zip(a_list, b_list)])
    check(lib.esvit_col_sums2(_code(dt), C.c_void_p(C.addressof(arr)), None, negG, Cc, _p(out), _p(ws), _stream()), "col_sums2(grouped)")
    return out


def col_affine2_grouped(x1s, a1s, a3s, x2s=None, a2s=None, act=0, outs=None):
    """col_affine2 of every group (its own coefficient vectors) in one launch -> list of y"""
    x1s = [_actc(t) for t in x1s]
    Cc, dt = x1s[0].shape[1], x1s[0].dtype
    n = len(x1s)
    x2s = [None] * n if x2s is None else list(x2s)
    a2s = [None] * n if a2s is None else [None if a is None else _f32c(a) for a in a2s]
    a1s, a3s = [_f32c(a) for a in a1s], [_f32c(a) for a in a3s]
    for x1, x2, a1, a2, a3 in zip(x1s, x2s, a1s, a2s, a3s):
        assert x1.shape[1] == Cc and x1.dtype == dt and a1.numel() == Cc and a3.numel() == Cc and (a2 is None or a2.numel() == Cc)
        assert x2 is None or (x2.dtype == dt and x2.shape == x1.shape and x2.is_contiguous())
    ys = _group_outs(outs, [t.shape for t in x1s], dt, x1s[0].device)
    arr, negG = _grid_groups([dict(p0=x1, p1=x2, out=y, a1=a1, a2=a2, a3=a3, nB=x1.shape[0], H=1, W=1, C=Cc, dtype=_code(dt))
                              for x1, x2, y, a1, a2, a3 in zip(x1s, x2s, ys, a1s, a2s, a3s)])
    check(lib.esvit_col_affine2(_code(dt), C.c_void_p(C.addressof(arr)), None, negG, Cc, None, None, None, int(act), None, _stream()), "col_affine2(grouped)")
    return ys


# ------------------------------------------------------------------------------------------------
# crop producer (datasets/build.py:203-261)
# ------------------------------------------------------------------------------------------------
AUG_PARAM_INTS = 24


def aug_max_box(S):
    """largest crop-box side aug_crops can resize to S x S"""
    return query(Q_AUG_MAX_BOX, S)


def aug_crops(src, images, params, S, max_h, max_w, planes=None, out=None):
    """DataAugmentationDINO for the n crops of one output size S described by ``params`` (int32 [n, 24], include/esvit_hip.h):
    src uint8 packed HWC images (readable up to the next 4-byte boundary), images int64 [n_img, 3] (byte offset, H, W).
    ``planes``: uint8 scratch of n * (3 S^2 + 4) bytes.  Returns (out fp32 [n, 3, S, S], uint8 [n, 3, S, S] view of the scratch =
    the resized, flipped crops before the jitter)."""
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    assert images.is_cuda and images.dtype == torch.int64 and images.is_contiguous() and images.shape[-1] == 3
    assert params.is_cuda and params.dtype == torch.int32 and params.is_contiguous() and params.shape[-1] == AUG_PARAM_INTS
    n = params.shape[0]
    need = n * (3 * S * S + 4)
    if planes is None:
        planes = torch.empty(need, dtype=torch.uint8, device=src.device)
    if out is None:
        out = torch.empty((n, 3, S, S), dtype=torch.float32, device=src.device)
    assert planes.is_cuda and planes.dtype == torch.uint8 and planes.is_contiguous() and planes.numel() >= need
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n * 3 * S * S
    check(lib.esvit_aug_crops(_p(src), _p(images), _p(params), n, S, int(max_h), int(max_w), _p(planes), _p(out), _stream()), "aug_crops")
    return out, planes.view(-1)[:n * 3 * S * S].view(n, 3, S, S)


# evaluation input (eval_knn.py:48-53, eval_linear.py:50-61)
AUG_EVAL = 0x40000000  # ESVIT_AUG_EVAL: OR'd into S, selects the evaluation mode
RESIZE_PARAM_INTS = 16
RESIZE_SCALE_ONE = 65536
FILTER_BICUBIC, FILTER_BILINEAR = 0, 1


def _scale_fx(pair):
    """(box side, resized side) -> the ratio in units of 1 / RESIZE_SCALE_ONE, rounded up (exact integer arithmetic), capped"""
    box, resized = int(pair[0]), int(pair[1])
    return min((box * RESIZE_SCALE_ONE + resized - 1) // resized, 0x7FFFFFFF)


def resize_fits(scale_h, scale_w):
    """whether resize_crops takes a call whose largest per-axis scales are ``scale_h`` = (box h, resized h) and ``scale_w``"""
    return bool(query(Q_RESIZE_FITS, _scale_fx(scale_h), _scale_fx(scale_w)))


def resize_crops(src, images, params, S, scale_h, scale_w, out=None):
    """box -> resize -> S x S window -> flip -> ToTensor + Normalize for the n crops described by ``params`` (int32 [n, 16]; the
    evaluation mode of esvit_aug_crops, include/esvit_hip.h) from packed images as aug_crops reads them.  ``scale_h`` /
    ``scale_w``: the (box side, resized side) pair of the crop with the largest ratio on that axis.  Returns out fp32 [n, 3, S, S]."""
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    assert images.is_cuda and images.dtype == torch.int64 and images.is_contiguous() and images.shape[-1] == 3
    assert params.is_cuda and params.dtype == torch.int32 and params.is_contiguous() and params.shape[-1] == RESIZE_PARAM_INTS
    n = params.shape[0]
    if out is None:
        out = torch.empty((n, 3, S, S), dtype=torch.float32, device=src.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n * 3 * S * S
    check(lib.esvit_aug_crops(_p(src), _p(images), _p(params), n, S | AUG_EVAL, _scale_fx(scale_h), _scale_fx(scale_w), None, _p(out), _stream()),
          "resize_crops")
    return out


# ------------------------------------------------------------------------------------------------
# global attention of the monolithic ViT backbones (models/vision_transformer.py:67-94)
# ------------------------------------------------------------------------------------------------
def vit_pad_tokens(N):
    """tokens per image rounded up to the granularity the batched GEMMs need (k-strided operands: multiples of 16)"""
    return -(-N // 16) * 16


def heads_split(x, B, N, nH, parts):
    """x [B * N, parts * C] token-major -> [parts, B, nH, Np, hd] (pad rows zero)"""
    x = _actc(x)
    C_ = x.shape[1] // parts
    hd, Np = C_ // nH, vit_pad_tokens(N)
    y = torch.empty((parts, B, nH, Np, hd), dtype=x.dtype, device=x.device)
    check(lib.esvit_heads_split(_code(x.dtype), _p(x), B, N, Np, nH, hd, parts, _p(y), _stream()), "heads_split")
    return y


def heads_merge(y, N):
    """y [parts, B, nH, Np, hd] -> [B * N, parts * nH * hd] token-major"""
    y = _actc(y)
    parts, B, nH, Np, hd = y.shape
    x = torch.empty((B * N, parts * nH * hd), dtype=y.dtype, device=y.device)
    check(lib.esvit_heads_merge(_code(y.dtype), _p(y), B, N, Np, nH, hd, parts, _p(x), _stream()), "heads_merge")
    return x


def _bmm(a, b, M, N, K, *, a_kstrided=0, b_kstrided=0, out=None):
    """batched esvit_gemm over the leading axis of contiguous 3-D operands: out[z] = op(a[z]) @ op(b[z]) -> [Z, M, N]"""
    Z = a.shape[0]
    if out is None:
        out = torch.empty((Z, M, N), dtype=a.dtype, device=a.device)
    assert out.is_contiguous() and out.shape == (Z, M, N) and a.is_contiguous() and b.is_contiguous()
    _gemm(a.dtype, A=a, B=b, C=out, M=M, N=N, K=K, lda=a.shape[2], ldb=b.shape[2], ldc=N, a_kstrided=a_kstrided, b_kstrided=b_kstrided,
          batch=Z, strideA=a.shape[1] * a.shape[2], strideB=b.shape[1] * b.shape[2], strideC=M * N)
    return out


def vit_attn_fwd(qkv, B, N, nH, scale, chunk=None):
    """Attention.forward between the qkv and proj projections (vision_transformer.py:76-83): qkv [B * N, 3C] -> (out [B * N, C],
    saved = (q | k | v [3, B nH, Np, hd], P [B nH, Np, Np])).  chunk (int32 [N]): Vision Longformer's sliding-chunk neighbourhood
    (esvit_softmax_rows_chunked_fwd) instead of global attention; or (table, nglo, tokens per chunk row) when the local tokens are
    ordered chunk row by chunk row, which lets the kernels skip the chunk rows a query cannot see."""
    C_ = qkv.shape[1] // 3
    hd, Np = C_ // nH, vit_pad_tokens(N)
    qkvh = heads_split(qkv, B, N, nH, 3).view(3, B * nH, Np, hd)
    prob = _bmm(qkvh[0], qkvh[1], Np, Np, hd)                                  # S = q k^T
    if chunk is not None:
        tab, nglo, rowtok = chunk if isinstance(chunk, tuple) else (chunk, 0, 0)
        assert tab.dtype == torch.int32 and tab.numel() == N and tab.is_contiguous()
        check(lib.esvit_softmax_rows_chunked_fwd(_code(prob.dtype), _p(prob), B * nH, N, Np, float(scale), _p(tab), int(nglo), int(rowtok), _stream()),
              "softmax_rows_chunked_fwd")
    else:
        check(lib.esvit_softmax_rows_fwd(_code(prob.dtype), _p(prob), B * nH, N, Np, float(scale), _stream()), "softmax_rows_fwd")
    o = _bmm(prob, qkvh[2], Np, hd, Np, b_kstrided=1)                          # O = P v
    return heads_merge(o.view(1, B, nH, Np, hd), N), (qkvh, prob)


def vit_attn_bwd(dout, saved, B, N, nH, scale, chunk=None):
    """gradient of vit_attn_fwd with respect to qkv: dout [B * N, C] -> dqkv [B * N, 3C] (chunk: as given to the forward; only the
    (table, nglo, tokens per chunk row) form changes anything -- the backward then skips the columns that are zero in P)"""
    qkvh, prob = saved
    _, Z, Np, hd = qkvh.shape
    do = heads_split(dout, B, N, nH, 1).view(Z, Np, hd)
    dqkvh = torch.empty_like(qkvh)
    _bmm(prob, do, Np, hd, Np, a_kstrided=1, b_kstrided=1, out=dqkvh[2])      # dv = P^T dO
    dp = _bmm(do, qkvh[2], Np, Np, hd)                                         # dP = dO v^T
    if isinstance(chunk, tuple) and chunk[2] > 0:
        check(lib.esvit_softmax_rows_chunked_bwd(_code(dp.dtype), _p(prob), _p(dp), Z, N, Np, float(scale), _p(chunk[0]), int(chunk[1]), int(chunk[2]),
                                                 _stream()), "softmax_rows_chunked_bwd")
    else:
        check(lib.esvit_softmax_rows_bwd(_code(dp.dtype), _p(prob), _p(dp), Z, N, Np, float(scale), _stream()), "softmax_rows_bwd")
    _bmm(dp, qkvh[1], Np, hd, Np, b_kstrided=1, out=dqkvh[0])                  # dq = dS k
    _bmm(dp, qkvh[0], Np, hd, Np, a_kstrided=1, b_kstrided=1, out=dqkvh[1])   # dk = dS^T q
    return heads_merge(dqkvh.view(3, B, nH, Np, hd), N)


# ---- flash attention for crops of any length (csrc/flash_attn.hip): the scores stay on the chip, nothing grows with N^2 -------------
ATTN_GLOBAL = 0x20000000  # ESVIT_ATTN_GLOBAL: passed as ws, selects the global mode of esvit_window_attn_fwd / _bwd


def global_attn_supported(dtype, hd):
    """the flash route exists for this shape: bf16 (the fp32 parity mode keeps the batched-GEMM route), head_dim 32 / 64"""
    return dtype == torch.bfloat16 and hd in (32, 64)


def global_attn_fwd(qkv, B, N, nH, scale, out=None):
    """Attention.forward between the projections (vision_transformer.py:76-83) for any N in one fused kernel: qkv [B * N, 3C] ->
    (out [B * N, C], saved = (qkv, out, lse fp32 [B, nH, N])).  out: optional destination whose first B * N rows are written."""
    qkv = _actc(qkv)
    Cc = qkv.shape[1] // 3
    assert qkv.shape[0] == B * N
    if out is None:
        out = torch.empty((B * N, Cc), dtype=qkv.dtype, device=qkv.device)
    assert out.dtype == qkv.dtype and out.is_contiguous() and out.shape[0] >= B * N and out.shape[1] == Cc
    lse = torch.empty((B, nH, N), dtype=torch.float32, device=qkv.device)
    ws = workspace(query(Q_GLOBAL_ATTN_WS, B * nH, N, 0), qkv.device, slot=3)
    check(lib.esvit_window_attn_fwd(_code(qkv.dtype), _p(qkv), None, None, N, None, ATTN_GLOBAL, _p(ws), None, 1, B, N, nH, Cc // nH,
                                    float(scale), _p(out), _p(lse), None, _stream()), "window_attn_fwd(global)")
    return out, (qkv, out, lse)


def global_attn_bwd(dout, saved, B, N, nH, scale, dqkv=None):
    """gradient of global_attn_fwd with respect to qkv: dout [B * N, C] -> dqkv [B * N, 3C] (dqkv: optional destination whose first
    B * N rows are written)"""
    qkv, out, lse = saved
    dout = _actc(dout)
    Cc = qkv.shape[1] // 3
    assert dout.shape == (B * N, Cc) and out.shape[0] >= B * N and dout.dtype == qkv.dtype
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    assert dqkv.dtype == qkv.dtype and dqkv.is_contiguous() and dqkv.shape[0] >= B * N and dqkv.shape[1] == 3 * Cc
    ws = workspace(query(Q_GLOBAL_ATTN_WS, B * nH, N, 1), qkv.device, slot=3)
    check(lib.esvit_window_attn_bwd(_code(qkv.dtype), _p(qkv), None, None, N, _p(dout), _p(out), _p(lse), None, ATTN_GLOBAL, _p(ws), None,
                                    1, B, N, nH, Cc // nH, float(scale), _p(dqkv), None, None, _stream()), "window_attn_bwd(global)")
    return dqkv


# ---- attention statistics (csrc/flash_attn.hip): entropy of every softmax row and a few rows of P, without P ------------------------
ATTN_STATS = 0x08000000  # ESVIT_ATTN_STATS: OR'd into ATTN_GLOBAL, selects the statistics mode of esvit_window_attn_fwd


def global_attn_stats_supported(dtype, hd):
    """the statistics kernels exist for this shape: bf16, head_dim 32 / 64 (any number of tokens)"""
    return dtype == torch.bfloat16 and hd in (32, 64)


def _stats_queries(queries, N, device):
    """a list / range / int tensor of token indices -> int32 device tensor, every index checked against [0, N) here: the library
    cannot read the array"""
    if queries is None:
        return None
    if torch.is_tensor(queries):
        q = queries.reshape(-1)
        assert not q.dtype.is_floating_point and q.dtype != torch.bool, "queries: integer token indices"
        if q.numel():
            lo, hi = int(q.min()), int(q.max())
            if lo < 0 or hi >= N:
                raise ValueError("global_attn_stats: query indices must lie in [0, %d), got %d .. %d" % (N, lo, hi))
        return q.to(device=device, dtype=torch.int32).contiguous()
    idx = [int(i) for i in queries]
    bad = [i for i in idx if not 0 <= i < N]
    if bad:
        raise ValueError("global_attn_stats: query indices must lie in [0, %d), got %r" % (N, bad[:8]))
    return torch.tensor(idx, dtype=torch.int32, device=device)


def global_attn_stats(qkv, B, N, nH, scale, queries=None, want_lse=False):
    """what an attention analysis reads of softmax(scale q k^T), without the score tensor: qkv [B * N, 3C] ->
    (entropy fp32 [B, nH, N] in nats, rows fp32 [B, nH, nq, N] of the listed queries or None, lse fp32 [B, nH, N] or None).
    queries: a list or an integer tensor of token indices in [0, N), the same for every image and head; duplicates allowed."""
    qkv = _actc(qkv)
    Cc = qkv.shape[1] // 3
    assert qkv.shape[0] == B * N
    qidx = _stats_queries(queries, N, qkv.device)
    nq = 0 if qidx is None else qidx.numel()
    both = torch.empty((B, nH, 1 + nq, N), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, nH, N), dtype=torch.float32, device=qkv.device) if want_lse else None
    check(lib.esvit_window_attn_fwd(_code(qkv.dtype), _p(qkv), None, _p(qidx) if nq else None, N, None, ATTN_GLOBAL | ATTN_STATS, None, None,
                                    1 + nq, B, N, nH, Cc // nH, float(scale), None, _p(lse) if want_lse else None, _p(both), _stream()),
          "window_attn_fwd(global, stats)")
    return both[:, :, 0], (both[:, :, 1:] if queries is not None else None), lse


# ---- fused sliding-chunk attention (csrc/chunk_attn.hip): the scores stay on the chip, nothing grows with N^2 --------------------
ATTN_SLIDING_CHUNK = 0x40000000  # ESVIT_ATTN_SLIDING_CHUNK: OR'd into ws, selects the sliding-chunk mode of esvit_window_attn_fwd / _bwd
CHUNK_W = 7                      # the chunk side the kernels are built for (every yaml of the reference)
CHUNK_MAX_NGLO = 7


def sliding_chunk_attn_supported(dtype, hd, w, nglo):
    """the fused sliding-chunk route exists for this shape: bf16 (the fp32 parity mode keeps the dense route), head_dim 32 / 48 / 64,
    7 x 7 chunks, at most 7 global tokens"""
    return dtype == torch.bfloat16 and hd in (32, 48, 64) and w == CHUNK_W and 0 <= nglo <= CHUNK_MAX_NGLO


def _chunk_grid(chunk, N):
    """(table, nglo, tokens per chunk row[, w]) -> (table, nglo, nx, ny, w)"""
    tab, nglo, rowtok = chunk[:3]
    w = chunk[3] if len(chunk) > 3 else CHUNK_W
    assert rowtok > 0 and rowtok % w == 0, "sliding-chunk attention needs the (table, nglo, tokens per chunk row) form"
    ny = rowtok // w
    nx = (N - nglo) // ny
    assert nglo + nx * ny == N and tab.dtype == torch.int32 and tab.numel() == N and tab.is_contiguous()
    return tab, int(nglo), nx, ny, int(w)


def sliding_chunk_attn_fwd(qkv, B, N, nH, scale, chunk, out=None):
    """Vision Longformer's sliding-chunk attention in one set of fused kernels: qkv [B * N, 3C] (tokens [globals | (x, y) row-major])
    -> (out [B * N, C], saved = (qkv, out, lse fp32 [B, nH, N])).  chunk = (table, nglo, tokens per chunk row) as MsViT._stage builds it.
    out: optional destination whose first B * N rows are written."""
    qkv = _actc(qkv)
    tab, nglo, nx, ny, w = _chunk_grid(chunk, N)
    Cc = qkv.shape[1] // 3
    assert qkv.shape[0] == B * N
    if out is None:
        out = torch.empty((B * N, Cc), dtype=qkv.dtype, device=qkv.device)
    assert out.dtype == qkv.dtype and out.is_contiguous() and out.shape[0] >= B * N and out.shape[1] == Cc
    lse = torch.empty((B, nH, N), dtype=torch.float32, device=qkv.device)
    ws = workspace(query(Q_CHUNK_ATTN_WS, B * nH, N, 0), qkv.device, slot=3)
    check(lib.esvit_window_attn_fwd(_code(qkv.dtype), _p(qkv), None, _p(tab), N, None, w | ATTN_SLIDING_CHUNK, _p(ws), None, nx, B, ny, nH, Cc // nH,
                                    float(scale), _p(out), _p(lse), None, _stream()), "window_attn_fwd(sliding chunk)")
    return out, (qkv, out, lse)


def sliding_chunk_attn_bwd(dout, saved, B, N, nH, scale, chunk, dqkv=None):
    """gradient of sliding_chunk_attn_fwd with respect to qkv: dout [B * N, C] -> dqkv [B * N, 3C] (dqkv: optional destination whose
    first B * N rows are written)"""
    qkv, out, lse = saved
    dout = _actc(dout)
    tab, nglo, nx, ny, w = _chunk_grid(chunk, N)
    Cc = qkv.shape[1] // 3
    assert dout.shape == (B * N, Cc) and out.shape[0] >= B * N and dout.dtype == qkv.dtype
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    assert dqkv.dtype == qkv.dtype and dqkv.is_contiguous() and dqkv.shape[0] >= B * N and dqkv.shape[1] == 3 * Cc
    ws = workspace(query(Q_CHUNK_ATTN_WS, B * nH, N, 1), qkv.device, slot=3)
    check(lib.esvit_window_attn_bwd(_code(qkv.dtype), _p(qkv), None, _p(tab), N, _p(dout), _p(out), _p(lse), None, w | ATTN_SLIDING_CHUNK, _p(ws), None,
                                    nx, B, ny, nH, Cc // nH, float(scale), _p(dqkv), None, None, _stream()), "window_attn_bwd(sliding chunk)")
    return dqkv


# ---- statistics of the sliding-chunk softmax (csrc/chunk_attn.hip): entropy of every row and a few rows of P, without P ------------
ATTN_CHUNK_STATS = 0x02000000  # ESVIT_ATTN_CHUNK_STATS: OR'd into ws | ATTN_SLIDING_CHUNK, selects the statistics mode of esvit_window_attn_fwd


def chunk_attn_stats_supported(dtype, hd, w, nglo):
    """the statistics kernels exist for this shape: every shape the fused sliding-chunk forward has"""
    return sliding_chunk_attn_supported(dtype, hd, w, nglo)


def chunk_attn_stats(qkv, B, N, nH, scale, chunk, queries=None, ent_out=None, rows_out=None):
    """what an attention analysis reads of the softmax sliding_chunk_attn_fwd computes, without a score tensor: qkv [B * N, 3C] (tokens
    [globals | (x, y) row-major]) -> (entropy fp32 [B, nH, N] in nats with 0 log 0 = 0, every row over the keys it sees; rows fp32
    [B, nH, nq, N] or None: the probability row of every listed query over all N tokens, exactly 0 where the query does not see).
    chunk = (table, nglo, tokens per chunk row[, w]) as MsViT._stage builds it.  queries: a list or an integer tensor of token indices
    in [0, N), the same for every image and head; duplicates allowed.  ent_out / rows_out: optional contiguous fp32 destinations of
    those shapes."""
    qkv = _actc(qkv)
    tab, nglo, nx, ny, w = _chunk_grid(chunk, N)
    Cc = qkv.shape[1] // 3
    assert qkv.shape[0] == B * N
    if ny >= 1 << 16:
        raise ValueError("chunk_attn_stats: at most %d grid columns, got %d" % ((1 << 16) - 1, ny))
    try:
        qidx = _stats_queries(queries, N, qkv.device)
    except ValueError as e:
        raise ValueError(str(e).replace("global_attn_stats", "chunk_attn_stats")) from None
    nq = 0 if qidx is None else qidx.numel()
    if nq >= 1 << 15:
        raise ValueError("chunk_attn_stats: at most %d listed queries, got %d" % ((1 << 15) - 1, nq))
    ent = torch.empty((B, nH, N), dtype=torch.float32, device=qkv.device) if ent_out is None else ent_out
    rows = None
    if queries is not None:
        rows = torch.empty((B, nH, nq, N), dtype=torch.float32, device=qkv.device) if rows_out is None else rows_out
    for t, shape in ((ent, (B, nH, N)), (rows, (B, nH, nq, N))):
        assert t is None or (t.shape == shape and t.dtype == torch.float32 and t.is_contiguous()), (shape, t.shape)
    ws = workspace(query(Q_CHUNK_ATTN_WS, B * nH, N, 0), qkv.device, slot=3)
    check(lib.esvit_window_attn_fwd(_code(qkv.dtype), _p(qkv), None, _p(tab), N, None, w | ATTN_SLIDING_CHUNK | ATTN_CHUNK_STATS, _p(ws), None, nx, B,
                                    ny | (nq << 16), nH, Cc // nH, float(scale), _p(qidx) if nq else None, _p(rows) if nq else None, _p(ent), _stream()),
          "window_attn_fwd(sliding chunk stats)")
    return ent, rows
