"""Autograd glue: each Function composes the C-ABI kernels (esvit_amd.ops) for one stage of the hot
path and carries the hand-derived backward.  No torch compute op is used on
the data path -- torch provides allocation, streams and the autograd graph only.

Stages (reference lines):
  SwinBlockFn      swin_transformer.py:275-333 (+120-152): LN -> pad/roll/partition -> qkv -> window
                   attention -> proj -> reverse/unroll/crop + residual -> LN -> MLP + residual
  SwinBlockMultiFn the same over the token rows of several resolution groups (swin_transformer.py:729-751)
  PatchEmbedFn, PatchEmbedMultiFn   swin_transformer.py:537-547
  PatchMergeFn, PatchMergeMultiFn   swin_transformer.py:393-420
  FinalNormFn      swin_transformer.py:687
  TokenMeanFn      swin_transformer.py:688-689
  DinoHeadFn       vision_transformer.py:384-418 without BatchNorm, any number of Linear layers
  DinoHeadBnFn     vision_transformer.py:391-402, 414-418 (use_bn), any number of BatchNorm layers
  ConvEmbedFn, CvtAttnFn, CvtFfnFn   cvt_v4_transformer.py:349-382, 108-220 (+75-105), 62-72  (BASELINE config 5)
  ConvEmbedMultiFn, CvtAttnMultiFn, CvtFfnMultiFn   the same over the token rows of several resolution groups (cvt_v4_transformer.py:625-628)
  VitPatchEmbedFn  vision_transformer.py:121-139
  VitBodyFn        one block body on token rows behind vit_block (vision_transformer.py:96-116), vit_block_multi (186-233: the rows of
                   several resolution groups) and vil_block (vision_longformer.py:36-118, layers/longformer2d.py)

Shared by the block families: the unfused MLP branch (_mlp_fwd / _mlp_bwd: LayerNorm -> fc1 + GELU -> fc2 + residual, called by the Swin,
ViT and Vision Longformer blocks and CvT's feed-forward), Swin's choice between the fused, the wide and the unfused MLP kernels
(_swin_mlp_fwd) and the fused backwards (_mlp_branch_bwd, _attn_branch_bwd).  A forward names the route it took (ctx.mlp_route,
ctx.attn_bwd_fused, the attention route of every segment of a ViT-family block: vit_attention's _att_saved) and saves its tensors by
name (_save_named); a backward reads both back and infers nothing from what was saved.
The weight gradients of the blocks and of DinoHeadFn are leaves launched through _side_run into their bucket slots (_wgrad, _ln_sinks),
and such a node joins (_side_join) before it returns.
"""
import math
import os
import types

import torch

from . import ops
from . import params as P
from .determinism import is_deterministic

LN_EPS = 1e-6


def ops_module():
    return ops


# PatchMerging on an odd feature map (swin_transformer.py:406-408): "copy" pads the token grid with a pass of its own (PadTokensFn) and
# keeps such crops off the ragged multi-crop route; "kernel" lets the merge kernel read the missing row / column as zeros
# (ops.merge_ln_fwd(pad=True), ESVIT_MERGE_PAD of include/esvit_hip.h) on both routes.  Neither setting has been timed: the default is
# what the code did before the switch existed.  Environment: ESVIT_MERGE_PAD=copy|kernel; anything else raises.
_MERGE_PAD_MODES = ("copy", "kernel")
MERGE_PAD = os.environ.get("ESVIT_MERGE_PAD", "copy")
if MERGE_PAD not in _MERGE_PAD_MODES:
    raise ValueError("ESVIT_MERGE_PAD: copy or kernel, not %r" % MERGE_PAD)


def merge_pad_in_kernel():
    """True: odd feature maps are padded inside the merge kernel (MERGE_PAD == "kernel" and an ops module that offers the mode -- the
    CPU restatement of the kernels does not and keeps the copy route)"""
    if MERGE_PAD not in _MERGE_PAD_MODES:
        raise ValueError("functional.MERGE_PAD: copy or kernel, not %r" % (MERGE_PAD,))
    return MERGE_PAD == "kernel" and bool(getattr(ops_module(), "MERGE_LN_PAD", False))


def merged_grid(H, W):
    """grid after one PatchMerging: odd sides are padded up first (swin_transformer.py:406-408)"""
    return (H + 1) // 2, (W + 1) // 2


def _no_dbias(o, N, hd):
    """keyword of o.window_attn_bwd for a caller WITHOUT a relative-position table: on windows of more than 64 tokens at head_dim 64 the
    bias gradient is a kernel of its own (window_attn_big.hip), which such a caller leaves out.  Passed only where it changes something
    and to an ops module that knows it (the CPU restatement of the kernels computes the slabs in passing and has no such switch)"""
    return {"want_dbias": False} if N > 64 and hd == 64 and getattr(o, "ATTN_BWD_OPTIONAL_DBIAS", False) else {}


def _relpos_kw(o):
    """keyword of o.relpos_bias_bwd in the deterministic mode (esvit_amd.set_deterministic): the fixed-order table gradient without
    atomics.  Passed only when the mode is on and to an ops module that knows it (the CPU restatement is deterministic anyway)"""
    return {"ordered": True} if is_deterministic() and getattr(o, "RELPOS_BWD_ORDERED", False) else {}


# ------------------------------------------------------------------------------------------------
# static per-geometry tables (index maps, shift masks), cached per device
# ------------------------------------------------------------------------------------------------
_GEOM = {}


class WindowGeometry:
    """Everything that depends only on (H, W, window, shift): the bit-exact slot<->token maps and the
    shift mask in the attention kernel's fragment layout."""

    def __init__(self, H, W, ws, shift, device):
        o = ops_module()
        win2tok, tok2win = o.window_maps(H, W, ws, shift)
        self.H, self.W, self.ws, self.shift = H, W, ws, shift
        self.N = ws * ws
        self.period = int(win2tok.size)           # window slots per image
        self.nW = self.period // self.N
        self.tokens = H * W
        self.win2tok = torch.from_numpy(win2tok).to(device)
        self.tok2win = torch.from_numpy(tok2win).to(device)
        self.region_ids = None
        if shift > 0:
            self.region_ids = torch.from_numpy(o.shift_region_ids(H, W, ws, shift)).to(device)


def geometry(H, W, ws, shift, device):
    key = (H, W, ws, shift, str(device), id(ops_module()))
    g = _GEOM.get(key)
    if g is None:
        g = WindowGeometry(H, W, ws, shift, device)
        _GEOM[key] = g
    return g


def _alias(t, sink):
    """a gradient that was written into a bucket slot goes to autograd as a FRESH alias of the slot (AccumulateGrad only adopts
    a tensor nobody else holds; it would clone the stored view)"""
    return t.detach() if sink is not None else t


def _wgrad(dy, x, param, shape2d=None, want_bias=False, bias_param=None):
    """weight (and bias) gradient of `param` = dy^T x; written straight into the data-parallel reducer's bucket slots when
    they are armed (params.grad_out), and handed to autograd as fresh aliases so that AccumulateGrad adopts them without a copy"""
    o = ops_module()
    sink = P.grad_out(param, shape2d)
    if not want_bias:
        return _alias(o.linear_wgrad(dy, x, out=sink), sink)
    sink_b = P.grad_out(bias_param) if bias_param is not None else None
    dw, db = o.linear_wgrad(dy, x, out=sink, want_bias=True, db_out=sink_b)
    return _alias(dw, sink), _alias(db, sink_b)



# ---- weight gradients on a second stream -------------------------------------------------------------------------------------------
# The weight-gradient GEMMs are leaves of the backward's dependency chain: nothing downstream in the same node reads them.  A Swin
# block's / head's / PatchMerging's backward launches them on a side stream behind an event and joins before it returns --
# every gradient is complete on the autograd stream when the node hands it over -- so that they share the CUs with the dgrad /
# LayerNorm / attention kernels of the chain (same-box A-B, profiles/r06_wgrad_stream_ab.txt: 48.47 -> 47.96 ms per step).  The stream has
# the default priority: a high-priority one measured 0.09 ms better alone and 10 ms WORSE beside RCCL's stream (ibid.).
# ESVIT_WGRAD_STREAM=0 puts them back in line.
WGRAD_STREAM = os.environ.get("ESVIT_WGRAD_STREAM", "1") != "0"
_wg_state = {}


def _side_run(fn, *keep):
    """fn() launches kernels whose inputs are ready on the current stream; `keep`: the tensors they read (held until _side_join, so
    that the caching allocator cannot hand their memory to the autograd stream while the side stream still reads it)"""
    if not (WGRAD_STREAM and keep[0].is_cuda):
        return fn()
    dev = keep[0].device.index
    st = _wg_state.get(dev)
    if st is None:
        st = _wg_state[dev] = {"stream": torch.cuda.Stream(device=dev, priority=int(os.environ.get("ESVIT_WGRAD_PRIO", "0"))), "keep": [],
                               "pending": False, "event": torch.cuda.Event()}
    ev = st["event"]  # one event per device, re-recorded: a wait refers to the record that precedes it in program order
    ev.record(torch.cuda.current_stream(dev))
    st["stream"].wait_event(ev)
    with torch.cuda.stream(st["stream"]):
        out = fn()
    st["keep"].append(keep)
    st["pending"] = True
    return out


_DEFER_PROBE = os.environ.get("ESVIT_PROBE_WGRAD_DEFER", "0") == "1"  # timing probe only (UNSAFE: gradients may be read before they are complete)


def _side_join(final=False):
    if _DEFER_PROBE and not final:
        return
    for dev, st in _wg_state.items():
        if st["pending"]:
            torch.cuda.current_stream(dev).wait_stream(st["stream"])
            st["keep"].clear()
            st["pending"] = False


def _ln_sinks(gparam, bparam):
    """bucket slots of a LayerNorm's (weight, bias) gradients, or None when no reducer is armed / either has none"""
    sg, sb = P.grad_out(gparam), P.grad_out(bparam)
    return (sg, sb) if sg is not None and sb is not None else None


def _weight(p, shape2d=None):
    """activation-dtype copy of an fp32 parameter; frozen parameters (the EMA teacher) are recast on every
    use because in-place `.data` updates (main_esvit.py:590) are invisible to version counters."""
    if p.requires_grad or P.is_managed(p):
        return P.cached_cast(p, shape2d)
    src = p.detach() if shape2d is None else p.detach().reshape(shape2d)
    return ops_module().cast_to_act(src.contiguous())


def _mlp_w(p, kind):
    """the copy of fc1.weight / fc2.weight the fused MLP kernels stream (ops.mlp_fused_weight), cached per parameter version like
    the plain cast; frozen parameters that nobody manages (a teacher outside the fused updater) are converted on every use"""
    o = ops_module()
    fn = lambda: o.mlp_fused_weight(getattr(o, kind), p.detach().contiguous())  # noqa: E731
    if p.requires_grad or P.is_managed(p):
        return P.cached(p, kind, fn)
    return fn()


def _perm_w(p):
    """the copy of qkv.weight / proj.weight the fused attention branch streams (ops.cast_weight, perm32), cached like _mlp_w"""
    o = ops_module()
    fn = lambda: o.cast_weight(p.detach().contiguous(), perm32=True)  # noqa: E731
    if p.requires_grad or P.is_managed(p):
        return P.cached(p, "ATTN_PERM32", fn)
    return fn()


# ---- fused attention branch (narrow stages, bf16): LayerNorm -> qkv -> 7x7 window attention -> proj -> residual in one kernel per
# resolution group (esvit_attn_branch_fwd).  Inference passes (the EMA teacher) write nothing but the branch output; a training
# pass also gets the tensors its (unfused) backward reads as side outputs of the same kernel.
ATTN_FUSED = os.environ.get("ESVIT_ATTN_FUSED", "1") != "0"  # (A-B runs switch back to the four-kernel sequence)


def _attn_fused(dt, C, nH, geoms, save, sizes=None):
    """save: a training pass (side outputs on).  Measured on the MI355X (tools/bench_attn_branch.py, B = 128 row counts): without
    side outputs the kernel beats the four-kernel sequence at both widths (C = 96: 226 vs 610 us on the 224-crop rows; C = 192:
    226 vs 299); WITH the 10 B per token-channel of side outputs it still wins at C = 96 (387 + 309 vs ~900 us per block over both
    groups) and loses at C = 192 (292 + 283 vs ~470), so a training pass takes it at C = 96 only"""
    rows, wins = (max(r for r, _ in sizes), max(w for _, w in sizes)) if sizes else (0, 0)  # (token rows, windows) of the largest call
    if not (ATTN_FUSED and all(g.ws == 7 for g in geoms) and ops_module().attn_branch_supported(dt, C, nH, max(g.N for g in geoms), rows, wins)):
        return False
    return C == 96 or not save


# stage 0 (bf16, C = 96, 7x7 windows): the branch's BACKWARD as one kernel per resolution group too (the backward mode of
# esvit_attn_branch_fwd): it recomputes the forward per window and keeps dWqkv, dWproj and the small gradients on the chip, so the forward
# writes no side outputs and the chain from the proj weight gradient to the LayerNorm backward disappears.  Opt-in ("1") until its A-B is
# won (profiles/attn_bwd_fused_ab.txt); the decision is taken in the forward (it decides what is saved) and read back from what was saved.
ATTN_BWD_FUSED = os.environ.get("ESVIT_ATTN_BWD_FUSED", "0") == "1"


def _attn_bwd_fused(o, dt, C, nH, geoms, sizes):
    """sizes: (token rows, windows) of every call"""
    return (ATTN_BWD_FUSED and hasattr(o, "attn_branch_bwd") and all(g.ws == 7 for g in geoms)
            and all(o.attn_branch_bwd_supported(dt, C, nH, g.N, r, w) for g, (r, w) in zip(geoms, sizes)))


# stage 0 (bf16, C = 96): what follows the window-attention backward has no window structure -- qkv data gradient, qkv weight gradient
# (on the side stream) and norm1's backward, 32 B per token-channel in four launches.  ops.attn_tail_bwd is the three in one pass over
# the rows (18 - 20 B), with LayerNorm(x) recomputed from the saved statistics.  "0": A-B runs.
ATTN_TAIL_FUSED = os.environ.get("ESVIT_ATTN_TAIL_FUSED", "1") != "0"


def _attn_tail_fused(o, dt, C):
    return ATTN_TAIL_FUSED and hasattr(o, "attn_tail_bwd") and o.attn_tail_bwd_supported(dt, C)


def _attn_tail_bwd(o, dqkv, X, mean1, rstd1, g1, Wqkv, gx1, pads, params, rowscale, rows_per_sample, want_act):
    """-> (gx, gx act copy or None, dg1, db1, dWqkv, dbqkv), the gradients in their bucket slots; pads: the window-attention backward's
    zero-pad slabs, whose column sums are the rest of the k / v bias gradient; params: (norm1.weight, norm1.bias, qkv.weight, qkv.bias)"""
    g1_p, b1_p, Wqkv_p, bqkv_p = params
    C = X.shape[1]
    wsink, bsink, ln1 = P.grad_out(Wqkv_p), P.grad_out(bqkv_p), _ln_sinks(g1_p, b1_p)
    gx, gxb, dWqkv, dbqkv, dg1, db1 = o.attn_tail_bwd(dqkv, X, mean1, rstd1, g1, b1_p.detach(), Wqkv, gx1, rowscale=rowscale if want_act else None,
                                                      rows_per_sample=rows_per_sample, want_act=want_act, out=wsink, db_out=bsink, gb_out=ln1)
    for dpad_ws in pads:
        o.colsum(dpad_ws, out=dbqkv[C:], accumulate=True)  # k/v bias gradient from the zero-pad slots (behind the reduce, same stream)
    return gx, gxb, _alias(dg1, ln1), _alias(db1, ln1), _alias(dWqkv, wsink), _alias(dbqkv, bsink)


def _attn_bwd_w(o, Wqkv_p, Wproj_p, Wqkv):
    """the bf16 copies the backward mode reads: the plain cast of qkv.weight (the copy every GEMM uses), its transpose and the transpose of
    proj.weight (ops.cast_weight), cached per parameter version like _perm_w"""
    def one(p_, kind):
        fn = lambda: o.cast_weight(p_.detach().contiguous(), transpose=True)  # noqa: E731
        return P.cached(p_, kind, fn) if (p_.requires_grad or P.is_managed(p_)) else fn()
    return Wqkv, one(Wqkv_p, "ATTN_BWD_QKVT"), one(Wproj_p, "ATTN_BWD_PROJT")


def _attn_branch_bwd(o, X, gx1, segs, nH, frags, index, table, Wqkv, params, g1, b1, bqkv, dp1, prev_scale, want_act):
    """the attention branch's backward, one launch per resolution group: X, gx1 fp32 [M, C] (branch input, dL/dx1); segs: (row0, nB, L,
    geom); frags: the groups' filled fragment-order bias; params: (g1, b1, table, Wqkv, bqkv, Wproj, bproj) parameters; dp1: per-row
    DropPath factors of the branch or None -> (gx, gx_act or None, dg1, db1, dtable, dWqkv, dbqkv, dWproj, dbproj).  The groups stack their
    partials and bias-gradient slabs: the last call's reduce goes straight into the armed bucket slots, the table's included"""
    g1_p, b1_p, table_p, Wqkv_p, bqkv_p, Wproj_p, bproj_p = params
    M, C = X.shape
    scale = (C // nH) ** -0.5
    sinks = [P.grad_out(p_) for p_ in (Wqkv_p, bqkv_p, Wproj_p, bproj_p, g1_p, b1_p)]
    tsink = P.grad_out(table_p)
    weights = _attn_bwd_w(o, Wqkv_p, Wproj_p, Wqkv)
    part, dbias, firsts = o.attn_branch_bwd_workspaces([nB * geom.nW for (_, nB, _, geom) in segs], nH, X.device)
    gx = torch.empty_like(X)
    gxb = torch.empty((M, C), dtype=Wqkv.dtype, device=X.device) if want_act else None
    outs = dtable = None
    for i, ((r0, nB, L, geom), frag) in enumerate(zip(segs, frags)):
        r1 = r0 + nB * L
        _, _, outs, _, dtable = o.attn_branch_bwd(X[r0:r1], gx1[r0:r1], g1, b1, LN_EPS, weights, bqkv, geom.win2tok, L, geom.ws, geom.region_ids, geom.nW, geom.N, nH,
                                          scale, bias_frag=frag, rowscale=None if dp1 is None else dp1[r0:r1],
                                          rowscale_out=None if (prev_scale is None or not want_act) else prev_scale[r0:r1], out=sinks if outs is None else outs,
                                          workspaces=(part, dbias), first_partial=firsts[i], finish=i == len(segs) - 1, gx_out=gx[r0:r1],
                                          gx_act_out=None if gxb is None else gxb[r0:r1], index=index, dtable=tsink, table_rows=table.shape[0])
    dWqkv, dbqkv, dWproj, dbproj, dg1, db1 = [_alias(t, sk) for t, sk in zip(outs, sinks)]
    return gx, gxb, dg1, db1, _alias(dtable, tsink), dWqkv, dbqkv, dWproj, dbproj


# ---- fused MLP branch (narrow stages, bf16): nothing hidden-sized is kept between forward and backward ------------------------
# forward: ONE kernel x1 -> x2 (esvit_mlp_fused_fwd).  backward: esvit_mlp_fused_bwd recomputes LayerNorm + pre-activation,
# produces dL/dx1 (+ its activation-dtype copy) and the operands of the two weight-gradient GEMMs; the LayerNorm parameter
# gradients fall out of the fc1 weight gradient (esvit_ln_fold_finish).
MLP_FUSED_TRAIN = os.environ.get("ESVIT_MLP_FUSED_TRAIN", "1") != "0"  # (A-B runs switch the training path back to the unfused sequence)


# the C = 384 branch: "0" the LayerNorm + two-GEMM sequence everywhere, "1" the fused kernel in inference passes (the EMA teacher), "2" also
# in the training pass (esvit_mlp_fused_fwd_train)
_WIDE = os.environ.get("ESVIT_MLP_WIDE_FUSED", "1")
MLP_WIDE_FUSED = _WIDE != "0"
MLP_WIDE_TRAIN = _WIDE == "2"


def _mlp_wide_train(W1, C, rows):
    """the wide stage's training pass: forward fused (esvit_mlp_fused_fwd_train writes the operands of the unfused backward)"""
    return MLP_WIDE_TRAIN and ops_module().mlp_fused_train_supported(W1.dtype, C, rows)


def _mlp_fused_infer(W1, C):
    return ops_module().mlp_fused_supported(W1.dtype, C) and (MLP_WIDE_FUSED or C != 384)


def _mlp_fused_train(W1, C):
    return MLP_FUSED_TRAIN and ops_module().mlp_fused_supported(W1.dtype, C, backward=True)


# stage 0 (bf16, C = 96): the same kernel also accumulates dW2, db2, G and db1 on the chip, so GELU(A), dA and xhat are never written
# and the two weight-gradient GEMMs with their split-K reduces disappear (esvit_mlp_fused_bwd's trailing arguments).  "0": A-B runs.
MLP_DW_ONCHIP = os.environ.get("ESVIT_MLP_DW_ONCHIP", "1") != "0"


def _mlp_dw_onchip(o, W1, C):
    return MLP_DW_ONCHIP and hasattr(o, "mlp_fused_bwd_dw") and o.mlp_fused_dw_supported(W1.dtype, C)


def _mlp_branch_bwd(o, x1, gy, dyb, g2, b2, W1, bfc1, params, dp_mlp, dp_out):
    """-> (gx1 fp32, gx1 act copy (scaled by dp_out), dg2, db2, dW1, dbfc1, dW2, dbfc2); dyb: cast(dp_mlp * gy) [M, C] act"""
    g2_p, b2_p, W1_p, bfc1_p, W2_p, bfc2_p = params
    if _mlp_dw_onchip(o, W1, x1.shape[1]):
        ln2 = _ln_sinks(g2_p, b2_p)
        wsink, bsink = P.grad_out(W1_p), P.grad_out(bfc1_p)
        w2sink, b2sink = P.grad_out(W2_p), P.grad_out(bfc2_p)
        gx1, dyw, dW2, dbfc2, G, dbfc1 = o.mlp_fused_bwd_dw(x1, gy, g2, b2, LN_EPS, _mlp_w(W1_p, "MLP_W1_BWD"), _mlp_w(W2_p, "MLP_W2T_BWD"),
                                                            _mlp_w(W1_p, "MLP_W1T_BWD"), bfc1, rowscale_mlp=dp_mlp, rowscale_out=dp_out,
                                                            out=(w2sink, wsink), db_out=(b2sink, bsink))
        # the fold is a leaf of the chain like the GEMMs it used to follow: same side stream, same join
        dW1, dg2, db2 = _side_run(lambda: o.ln_fold_finish(G, dbfc1, W1_p.detach(), g2, b2, gb_out=ln2), G, dbfc1)
        return gx1, dyw, _alias(dg2, ln2), _alias(db2, ln2), _alias(dW1, wsink), _alias(dbfc1, bsink), _alias(dW2, w2sink), _alias(dbfc2, b2sink)
    gx1, dyw, xhat, a1g, da1 = o.mlp_fused_bwd(x1, gy, g2, b2, LN_EPS, _mlp_w(W1_p, "MLP_W1_BWD"), _mlp_w(W2_p, "MLP_W2T_BWD"), _mlp_w(W1_p, "MLP_W1T_BWD"), bfc1,
                                               rowscale_mlp=dp_mlp, rowscale_out=dp_out)
    ln2 = _ln_sinks(g2_p, b2_p)
    wsink, bsink = P.grad_out(W1_p), P.grad_out(bfc1_p)

    def wgrads():
        dW2, dbfc2 = _wgrad(dyb, a1g, W2_p, want_bias=True, bias_param=bfc2_p)
        G, dbfc1 = o.linear_wgrad(da1, xhat, out=wsink, want_bias=True, db_out=bsink)  # G = dA^T xhat: LayerNorm folded out
        dW1, dg2, db2 = o.ln_fold_finish(G, dbfc1, W1_p.detach(), g2, b2, gb_out=ln2)
        return dW2, dbfc2, dbfc1, dW1, dg2, db2

    dW2, dbfc2, dbfc1, dW1, dg2, db2 = _side_run(wgrads, dyb, a1g, da1, xhat)
    del a1g, da1, xhat
    return gx1, dyw, _alias(dg2, ln2), _alias(db2, ln2), _alias(dW1, wsink), _alias(dbfc1, bsink), dW2, dbfc2


# ---- the unfused MLP branch: LayerNorm -> fc1 + GELU -> fc2 + residual.  Row-wise, so the Swin, ViT and Vision Longformer blocks and
# CvT's feed-forward all run these two bodies, per resolution group or over the rows of all groups alike ---------------------------------
_MLP_SAVED = ("mean2", "rstd2", "h", "a1", "a1g")


def _mlp_fwd(o, x1, prm, W1, W2, eps, rowscale, rows_per_sample, save, quick=False):
    """x1 fp32 [M, C]; prm: (norm.weight, norm.bias, fc1.bias, fc2.bias); W1, W2: activation-dtype weights; quick: CvT's QuickGELU;
    rowscale: None or the DropPath factors, one per `rows_per_sample` rows -> (x2 fp32, (mean2, rstd2, h, a1, a1g) when saving)"""
    g2, b2, bfc1, bfc2 = prm
    h, _, mean2, rstd2 = o.layernorm_fwd(x1, g2, b2, eps)
    if save:
        a1g, a1 = o.linear_fwd(h, W1, bfc1, gelu=True, want_preact=True, quick=quick)
    else:  # (inference keeps nothing: the LayerNorm output goes before fc2 allocates)
        a1g, a1, h = o.linear_fwd(h, W1, bfc1, gelu=True, quick=quick), None, None
    x2 = o.linear_fwd(a1g, W2, bfc2, residual=x1, rowscale=rowscale, rows_per_sample=rows_per_sample, out_f32=True)
    return x2, ((mean2, rstd2, h, a1, a1g) if save else None)


def _mlp_bwd(o, dyb, h, a1, a1g, W1, W2, params, quick=False, shapes2d=(None, None)):
    """dyb: cast(DropPath * dL/dx2) [M, C]; params: (fc1.weight, fc1.bias, fc2.weight, fc2.bias) parameters; shapes2d: the matrix
    shapes of CvT's 1x1-conv weights -> (dh, dW1, dbfc1, dW2, dbfc2); the caller's LayerNorm backward takes dh.  The two weight-gradient
    GEMMs are leaves of the chain: side stream, bucket slots, and the CALLER joins (_side_join) before its node returns"""
    W1_p, bfc1_p, W2_p, bfc2_p = params
    dW2, dbfc2 = _side_run(lambda: _wgrad(dyb, a1g, W2_p, shapes2d[1], want_bias=True, bias_param=bfc2_p), dyb, a1g)
    da1 = o.linear_dgrad(dyb, W2, gelu_preact=a1, quick=quick)
    dW1, dbfc1 = _side_run(lambda: _wgrad(da1, h, W1_p, shapes2d[0], want_bias=True, bias_param=bfc1_p), da1, h)
    dh = o.linear_dgrad(da1, W1)
    return dh, dW1, dbfc1, dW2, dbfc2


def _per_row(rowscale, rows_per_sample):
    """(the fused MLP kernels take per-row DropPath factors)"""
    return rowscale if rowscale is None or rows_per_sample == 1 else rowscale.repeat_interleave(rows_per_sample)


def _swin_mlp_fwd(o, x1, prm, W1, W2, w1p, rowscale, rows_per_sample, save, next_norm=None):
    """the MLP branch of a Swin block on x1 fp32 [M, C] -> (x2, route, what the backward of that route reads or None, the next block's
    `pre` or None).  Routes:
      "fused"  narrow stage: LayerNorm -> fc1 + GELU -> fc2 + residual in one kernel, the hidden activation never reaches HBM (the
               training pass keeps x1 only: the backward recomputes).  Wide stage (C = 384), inference pass: the same, without the next
               LayerNorm.  next_norm: (weight, bias) of the NEXT block's norm1 -- the kernel then also emits that block's `pre`
      "wide"   wide stage, training pass: one kernel writes x2 and what the unfused backward reads (LayerNorm output and statistics,
               pre-activation, GELU) in place of the LayerNorm launch and the two GEMM launches
      "plain"  the unfused sequence (_mlp_fwd)"""
    g2, b2, bfc1, bfc2 = prm
    M, C = x1.shape
    if (not save and _mlp_fused_infer(W1, C)) or (save and _mlp_fused_train(W1, C)):
        rs = _per_row(rowscale, rows_per_sample)
        w1k = W1 if C == 384 else _mlp_w(w1p, "MLP_W1_FWD")
        if next_norm is not None and C != 384:
            x2, nxt = o.mlp_fused_fwd(x1, g2, b2, LN_EPS, w1k, bfc1, W2, bfc2, rowscale=rs, next_norm=(next_norm[0].detach(), next_norm[1].detach()))
            return x2, "fused", None, nxt
        return o.mlp_fused_fwd(x1, g2, b2, LN_EPS, w1k, bfc1, W2, bfc2, rowscale=rs), "fused", None, None
    if save and _mlp_wide_train(W1, C, M):
        x2, a1, a1g, h, mean2, rstd2 = o.mlp_fused_fwd_train(x1, g2, b2, LN_EPS, W1, bfc1, W2, bfc2, rowscale=_per_row(rowscale, rows_per_sample))
        return x2, "wide", (mean2, rstd2, h, a1, a1g), None
    x2, saved = _mlp_fwd(o, x1, prm, W1, W2, LN_EPS, rowscale, rows_per_sample, save)
    return x2, "plain", saved, None


# ---- what a forward keeps for its backward goes by name: the routes of a block save different sets, and a backward that counted
# positions would read another route's tensor the day one of them saves one more ----------------------------------------------------
def _save_named(ctx, **named):
    """ctx.save_for_backward of tensors (None allowed) and tuples of tensors under their names"""
    flat, at = [], {}
    for name, v in named.items():
        if isinstance(v, (tuple, list)):
            at[name] = (len(flat), len(flat) + len(v))
            flat.extend(v)
        else:
            at[name] = len(flat)
            flat.append(v)
    ctx.saved_at = at
    ctx.save_for_backward(*flat)


def _load_named(ctx):
    """-> namespace of what _save_named kept"""
    t = ctx.saved_tensors
    return types.SimpleNamespace(**{name: (tuple(t[at[0]:at[1]]) if isinstance(at, tuple) else t[at]) for name, at in ctx.saved_at.items()})


# ------------------------------------------------------------------------------------------------
# Swin block
# ------------------------------------------------------------------------------------------------
def _block_forward(x, geom, nH, index, dp, prm, wts, save, w1p=None, wattn=None):
    """x fp32 [nB, L, C].  prm: fp32 parameters; wts: activation-dtype weight copies.
    dp: None or (scale_attn [nB], scale_mlp [nB]) DropPath factors.
    -> (y, None), or when saving (y, (is the attention backward the one-kernel mode, MLP route, tensors for the backward by name))"""
    o = ops_module()
    (g1, b1, table, bqkv, bproj, g2, b2, bfc1, bfc2) = prm
    (Wqkv, Wproj, W1, W2) = wts
    nB, L, C = x.shape
    x2d = x.view(nB * L, C)
    scale = (C // nH) ** -0.5
    dp1, dp2 = (None, None) if dp is None else dp
    # everything stays in token order: the attention kernel applies pad/roll/partition through geom.win2tok and
    # injects the qkv bias at zero-pad slots, so no GEMM ever runs on pad rows
    frag = o.new_bias_frag(nH, geom.N, x.device) if save else None  # kept for the backward (no second fill)
    bwd_fused = False
    if wattn is not None and _attn_fused(Wqkv.dtype, C, nH, (geom,), save, [(nB * L, nB * geom.nW)]):
        rs1 = None if dp1 is None else dp1.repeat_interleave(L)
        # (a training pass whose backward is the one-kernel mode needs no side outputs)
        bwd_fused = bool(save) and _attn_bwd_fused(o, Wqkv.dtype, C, nH, (geom,), [(nB * L, nB * geom.nW)])
        side = bool(save) and not bwd_fused
        res = o.attn_branch_fwd(x2d, g1, b1, LN_EPS, _perm_w(wattn[0]), bqkv, _perm_w(wattn[1]), bproj, geom.win2tok, L, table, geom.ws, geom.region_ids,
                                geom.nW, geom.N, nH, scale, rowscale=rs1, bias_frag=frag, save=side)
        lse = None
        if side:
            x1, (xw, mean1, rstd1, qkv, ao) = res
        else:
            x1 = res
            xw = mean1 = rstd1 = qkv = ao = None
    else:
        xw, _, mean1, rstd1 = o.layernorm_fwd(x2d, g1, b1, LN_EPS)
        qkv = o.linear_fwd(xw, Wqkv, bqkv)
        ao, lse = o.window_attn_fwd(qkv, bqkv, geom.win2tok, L, table, geom.ws, geom.region_ids, geom.nW, geom.N, nH, scale, bias_frag=frag)
        x1 = o.linear_fwd(ao, Wproj, bproj, residual=x2d, rowscale=dp1, rows_per_sample=L, out_f32=True)
    if not save:  # inference keeps nothing for a backward: the attention branch's intermediates go before the MLP allocates its own
        xw = qkv = ao = None
    x2, route, mlp_saved, _ = _swin_mlp_fwd(o, x1, (g2, b2, bfc1, bfc2), W1, W2, w1p, dp2, L, save)
    if not save:
        return x2.view(nB, L, C), None
    saved = dict(mean1=mean1, rstd1=rstd1, xw=xw, qkv=qkv, ao=ao, x1=x1, lse=lse, frag=frag, **dict(zip(_MLP_SAVED, mlp_saved or ())))
    return x2.view(nB, L, C), (bwd_fused, route, saved)


class SwinBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, geom, nH, index, dp, g1, b1, table, Wqkv_p, bqkv, Wproj_p, bproj, g2, b2, W1_p, bfc1, W2_p, bfc2):
        Wqkv, Wproj, W1, W2 = wts = (_weight(Wqkv_p), _weight(Wproj_p), _weight(W1_p), _weight(W2_p))
        x = x.contiguous()
        y, (ctx.attn_bwd_fused, ctx.mlp_route, saved) = _block_forward(x, geom, nH, index, dp, (g1, b1, table, bqkv, bproj, g2, b2, bfc1, bfc2), wts, True, W1_p,
                                                                       (Wqkv_p, Wproj_p))
        ctx.geom, ctx.nH, ctx.dp = geom, nH, dp
        ctx.wparams = (Wqkv_p, Wproj_p, W1_p, W2_p)
        ctx.mlp_params = (g2, b2, W1_p, bfc1, W2_p, bfc2)
        ctx.attn_params = (g1, b1, table, Wqkv_p, bqkv, Wproj_p, bproj)
        _save_named(ctx, x=x, index=index, g1=g1, table=table, g2=g2, bqkv=bqkv, b2=b2, bfc1=bfc1, Wqkv=Wqkv, Wproj=Wproj, W1=W1, W2=W2, **saved)
        return y

    @staticmethod
    def backward(ctx, gy):
        o = ops_module()
        geom, nH, dp = ctx.geom, ctx.nH, ctx.dp
        s = _load_named(ctx)
        x, x1, g1, g2, bqkv = s.x, s.x1, s.g1, s.g2, s.bqkv
        nB, L, C = x.shape
        M = nB * L
        scale = (C // nH) ** -0.5
        dp1, dp2 = (None, None) if dp is None else dp
        gy = gy.contiguous().view(M, C)
        Wqkv_p, Wproj_p, W1_p, W2_p = ctx.wparams
        g1_p, b1_p, table_p, _, bqkv_p, _, bproj_p = ctx.attn_params
        g2_p, b2_p, _, bfc1_p, _, bfc2_p = ctx.mlp_params
        # ---- MLP branch ----
        fused_mlp = ctx.mlp_route == "fused"
        onchip = fused_mlp and _mlp_dw_onchip(o, s.W1, C)  # (the kernel scales and casts gy itself: no activation-dtype copy is read)
        dyb = None if onchip else o.gather_cast(gy, M, rowscale=dp2, rows_per_sample=L)
        if fused_mlp:
            gx1, dyw, dg2, db2, dW1, dbfc1, dW2, dbfc2 = _mlp_branch_bwd(o, x1, gy, dyb, g2, s.b2, s.W1, s.bfc1, ctx.mlp_params, _per_row(dp2, L), _per_row(dp1, L))
        else:
            dh, dW1, dbfc1, dW2, dbfc2 = _mlp_bwd(o, dyb, s.h, s.a1, s.a1g, s.W1, s.W2, (W1_p, bfc1_p, W2_p, bfc2_p))
            ln2 = _ln_sinks(g2_p, b2_p)
            # (the LayerNorm backward also emits the DropPath-scaled activation-dtype copy of gx1, the attention branch's operand)
            gx1, dyw, dg2, db2 = o.layernorm_bwd_cast(dh, x1, s.mean2, s.rstd2, g2, g_in=gy, rowscale=dp1, rows_per_sample=L, gb_out=ln2)
            dg2, db2 = _alias(dg2, ln2), _alias(db2, ln2)
        # ---- attention branch ----
        if ctx.attn_bwd_fused:
            gx, _, dg1, db1, dtable, dWqkv, dbqkv, dWproj, dbproj = _attn_branch_bwd(
                o, x.view(M, C), gx1, ((0, nB, L, geom),), nH, (s.frag,), s.index, s.table, s.Wqkv, ctx.attn_params, g1, b1_p.detach(), bqkv,
                _per_row(dp1, L), None, False)
            _side_join()
            return (gx.view(nB, L, C), None, None, None, None, dg1, db1, dtable, dWqkv, dbqkv, dWproj, dbproj, dg2, db2, dW1, dbfc1,
                    dW2, dbfc2)
        dWproj, dbproj = _side_run(lambda: _wgrad(dyw, s.ao, Wproj_p, want_bias=True, bias_param=bproj_p), dyw, s.ao)
        dao = o.linear_dgrad(dyw, s.Wproj)
        dqkv, dbias_ws, dpad_ws = o.window_attn_bwd(s.qkv, bqkv, geom.win2tok, L, dao, s.ao, s.lse, None, geom.ws, geom.region_ids,
                                                    geom.nW, geom.N, nH, scale, bias_frag=s.frag)
        tsink = P.grad_out(table_p)
        dtable = _alias(o.relpos_bias_bwd(dbias_ws, s.index, geom.N, s.table.shape[0], out=tsink, accumulate=False if tsink is not None else None,
                                          **_relpos_kw(o)), tsink)
        if _attn_tail_fused(o, s.Wqkv.dtype, C):
            gx, _, dg1, db1, dWqkv, dbqkv = _attn_tail_bwd(o, dqkv, x.view(M, C), s.mean1, s.rstd1, g1, s.Wqkv, gx1, (dpad_ws,),
                                                           (g1_p, b1_p, Wqkv_p, bqkv_p), None, 1, False)
            _side_join()
            return (gx.view(nB, L, C), None, None, None, None, dg1, db1, dtable, dWqkv, dbqkv, dWproj, dbproj, dg2, db2, dW1, dbfc1, dW2, dbfc2)
        wsink, bsink = P.grad_out(Wqkv_p), P.grad_out(bqkv_p)

        def wqkv():
            dWqkv, dbqkv = o.linear_wgrad(dqkv, s.xw, out=wsink, want_bias=True, db_out=bsink)
            o.colsum(dpad_ws, out=dbqkv[C:], accumulate=True)  # k/v bias gradient from the zero-pad slots
            return dWqkv, dbqkv

        dWqkv, dbqkv = _side_run(wqkv, dqkv, s.xw, dpad_ws)
        dWqkv, dbqkv = _alias(dWqkv, wsink), _alias(dbqkv, bsink)
        dxw = o.linear_dgrad(dqkv, s.Wqkv)
        ln1 = _ln_sinks(g1_p, b1_p)
        gx, dg1, db1 = o.layernorm_bwd(dxw, x.view(M, C), s.mean1, s.rstd1, g1, g_in=gx1, gb_out=ln1)
        _side_join()
        return (gx.view(nB, L, C), None, None, None, None, _alias(dg1, ln1), _alias(db1, ln1), dtable, dWqkv, dbqkv, dWproj, dbproj, dg2, db2, dW1, dbfc1,
                dW2, dbfc2)


# ---- ragged multi-resolution block: all crops of a step in ONE set of GEMM / LayerNorm launches ---------------------
# LayerNorm, the four GEMMs and the residual adds of a block are row-wise, so the token rows of the 224^2 crops and of the
# 96^2 crops can run through them together; only the window attention depends on the image geometry and is launched once per
# resolution group on its row range.  Compared with one pass per group (swin_transformer.py:729-751) this halves the GEMM /
# LayerNorm launches, removes the gradient-accumulation adds of every parameter used by both passes, halves the split-K
# partial traffic of the weight gradients and gives the small local-crop GEMMs of stages 2-3 full grids.
def _block_forward_multi(X, segs, nH, dp_rows, prm, wts, save, pre=None, next_norm=None, w1p=None, wattn=None):
    """X fp32 [M, C]; segs: tuple of (row0, nB, L, geom); dp_rows: None or (per-row DropPath scale attn [M], mlp [M]).
    pre: (norm1(X) in the activation dtype, mean, rstd) when the previous block's fused MLP kernel already produced them;
    next_norm: (weight, bias) of the NEXT block's norm1 -- the fused MLP kernel then also emits that block's `pre`.
    -> (y, None or (is the attention backward the one-kernel mode, MLP route, tensors for the backward by name), lses, next block's pre or None)"""
    o = ops_module()
    (g1, b1, table, bqkv, bproj, g2, b2, bfc1, bfc2) = prm
    (Wqkv, Wproj, W1, W2) = wts
    M, C = X.shape
    scale = (C // nH) ** -0.5
    dp1, dp2 = (None, None) if dp_rows is None else dp_rows
    fused_attn = wattn is not None and _attn_fused(Wqkv.dtype, C, nH, [sg[3] for sg in segs], save, [(sg[1] * sg[2], sg[1] * sg[3].nW) for sg in segs])
    lses, frags = [], {}
    bwd_fused = False
    if fused_attn:
        # the whole branch in one kernel per resolution group; `pre` (the LayerNorm output the previous block's fused MLP kernel may
        # have produced) is not needed: the kernel normalises the rows it loads for the residual anyway
        Wq_p, Wp_p = _perm_w(wattn[0]), _perm_w(wattn[1])
        x1 = torch.empty_like(X)
        # (a training pass whose backward is the one-kernel mode needs no side outputs)
        bwd_fused = bool(save) and _attn_bwd_fused(o, Wqkv.dtype, C, nH, [sg[3] for sg in segs], [(sg[1] * sg[2], sg[1] * sg[3].nW) for sg in segs])
        side = bool(save) and not bwd_fused
        if side:
            xw = torch.empty((M, C), dtype=Wqkv.dtype, device=X.device)
            qkv = torch.empty((M, 3 * C), dtype=Wqkv.dtype, device=X.device)
            ao = torch.empty((M, C), dtype=Wqkv.dtype, device=X.device)
            mean1 = torch.empty((M,), dtype=torch.float32, device=X.device)
            rstd1 = torch.empty_like(mean1)
        else:
            xw = qkv = ao = mean1 = rstd1 = None
        for (r0, nB, L, geom) in segs:
            r1 = r0 + nB * L
            first = (geom.ws, geom.N) not in frags
            if first:
                frags[(geom.ws, geom.N)] = o.new_bias_frag(nH, geom.N, X.device)
            sv = (xw[r0:r1], mean1[r0:r1], rstd1[r0:r1], qkv[r0:r1], ao[r0:r1]) if side else False
            o.attn_branch_fwd(X[r0:r1], g1, b1, LN_EPS, Wq_p, bqkv, Wp_p, bproj, geom.win2tok, L, table if first else None, geom.ws, geom.region_ids,
                              geom.nW, geom.N, nH, scale, rowscale=None if dp1 is None else dp1[r0:r1], out=x1[r0:r1],
                              bias_frag=frags[(geom.ws, geom.N)], save=sv)
            lses.append((None, frags[(geom.ws, geom.N)]))
        # (the next block of the stage takes the same route and needs no LayerNorm hand-over)
        next_norm = None
    else:
        if pre is not None:
            xw, mean1, rstd1 = pre
        else:
            xw, _, mean1, rstd1 = o.layernorm_fwd(X, g1, b1, LN_EPS)
        qkv = o.linear_fwd(xw, Wqkv, bqkv)
        ao = torch.empty((M, C), dtype=qkv.dtype, device=X.device)
        for (r0, nB, L, geom) in segs:
            r1 = r0 + nB * L
            # the fragment-order bias is built once per block and step: later groups and the backward reuse it
            first = (geom.ws, geom.N) not in frags
            if first:
                frags[(geom.ws, geom.N)] = o.new_bias_frag(nH, geom.N, X.device)
            _, lse = o.window_attn_fwd(qkv[r0:r1], bqkv, geom.win2tok, L, table if first else None, geom.ws, geom.region_ids, geom.nW, geom.N, nH, scale,
                                       out=ao[r0:r1], bias_frag=frags[(geom.ws, geom.N)])
            lses.append((lse, frags[(geom.ws, geom.N)]))
        x1 = o.linear_fwd(ao, Wproj, bproj, residual=X, rowscale=dp1, rows_per_sample=1, out_f32=True)
    x2, route, mlp_saved, nxt = _swin_mlp_fwd(o, x1, (g2, b2, bfc1, bfc2), W1, W2, w1p, dp2, 1, save, next_norm)
    if not save:
        return x2, None, lses, nxt
    saved = dict(mean1=mean1, rstd1=rstd1, xw=xw, qkv=qkv, ao=ao, x1=x1, **dict(zip(_MLP_SAVED, mlp_saved or ())))
    return x2, (bwd_fused, route, saved), lses, nxt


class SwinBlockMultiFn(torch.autograd.Function):
    """One Swin block over the token rows of several resolution groups.

    Besides y the block returns a SHADOW output ysh (an uninitialised [M, C] tensor of the activation dtype, never read or
    written in the forward).  It exists for the backward: the next block of the stage takes (y, ysh) as inputs and returns,
    as the "gradient" of ysh, cast(prev_scale * dL/dy) -- the activation-dtype, DropPath-scaled copy of dL/dy that this block's
    MLP-branch GEMMs need as their operand -- emitted by the LayerNorm-backward pass that produces dL/dy anyway
    (ops.layernorm_bwd_cast) instead of a separate read-and-cast pass over dL/dy.  If nobody consumes ysh (last block of a
    stage) its gradient arrives as None and the block casts dL/dy itself."""

    @staticmethod
    def forward(ctx, X, Xsh, segs, nH, index, dp_rows, prev_scale, pre, next_norm, g1, b1, table, Wqkv_p, bqkv, Wproj_p, bproj, g2, b2, W1_p, bfc1,
                W2_p, bfc2):
        """pre / next_norm: see _block_forward_multi (plain tuples: no gradient flows through them -- norm1's own backward uses
        the saved statistics).  Third output: the next block's `pre` tuple flattened (xw, mean, rstd), or three None"""
        Wqkv, Wproj, W1, W2 = wts = (_weight(Wqkv_p), _weight(Wproj_p), _weight(W1_p), _weight(W2_p))
        X = X.contiguous()
        y, (ctx.attn_bwd_fused, ctx.mlp_route, saved), lses, nxt = _block_forward_multi(X, segs, nH, dp_rows, (g1, b1, table, bqkv, bproj, g2, b2, bfc1, bfc2), wts,
                                                                                        True, pre, next_norm, W1_p, (Wqkv_p, Wproj_p))
        ctx.segs, ctx.nH, ctx.dp_rows, ctx.lses = segs, nH, dp_rows, lses
        ctx.wparams = (Wqkv_p, Wproj_p, W1_p, W2_p)
        ctx.sparams = (g1, b1, table, bqkv, bproj, g2, b2, bfc1, bfc2)  # small parameters: their gradients go to bucket slots too
        ctx.emit_shadow, ctx.prev_scale = Xsh is not None, prev_scale
        ctx.set_materialize_grads(False)
        _save_named(ctx, X=X, index=index, g1=g1, table=table, g2=g2, bqkv=bqkv, b2=b2, bfc1=bfc1, Wqkv=Wqkv, Wproj=Wproj, W1=W1, W2=W2, **saved)
        ysh = torch.empty(X.shape, dtype=Wqkv.dtype, device=X.device)
        if nxt is None:
            return y, ysh, None, None, None
        ctx.mark_non_differentiable(*nxt)
        return (y, ysh) + tuple(nxt)

    @staticmethod
    def backward(ctx, gy, gysh, *_unused):
        o = ops_module()
        segs, nH, dp_rows = ctx.segs, ctx.nH, ctx.dp_rows
        s = _load_named(ctx)
        X, index, g1, table, g2, bqkv, Wqkv, x1, xw, qkv, ao = s.X, s.index, s.g1, s.table, s.g2, s.bqkv, s.Wqkv, s.x1, s.xw, s.qkv, s.ao
        M, C = X.shape
        scale = (C // nH) ** -0.5
        dp1, dp2 = (None, None) if dp_rows is None else dp_rows
        gy = gy.contiguous()
        Wqkv_p, Wproj_p, W1_p, W2_p = ctx.wparams
        g1_p, b1_p, table_p, bqkv_p, bproj_p, g2_p, b2_p, bfc1_p, bfc2_p = ctx.sparams
        # ---- MLP branch ----
        fused_mlp = ctx.mlp_route == "fused"
        if gysh is not None:
            dyb = gysh.contiguous()
        else:
            dyb = None if (fused_mlp and _mlp_dw_onchip(o, s.W1, C)) else o.gather_cast(gy, M, rowscale=dp2, rows_per_sample=1)
        if fused_mlp:
            gx1, dyw, dg2, db2, dW1, dbfc1, dW2, dbfc2 = _mlp_branch_bwd(o, x1, gy, dyb, g2, s.b2, s.W1, s.bfc1,
                                                                          (g2_p, b2_p, W1_p, bfc1_p, W2_p, bfc2_p), dp2, dp1)
        else:
            dh, dW1, dbfc1, dW2, dbfc2 = _mlp_bwd(o, dyb, s.h, s.a1, s.a1g, s.W1, s.W2, (W1_p, bfc1_p, W2_p, bfc2_p))
            ln2 = _ln_sinks(g2_p, b2_p)
            gx1, dyw, dg2, db2 = o.layernorm_bwd_cast(dh, x1, s.mean2, s.rstd2, g2, g_in=gy, rowscale=dp1, rows_per_sample=1, gb_out=ln2)
            dg2, db2 = _alias(dg2, ln2), _alias(db2, ln2)
        # ---- attention branch ----
        if ctx.attn_bwd_fused:
            gx, gxb, dg1, db1, dtable, dWqkv, dbqkv, dWproj, dbproj = _attn_branch_bwd(
                o, X, gx1, segs, nH, [fr for (_, fr) in ctx.lses], index, table, Wqkv, (g1_p, b1_p, table_p, Wqkv_p, bqkv_p, Wproj_p, bproj_p), g1,
                b1_p.detach(), bqkv, dp1, ctx.prev_scale, ctx.emit_shadow)
            _side_join()
            return (gx, gxb, None, None, None, None, None, None, None, dg1, db1, dtable, dWqkv, dbqkv, dWproj, dbproj, dg2, db2, dW1, dbfc1, dW2, dbfc2)
        dWproj, dbproj = _side_run(lambda: _wgrad(dyw, ao, Wproj_p, want_bias=True, bias_param=bproj_p), dyw, ao)
        dao = o.linear_dgrad(dyw, s.Wproj)
        dqkv = torch.empty_like(qkv)
        tsink = P.grad_out(table_p)
        # the bias-gradient slabs of all groups in one buffer: ONE fold + scatter launch per block (every launch between the large kernels of
        # this chain is ~10 us of step time, profiles/r06_finish_offchain_ab.txt)
        N = segs[0][3].N
        assert all(geom.N == N for (_, _, _, geom) in segs)
        dbuf, dslabs = o.attn_dbias_slabs(N, [nB * geom.nW for (_, nB, _, geom) in segs], nH, qkv.device)
        pads = []
        for (r0, nB, L, geom), (lse, frag), dslab in zip(segs, ctx.lses, dslabs):
            r1 = r0 + nB * L
            _, _, dpad_ws = o.window_attn_bwd(qkv[r0:r1], bqkv, geom.win2tok, L, dao[r0:r1], ao[r0:r1], lse, None, geom.ws, geom.region_ids,
                                              geom.nW, geom.N, nH, scale, dqkv_out=dqkv[r0:r1], bias_frag=frag, dbias_out=dslab)
            pads.append(dpad_ws)
        dtable = o.relpos_bias_bwd(dbuf, index, N, table.shape[0], out=tsink, accumulate=False if tsink is not None else None, **_relpos_kw(o))
        dtable = _alias(dtable, tsink)
        if _attn_tail_fused(o, Wqkv.dtype, C):  # (the previous block's operand rides along with dL/dX when it has a reader)
            gx, gxb, dg1, db1, dWqkv, dbqkv = _attn_tail_bwd(o, dqkv, X, s.mean1, s.rstd1, g1, Wqkv, gx1, pads, (g1_p, b1_p, Wqkv_p, bqkv_p),
                                                             ctx.prev_scale, 1, ctx.emit_shadow)
            _side_join()
            return (gx, gxb, None, None, None, None, None, None, None, dg1, db1, dtable, dWqkv, dbqkv, dWproj, dbproj, dg2, db2, dW1, dbfc1, dW2, dbfc2)
        wsink, bsink = P.grad_out(Wqkv_p), P.grad_out(bqkv_p)

        def wqkv():
            dWqkv, dbqkv = o.linear_wgrad(dqkv, xw, out=wsink, want_bias=True, db_out=bsink)
            for dpad_ws in pads:
                o.colsum(dpad_ws, out=dbqkv[C:], accumulate=True)  # k/v bias gradient from the zero-pad slots
            return dWqkv, dbqkv

        dWqkv, dbqkv = _side_run(wqkv, dqkv, xw, pads)
        dWqkv, dbqkv = _alias(dWqkv, wsink), _alias(dbqkv, bsink)
        dxw = o.linear_dgrad(dqkv, Wqkv)
        ln1 = _ln_sinks(g1_p, b1_p)
        if ctx.emit_shadow:  # the previous block's operand rides along with dL/dX
            gx, gxb, dg1, db1 = o.layernorm_bwd_cast(dxw, X, s.mean1, s.rstd1, g1, g_in=gx1, rowscale=ctx.prev_scale, rows_per_sample=1, gb_out=ln1)
        else:
            gx, dg1, db1 = o.layernorm_bwd(dxw, X, s.mean1, s.rstd1, g1, g_in=gx1, gb_out=ln1)
            gxb = None
        dg1, db1 = _alias(dg1, ln1), _alias(db1, ln1)
        _side_join()
        return (gx, gxb, None, None, None, None, None, None, None, dg1, db1, dtable, dWqkv, dbqkv, dWproj, dbproj, dg2, db2, dW1, dbfc1, dW2, dbfc2)


def swin_block_multi(X, segs, nH, index, dp_rows, prm_list, shadow=None, prev_scale=None, pre=None, next_norm=None):
    """one Swin block over the token rows of several resolution groups; X fp32 [M, C].  -> (y, shadow of y or None, next block's
    `pre` or None); pass the previous block's shadow and its MLP-branch DropPath row scale to let this block's backward emit that
    block's cast gradient (see SwinBlockMultiFn).  pre / next_norm: the LayerNorm hand-over between the blocks of a stage
    (_block_forward_multi)"""
    if torch.is_grad_enabled() and (X.requires_grad or any(p.requires_grad for p in prm_list)):
        y, ysh, xw, mean, rstd = SwinBlockMultiFn.apply(X, shadow, segs, nH, index, dp_rows, prev_scale, pre, next_norm, *prm_list)
        w1 = _weight(prm_list[9])
        if _mlp_fused_train(w1, X.shape[1]) and _mlp_dw_onchip(ops_module(), w1, X.shape[1]):
            ysh = None  # (this block's MLP backward scales and casts dL/dy itself: nobody would read the copy its successor wrote)
        return y, ysh, (None if xw is None else (xw, mean, rstd))
    g1, b1, table, Wqkv, bqkv, Wproj, bproj, g2, b2, W1, bfc1, W2, bfc2 = prm_list
    wts = (_weight(Wqkv), _weight(Wproj), _weight(W1), _weight(W2))
    y, _, _, nxt = _block_forward_multi(X.contiguous(), segs, nH, dp_rows, (g1, b1, table, bqkv, bproj, g2, b2, bfc1, bfc2), wts, False, pre, next_norm, W1,
                                        (Wqkv, Wproj))
    return y, None, nxt


def swin_block(x, geom, nH, index, dp, prm_list):
    """prm_list: [g1, b1, table, Wqkv, bqkv, Wproj, bproj, g2, b2, W1, bfc1, W2, bfc2] (fp32 parameters)."""
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in prm_list)):
        return SwinBlockFn.apply(x, geom, nH, index, dp, *prm_list)
    g1, b1, table, Wqkv, bqkv, Wproj, bproj, g2, b2, W1, bfc1, W2, bfc2 = prm_list
    wts = (_weight(Wqkv), _weight(Wproj), _weight(W1), _weight(W2))
    y, _ = _block_forward(x.contiguous(), geom, nH, index, dp, (g1, b1, table, bqkv, bproj, g2, b2, bfc1, bfc2), wts, False, W1, (Wqkv, Wproj))
    return y


def swin_block_attention(x, geom, nH, index, prm_list):
    """forward of one block that also returns the softmax tensor (swin_transformer.py:146,152); inference only."""
    o = ops_module()
    g1, b1, table, Wqkv, bqkv, Wproj, bproj, g2, b2, W1, bfc1, W2, bfc2 = prm_list
    nB, L, C = x.shape
    x2d = x.contiguous().view(nB * L, C)
    xw, _, _, _ = o.layernorm_fwd(x2d, g1, b1, LN_EPS)
    qkv = o.linear_fwd(xw, _weight(Wqkv), bqkv)
    _, _, attn = o.window_attn_fwd(qkv, bqkv, geom.win2tok, L, table, geom.ws, geom.region_ids, geom.nW, geom.N, nH, (C // nH) ** -0.5,
                                   want_attn=True)
    return attn


def _window_stats_route(o, dtype, N, hd):
    """do the window statistics take the kernels (ops.window_attn_stats)?  When the ops module has the entry and supports the shape; an
    ops module without it (the CPU restatement, oracle/ops_ref.py) or an unsupported shape reduces the maps of window_attn_fwd"""
    if not hasattr(o, "window_attn_stats"):
        return False
    sup = getattr(o, "window_attn_stats_supported", None)
    return sup is not None and bool(sup(dtype, N, hd))


def window_attention_stats(o, qkv, qkv_bias, geom, L, table, nH, scale, slots=None):
    """what an attention analysis reads of a block's window softmax, token-ordered qkv [nB * L, 3C] -> (entropy fp32 [nB * nW, nH, N] in
    nats with 0 log 0 = 0, window-slot order; rows fp32 [nB, nH, nq, N] of the listed slots w * N + i over their own windows, or None).
    The statistics mode of the window kernels never forms a map; the fall-back forms the maps of o.window_attn_fwd(want_attn=True) for a
    slice of the batch at a time and reduces them in torch."""
    nW, N = geom.nW, geom.N
    hd = qkv.shape[1] // 3 // nH
    if _window_stats_route(o, qkv.dtype, N, hd):
        return o.window_attn_stats(qkv, qkv_bias, geom.win2tok, L, table, geom.ws, geom.region_ids, nW, N, nH, scale, slots=slots)
    idx = None
    if slots is not None:
        idx = torch.as_tensor(list(slots) if isinstance(slots, range) else slots, device=qkv.device).reshape(-1).long()
        if idx.numel() and not (0 <= int(idx.min()) and int(idx.max()) < nW * N):
            raise ValueError("window_attention_stats: slot indices must lie in [0, %d)" % (nW * N))
    nB = qkv.shape[0] // L
    step = max(1, _STATS_SLICE_ELEMS // (nW * nH * N * N))
    ents, rows = [], []
    for b0 in range(0, nB, step):
        nb = min(step, nB - b0)
        p = o.window_attn_fwd(qkv[b0 * L:(b0 + nb) * L], qkv_bias, geom.win2tok, L, table, geom.ws, geom.region_ids, nW, N, nH, scale,
                              want_attn=True)[2].float()
        ents.append(torch.special.entr(p).sum(-1))
        if idx is not None:  # [nb, nW, nH, N, N] -> the rows (window, query) of the list: [nb, nH, nq, N]
            rows.append(p.view(nb, nW, nH, N, N)[:, idx // N, :, idx % N].permute(1, 2, 0, 3) if idx.numel()
                        else p.new_zeros(nb, nH, 0, N))
    return torch.cat(ents), (torch.cat(rows) if idx is not None else None)


def swin_block_attention_stats(x, geom, nH, index, prm_list, slots=None):
    """window_attention_stats of a block's attention on its input x fp32 [nB, L, C] (LayerNorm and the qkv projection are recomputed, as
    swin_block_attention does); inference only."""
    o = ops_module()
    g1, b1, table, Wqkv, bqkv = prm_list[:5]
    nB, L, C = x.shape
    xw, _, _, _ = o.layernorm_fwd(x.contiguous().view(nB * L, C), g1, b1, LN_EPS)
    qkv = o.linear_fwd(xw, _weight(Wqkv), bqkv)
    return window_attention_stats(o, qkv, bqkv, geom, L, table, nH, (C // nH) ** -0.5, slots)


# ------------------------------------------------------------------------------------------------
# PatchEmbed / PatchMerging / final norm / pooling
# ------------------------------------------------------------------------------------------------
def _patch_cols(o, img, patch, Kc, out=None):
    """im2col of [nB, 3, H, W] for the patch projection.  An ops module whose patch_im2col takes square images only (the CPU restatement)
    gets the columns of a rectangle from F.unfold, which has the same (c, ph, pw) order (as VitPatchEmbedFn)"""
    H, Wd = img.shape[-2:]
    if H == Wd or getattr(o, "PATCH_IM2COL_RECT", False):
        return o.patch_im2col(img.contiguous(), patch, Kc) if out is None else o.patch_im2col(img.contiguous(), patch, Kc, out=out)
    if H % patch or Wd % patch:
        raise ValueError("patch embedding: image %dx%d is not made of whole %d-pixel patches" % (H, Wd, patch))
    cols = o.cast_to_act(torch.nn.functional.unfold(img.float(), patch, stride=patch).transpose(1, 2).reshape(-1, Kc).contiguous())
    return cols if out is None else out.copy_(cols)


# bf16 mode, 4 x 4 patches of 3 channels with PATCH_NORM: projection + LayerNorm in ONE kernel straight from the images, and a backward
# that recomputes them per tile and keeps dW, dbp, dgamma, dbeta on the chip (the fused mode of esvit_patch_im2col) -- the column matrix,
# the projection output and dL/dy are never written, and only the images, mean, rstd are kept for the backward.  "0": A-B runs.
PATCH_FUSED = os.environ.get("ESVIT_PATCH_FUSED", "1") != "0"


def _patch_fused(o, Wp, g, patch, imgs):
    return (PATCH_FUSED and g is not None and hasattr(o, "patch_embed_fwd") and o.act_dtype() == torch.bfloat16
            and o.patch_embed_supported(o.act_dtype(), Wp.shape[0], patch, Wp.shape[1])
            and all(im.dtype == torch.float32 and im.shape[1] == 3 and im.shape[2] % 4 == 0 and im.shape[3] % 4 == 0 for im in imgs))


def _patch_fused_fwd(ctx, o, Wp, bp, g, b, imgs):
    E = Wp.shape[0]
    imgs = [im.contiguous() for im in imgs]
    W = _weight(Wp, (E, o.PATCH_EMBED_K))
    train = any(ctx.needs_input_grad)
    x, mean, rstd = o.patch_embed_fwd(imgs, W, bp.detach(), g.detach(), b.detach(), LN_EPS, stats=train)
    ctx.fused, ctx.params = True, (Wp, bp, g, b)
    if train:
        ctx.save_for_backward(mean, rstd, g, W, bp, *imgs)
    return x


def _patch_fused_bwd(ctx, o, gx):
    mean, rstd, g, W, bp = ctx.saved_tensors[:5]
    imgs = list(ctx.saved_tensors[5:])
    Wp, bp_p, g_p, b_p = ctx.params
    E = W.shape[0]
    sinks = [P.grad_out(Wp, (E, o.PATCH_EMBED_K)), P.grad_out(bp_p), P.grad_out(g_p), P.grad_out(b_p)]
    part, nparts = o.patch_embed_bwd(imgs, W, bp.detach(), g.detach(), gx.contiguous().view(mean.shape[0], E), mean, rstd)
    # the fold of the partial records is a leaf like the weight-gradient GEMM it replaces: same side stream, same join
    outs = _side_run(lambda: o.patch_embed_reduce(part, nparts, E, out=sinks), part)
    _side_join()
    dW, dbp, dg, db = [_alias(t, sk) for t, sk in zip(outs, sinks)]
    return dW.view(ctx.wshape), dbp, dg, db


class PatchEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, Wp, bp, g, b, patch):
        o = ops_module()
        E = Wp.shape[0]
        Kc = Wp.shape[1] * patch * patch
        nB, _, S, Sw = img.shape
        ctx.fused = False
        if _patch_fused(o, Wp, g, patch, [img]):
            ctx.wshape = tuple(Wp.shape)
            return _patch_fused_fwd(ctx, o, Wp, bp, g, b, [img]).view(nB, (S // patch) * (Sw // patch), E)
        cols = _patch_cols(o, img, patch, Kc)
        W = _weight(Wp, (E, Kc))
        y = o.linear_fwd(cols, W, bp, out_f32=True)
        ctx.wshape = tuple(Wp.shape)
        if g is None:  # PATCH_NORM False (swin_transformer.py:476-477, 492-493): the projection is the embedding
            ctx.save_for_backward(cols)
            return y.view(nB, (S // patch) * (Sw // patch), E)
        x, _, mean, rstd = o.layernorm_fwd(y, g, b, LN_EPS, dtype=torch.float32)
        ctx.save_for_backward(cols, y, mean, rstd, g)
        return x.view(nB, (S // patch) * (Sw // patch), E)

    @staticmethod
    def backward(ctx, gx):
        o = ops_module()
        if ctx.fused:
            return (None,) + _patch_fused_bwd(ctx, o, gx) + (None,)
        if len(ctx.saved_tensors) == 1:
            (cols,) = ctx.saved_tensors
            M = cols.shape[0]
            dW, dbp = o.linear_wgrad(o.gather_cast(gx.contiguous().view(M, -1), M), cols, want_bias=True)
            return None, dW.view(ctx.wshape), dbp, None, None, None
        cols, y, mean, rstd, g = ctx.saved_tensors
        M, E = y.shape
        dyb, dg, db = o.layernorm_bwd_to_act(gx.contiguous().view(M, E), y, mean, rstd, g)  # (as PatchEmbedMultiFn)
        dW, dbp = o.linear_wgrad(dyb, cols, want_bias=True)
        dW = dW.view(ctx.wshape)
        return None, dW, dbp, dg, db, None


class PatchEmbedMultiFn(torch.autograd.Function):
    """PatchEmbed of several image batches (one per resolution) at once: the im2col images of all groups share one row
    buffer, so the projection GEMM, its LayerNorm and their backward run once.  Returns fp32 token rows [sum_g nB_g L_g, E]
    (group-major, then sample, then token -- the layout Fn.swin_block_multi consumes)."""

    @staticmethod
    def forward(ctx, Wp, bp, g, b, patch, *imgs):
        o = ops_module()
        E = Wp.shape[0]
        Kc = Wp.shape[1] * patch * patch
        ctx.wshape, ctx.n_img, ctx.fused = tuple(Wp.shape), len(imgs), False
        if _patch_fused(o, Wp, g, patch, imgs):
            return _patch_fused_fwd(ctx, o, Wp, bp, g, b, imgs)
        rows = [im.shape[0] * (im.shape[2] // patch) * (im.shape[3] // patch) for im in imgs]  # one entry per crop tensor, in crop order
        cols = torch.empty((sum(rows), Kc), dtype=o.act_dtype(), device=imgs[0].device)
        r0 = 0
        for im, n in zip(imgs, rows):  # (the reference concatenates the crops of a resolution first, swin_transformer.py:741)
            _patch_cols(o, im, patch, Kc, out=cols[r0:r0 + n])
            r0 += n
        y = o.linear_fwd(cols, _weight(Wp, (E, Kc)), bp, out_f32=True)
        ctx.wshape, ctx.n_img = tuple(Wp.shape), len(imgs)
        if g is None:  # PATCH_NORM False
            ctx.save_for_backward(cols)
            return y
        x, _, mean, rstd = o.layernorm_fwd(y, g, b, LN_EPS, dtype=torch.float32)
        ctx.save_for_backward(cols, y, mean, rstd, g)
        return x

    @staticmethod
    def backward(ctx, gx):
        o = ops_module()
        if ctx.fused:
            return _patch_fused_bwd(ctx, o, gx) + (None,) + (None,) * ctx.n_img
        if len(ctx.saved_tensors) == 1:
            (cols,) = ctx.saved_tensors
            M = cols.shape[0]
            dW, dbp = o.linear_wgrad(o.gather_cast(gx.contiguous().view(M, -1), M), cols, want_bias=True)
            return (dW.view(ctx.wshape), dbp, None, None, None) + (None,) * ctx.n_img
        cols, y, mean, rstd, g = ctx.saved_tensors
        M, E = y.shape
        # dL/dy of the norm is only ever the operand of the projection's weight gradient: written once, in the activation dtype
        dya, dg, db = o.layernorm_bwd_to_act(gx.contiguous().view(M, E), y, mean, rstd, g)
        dW, dbp = o.linear_wgrad(dya, cols, want_bias=True)
        return (dW.view(ctx.wshape), dbp, dg, db, None) + (None,) * ctx.n_img


class PatchMergeMultiFn(torch.autograd.Function):
    """PatchMerging over the token rows of several resolution groups: the 2x2 gather + LayerNorm(4C) runs per group (it
    depends on the grid) into one shared row buffer; the reduction GEMM, its dgrad and wgrad run once over all rows.
    X fp32 [M, C], groups: tuple of (row0, nB, H, W) -> fp32 [sum nB*Ho*Wo, 2C] with the groups in the same order ((Ho, Wo) =
    merged_grid(H, W): M/4 rows when every grid is even; an odd grid goes through the pad mode of the kernel, see MERGE_PAD).

    The node takes part in the shadow protocol of SwinBlockMultiFn on both sides.  Xsh / prev_scale: the shadow output and the
    MLP-branch DropPath row scale of the stage's last block -- the LayerNorm backward that produces dL/dX also emits
    cast(prev_scale * dL/dX), that block's GEMM operand.  Second output: a shadow of the merged rows for the next stage's first block,
    whose LayerNorm backward hands back cast(dL/dY) -- the operand of this node's reduction GEMMs -- instead of a cast pass over dL/dY."""

    @staticmethod
    def forward(ctx, X, Xsh, prev_scale, groups, g, b, Wr):
        o = ops_module()
        X = X.contiguous()
        M, C = X.shape
        qs, Q = merged_row_offsets(groups)
        y = torch.empty((Q, 4 * C), dtype=o.act_dtype(), device=X.device)
        mean = torch.empty((Q,), dtype=torch.float32, device=X.device)
        rstd = torch.empty_like(mean)
        for (r0, nB, H, W), (q0, q1) in zip(groups, qs):
            o.merge_ln_fwd(X[r0:r0 + nB * H * W].view(nB, H * W, C), g, b, LN_EPS, H, W, out=(y[q0:q1], mean[q0:q1], rstd[q0:q1]),
                           **_merge_pad_kw(H, W))
        Wc = _weight(Wr)
        out = o.linear_fwd(y, Wc, None, out_f32=True)
        ctx.save_for_backward(X, y, mean, rstd, g, Wc)
        ctx.groups, ctx.wparam = groups, Wr
        ctx.emit_shadow, ctx.prev_scale = Xsh is not None, prev_scale
        ctx.set_materialize_grads(False)
        outsh = torch.empty(out.shape, dtype=y.dtype, device=X.device) if any(ctx.needs_input_grad) else None
        return out, outsh

    @staticmethod
    def backward(ctx, go, gosh):
        o = ops_module()
        X, y, mean, rstd, g, Wc = ctx.saved_tensors
        M, C = X.shape
        qs, Q = merged_row_offsets(ctx.groups)
        gob = gosh.contiguous() if gosh is not None else o.gather_cast(go.contiguous(), Q)
        dWr = _side_run(lambda: _wgrad(gob, y, ctx.wparam), gob, y)
        dy = o.linear_dgrad(gob, Wc)
        dX = torch.empty_like(X)
        dXsh = torch.empty((M, C), dtype=y.dtype, device=X.device) if ctx.emit_shadow else None
        ps = ctx.prev_scale
        gb = torch.empty((2, 4 * C), dtype=torch.float32, device=X.device)  # dgamma | dbeta: the first group writes, later ones accumulate
        for gi, ((r0, nB, H, W), (q0, q1)) in enumerate(zip(ctx.groups, qs)):
            r1 = r0 + nB * H * W
            o.merge_ln_bwd(dy[q0:q1], X[r0:r1].view(nB, H * W, C), mean[q0:q1], rstd[q0:q1], g, H, W, dx_out=dX[r0:r1], gb_out=gb,
                           accumulate=gi > 0, act_out=None if dXsh is None else dXsh[r0:r1], rowscale=None if (ps is None or dXsh is None) else ps[r0:r1],
                           **_merge_pad_kw(H, W))
        _side_join()
        return dX, dXsh, None, None, gb[0], gb[1], dWr


def merged_row_offsets(groups):
    """groups (row0, nB, H, W) -> ([(q0, q1) merged-row range per group], total merged rows): cumulative, since a group with an odd
    side has more than a quarter of its rows left"""
    qs, q = [], 0
    for (_, nB, H, W) in groups:
        Ho, Wo = merged_grid(H, W)
        qs.append((q, q + nB * Ho * Wo))
        q += nB * Ho * Wo
    return qs, q


def _merge_pad_kw(H, W):
    """keyword of o.merge_ln_fwd / _bwd: an odd grid asks for the pad mode of the kernel (an even one is called as ever)"""
    return {"pad": True} if (H % 2 or W % 2) else {}


class PatchMergeFn(torch.autograd.Function):
    """x fp32 [nB, H*W, C] -> [nB, Ho*Wo, 2C], (Ho, Wo) = merged_grid(H, W); an odd H or W goes through the kernel's pad mode (the caller
    has checked that the ops module offers it, or padded the grid itself)"""

    @staticmethod
    def forward(ctx, x, H, W, g, b, Wr):
        o = ops_module()
        x = x.contiguous()
        nB, L, C = x.shape
        Ho, Wo = merged_grid(H, W)
        y, mean, rstd = o.merge_ln_fwd(x, g, b, LN_EPS, H, W, **_merge_pad_kw(H, W))
        Wc = _weight(Wr)
        out = o.linear_fwd(y, Wc, None, out_f32=True)
        ctx.save_for_backward(x, y, mean, rstd, g, Wc)
        ctx.hw, ctx.wparam = (H, W), Wr
        return out.view(nB, Ho * Wo, 2 * C)

    @staticmethod
    def backward(ctx, go):
        o = ops_module()
        x, y, mean, rstd, g, Wc = ctx.saved_tensors
        H, W = ctx.hw
        rows = y.shape[0]
        gb = o.gather_cast(go.contiguous().view(rows, -1), rows)
        dWr = _wgrad(gb, y, ctx.wparam)
        dy = o.linear_dgrad(gb, Wc)
        dx, dg, db = o.merge_ln_bwd(dy, x, mean, rstd, g, H, W, **_merge_pad_kw(H, W))
        return dx, None, None, dg, db, dWr


class PadTokensFn(torch.autograd.Function):
    """zero-pad a token grid at the bottom / right ([nB, H*W, C] -> [nB, Hp*Wp, C]): F.pad of PatchMerging for odd feature
    maps (swin_transformer.py:406-408); the backward is the crop"""

    @staticmethod
    def forward(ctx, x, H, W, Hp, Wp):
        nB, L, C = x.shape
        ctx.geo = (nB, H, W, Hp, Wp)
        return ops_module().pad_crop_tokens(x.contiguous().view(nB * L, C), nB, H, W, Hp, Wp).view(nB, Hp * Wp, C)

    @staticmethod
    def backward(ctx, gy):
        nB, H, W, Hp, Wp = ctx.geo
        C = gy.shape[-1]
        return ops_module().pad_crop_tokens(gy.contiguous().view(nB * Hp * Wp, C), nB, Hp, Wp, H, W).view(nB, H * W, C), None, None, None, None


class FinalNormFn(torch.autograd.Function):
    """x fp32 [nB, T, C] -> LayerNorm(x) fp32 (the region features the loss matches on stay fp32)."""

    @staticmethod
    def forward(ctx, x, g, b, eps=LN_EPS):
        o = ops_module()
        x = x.contiguous()
        y, _, mean, rstd = o.layernorm_fwd(x.view(-1, x.shape[-1]), g, b, eps, dtype=torch.float32)
        ctx.save_for_backward(x, mean, rstd, g)
        ctx.nparams = (g, b)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        o = ops_module()
        x, mean, rstd, g = ctx.saved_tensors
        C = x.shape[-1]
        sinks = _ln_sinks(*ctx.nparams)
        dx, dg, db = o.layernorm_bwd(gy.contiguous().view(-1, C), x.view(-1, C), mean, rstd, g, gb_out=sinks)
        return dx.view(x.shape), _alias(dg, sinks), _alias(db, sinks), None


class TokenMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        o = ops_module()
        m, _ = o.token_mean_fwd(x.contiguous())
        ctx.T = x.shape[1]
        return m

    @staticmethod
    def backward(ctx, gm):
        return ops_module().token_mean_bwd(gm.contiguous(), None, ctx.T)


# ------------------------------------------------------------------------------------------------
# DINOHead
# ------------------------------------------------------------------------------------------------
def _last_layer_weight(v, g):
    o = ops_module()
    if v.requires_grad or g.requires_grad:
        return P.cached(v, "wn", lambda: o.weightnorm_fwd(v.detach(), g.detach()))
    return o.weightnorm_fwd(v.detach(), g.detach())


def _last_logits(o, z, w, stats):
    """logits of the weight-normed last layer (vision_transformer.py:418); with stats = (inv_temp, center) and a shape the GEMM's
    statistics epilogue covers also their softmax row statistics -> (logits, row_max | None, row_lse | None)"""
    if stats is not None and o.row_stats_supported(z.dtype, z.shape[0], w.shape[0]):
        return o.linear_fwd(z, w, row_stats=stats)
    return o.linear_fwd(z, w), None, None


def _head_forward(x, params, save, stats=None):
    """DINOHead without BatchNorm and with any number of Linear layers (vision_transformer.py:388-402, 414-418): nlayers = 1 is one
    Linear into the bottleneck, otherwise Linear + GELU (nlayers - 1 times) and a last Linear; then l2-normalise and the weight-normed
    last layer.  params = (W_1, b_1, ..., W_L, b_L, weight_v, weight_g) -> ((logits, row_max | None, row_lse | None), tensors for the
    backward by name).  save False: an inference pass, which writes no pre-activations"""
    o = ops_module()
    L = (len(params) - 2) // 2
    Wp, bp = params[0:2 * L:2], params[1:2 * L:2]
    v, g = params[2 * L:]
    Ws = [_weight(w) for w in Wp]
    acts, pres = [o.cast_to_act(x.contiguous())], []
    for i in range(L - 1):
        if save:
            hg, hpre = o.linear_fwd(acts[-1], Ws[i], bp[i], gelu=True, want_preact=True)
        else:
            hg, hpre = o.linear_fwd(acts[-1], Ws[i], bp[i], gelu=True), None
        acts.append(hg)
        pres.append(hpre)
    hL = o.linear_fwd(acts[-1], Ws[L - 1], bp[L - 1])
    z, inv = o.l2norm_fwd(hL)
    w, winv = _last_layer_weight(v, g)
    return _last_logits(o, z, w, stats), dict(z=z, inv=inv, w=w, winv=winv, Ws=Ws, acts=acts, pres=pres)


class DinoHeadFn(torch.autograd.Function):
    """_head_forward and its backward: every weight gradient is a leaf on the side stream, the last layer's together with the
    weight-norm backward it feeds"""

    @staticmethod
    def forward(ctx, x, stats, *params):
        (logits, mx, lse), kept = _head_forward(x, params, True, stats)
        L = (len(params) - 2) // 2
        v, g = params[2 * L:]
        ctx.need_dg = g.requires_grad
        ctx.wparams, ctx.bparams, ctx.vparam = params[0:2 * L:2], params[1:2 * L:2], v
        _save_named(ctx, v=v, g=g, **kept)
        if mx is not None:
            ctx.mark_non_differentiable(mx, lse)
        return logits, mx, lse

    @staticmethod
    def backward(ctx, dlogits, _gmx=None, _glse=None):
        o = ops_module()
        s = _load_named(ctx)
        L = len(s.Ws)
        dlogits = dlogits.contiguous()
        dz = o.linear_dgrad(dlogits, s.w)
        sink = P.grad_out(ctx.vparam)

        def wlast():
            dw = o.linear_wgrad(dlogits, s.z)
            return o.weightnorm_bwd(dw, s.v, s.g, s.winv, ctx.need_dg, dv_out=sink)

        dv, dg = _side_run(wlast, dlogits, s.z)
        dh = o.l2norm_bwd(dz, s.z, s.inv)
        grads = [None] * (2 * L)
        for i in range(L - 1, -1, -1):
            grads[2 * i], grads[2 * i + 1] = _side_run(lambda dh=dh, i=i: _wgrad(dh, s.acts[i], ctx.wparams[i], want_bias=True, bias_param=ctx.bparams[i]),
                                                       dh, s.acts[i])
            if i > 0:
                dh = o.linear_dgrad(dh, s.Ws[i], gelu_preact=s.pres[i - 1])
        dx = o.linear_dgrad(dh, s.Ws[0], out_f32=True)
        _side_join()
        return (dx, None) + tuple(grads) + (_alias(dv, sink), dg)


def dino_head(x, prm, stats=None):
    """prm = (W_1, b_1, ..., W_L, b_L, weight_v, weight_g) -> (logits, row_max, row_lse): the statistics are None unless stats =
    (inv_temp, center) was given and the shape allows"""
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in prm)):
        return DinoHeadFn.apply(x, stats, *prm)
    return _head_forward(x, prm, False, stats)[0]


def dino_head_n(x, lin_params, v, g, stats=None):
    """lin_params: [(W, b), ...] of the head's Linear layers in order -> (logits, row_max | None, row_lse | None)"""
    return dino_head(x, [p for wb in lin_params for p in wb] + [v, g], stats)


class ApeAddFn(torch.autograd.Function):
    """x + absolute_pos_embed (swin_transformer.py:680-681, USE_APE): x fp32 [nB, L, C], ape fp32 [1, L, C].  Viewed as
    [1, nB, L*C] the broadcast over the images is the token-broadcast of esvit_token_mean_bwd (x_b + nB*ape / nB), and the
    parameter gradient, the sum over the images, is nB times esvit_token_mean_fwd -- no new kernel."""

    @staticmethod
    def forward(ctx, x, ape):
        o = ops_module()
        nB, L, C = x.shape
        if tuple(ape.shape) != (1, L, C):
            raise ValueError("absolute_pos_embed %s does not fit %d tokens: USE_APE supports crops of the construction resolution only "
                             "(the reference's broadcast add fails the same way)" % (tuple(ape.shape), L))
        n = torch.full((), float(nB), dtype=torch.float32, device=x.device)
        g = o.scale_inplace(ape.detach().clone().view(1, L * C), n)
        ctx.n = n
        return o.token_mean_bwd(g, x.contiguous().view(1, nB, L * C), nB).view(nB, L, C)

    @staticmethod
    def backward(ctx, gy):
        o = ops_module()
        nB, L, C = gy.shape
        dape, _ = o.token_mean_fwd(gy.contiguous().view(1, nB, L * C), dtype=torch.float32)
        return gy, o.scale_inplace(dape, ctx.n).view(1, L, C)


# ---- DINOHead(use_bn=True): Linear -> BatchNorm1d -> GELU (x2) -> Linear -> l2-normalise -> weight-normed last layer
# (vision_transformer.py:391-402, 414-418).  The Linear writes its pre-norm output d; one pass gives the batch sums, the
# [C]-sized coefficient kernel turns them into y = a d + shift and updates the running statistics, and GELU rides on the
# affine pass.  Statistics are summed over the ranks (main_esvit.py:365-379 converts every BatchNorm to SyncBatchNorm).
HEAD_BN_EPS = 1e-5
HEAD_BN_MOMENTUM = 0.1


def _head_bn_coef(o, d, st, gam, bet):
    """-> (coef [4, C], n): batch statistics in training mode, the running ones in eval mode"""
    if st.get("eval"):
        return o.bn_eval_coeffs(st["eval_mean"], st["eval_var"], gam, bet, HEAD_BN_EPS), float(d.shape[0])
    sums = o.col_sums2(d, d)
    n = float(d.shape[0] * _allreduce_stats(sums, st.get("group")))
    coef = o.bn_fwd_coeffs(sums, n, gam, bet, HEAD_BN_EPS, HEAD_BN_MOMENTUM, st.get("running_mean"), st.get("running_var"))
    if st.get("num_batches_tracked") is not None:
        st["num_batches_tracked"].add_(1)
    return coef, n


def _bn_gelu_bwd(o, dh, d, coef, gam, n, group, eval_bn):
    """dh = dL/d GELU(BN(d)) -> (dL/dd, dgamma, dbeta)"""
    du = o.col_affine2(d, coef[0], coef[1], x2=dh, act=2)     # through the GELU, at the rebuilt BN output
    red = o.bn_bwd_local(o.col_sums2(du, d), coef)            # (sum du, sum du*xhat) of this rank = (d beta, d gamma)
    dbet, dgam = red[0].clone(), red[1].clone()
    if eval_bn:
        abc = o.bn_bwd_coeffs(None, n, gam, coef)
    else:
        _allreduce_stats(red, group)
        abc = o.bn_bwd_coeffs(red, n, gam, coef)
    return o.col_affine2(du, abc[0], abc[2], d, abc[1]), dgam, dbet


class DinoHeadBnFn(torch.autograd.Function):
    """DINOHead(use_bn=True) with any number of layers (vision_transformer.py:391-402): (Linear -> BatchNorm1d -> GELU) nlayers - 1
    times, a Linear into the bottleneck, l2-normalise, the weight-normed last layer.  params = (W_1, b_1, bn_1.weight, bn_1.bias, ...,
    W_L, b_L, weight_v, weight_g); bn_states: one dict per BatchNorm.  Applied in every mode: the forward updates the running statistics
    and num_batches_tracked of a training-mode BatchNorm"""

    @staticmethod
    def forward(ctx, x, bn_states, stats, *params):
        o = ops_module()
        L = len(params) // 4                                # hidden layers carry four tensors, the last Linear and the last layer two each
        hid = [params[4 * i:4 * i + 4] for i in range(L - 1)]
        Wl, bl, v, g = params[4 * (L - 1):]
        h = o.cast_to_act(x.contiguous())
        hidden, ns = [], []
        for (Wp, b, gam, bet), st in zip(hid, bn_states):
            W = _weight(Wp)
            gam_, bet_ = gam.detach().contiguous(), bet.detach().contiguous()
            d = o.linear_fwd(h, W, b)
            coef, n = _head_bn_coef(o, d, st, gam_, bet_)
            hidden += [W, h, d, coef, gam_]
            ns.append(n)
            h = o.col_affine2(d, coef[0], coef[1], act=1)
        WL = _weight(Wl)
        hL = o.linear_fwd(h, WL, bl)
        z, inv = o.l2norm_fwd(hL)
        w, winv = _last_layer_weight(v, g)
        logits, mx, lse = _last_logits(o, z, w, stats)
        ctx.ns = ns
        ctx.group, ctx.eval_bn = (bn_states[0].get("group"), bool(bn_states[0].get("eval"))) if bn_states else (None, False)
        ctx.need_dg = g.requires_grad
        ctx.wparams = tuple(hp[0] for hp in hid) + (Wl,)
        ctx.vparam = v
        _save_named(ctx, v=v, g=g, z=z, inv=inv, w=w, winv=winv, WL=WL, hlast=h, hidden=hidden)
        if mx is not None:
            ctx.mark_non_differentiable(mx, lse)
        return logits, mx, lse

    @staticmethod
    def backward(ctx, dlogits, _gmx=None, _glse=None):
        o = ops_module()
        s = _load_named(ctx)
        L = len(ctx.wparams)
        per = [s.hidden[5 * i:5 * i + 5] for i in range(L - 1)]   # (W, input, pre-norm output, coef, gamma) of hidden layer i
        dlogits = dlogits.contiguous()
        dz = o.linear_dgrad(dlogits, s.w)
        dw = o.linear_wgrad(dlogits, s.z)
        sink = P.grad_out(ctx.vparam)
        dv, dg = o.weightnorm_bwd(dw, s.v, s.g, s.winv, ctx.need_dg, dv_out=sink)
        dh = o.l2norm_bwd(dz, s.z, s.inv)
        dWl, dbl = _wgrad(dh, s.hlast, ctx.wparams[L - 1], want_bias=True)
        dh = o.linear_dgrad(dh, s.WL)
        grads = [None] * (4 * (L - 1))
        for i in range(L - 2, -1, -1):
            W, hin, d, coef, gam = per[i]
            dd, dgam, dbet = _bn_gelu_bwd(o, dh, d, coef, gam, ctx.ns[i], ctx.group, ctx.eval_bn)
            dW, db = _wgrad(dd, hin, ctx.wparams[i], want_bias=True)
            grads[4 * i:4 * i + 4] = [dW, db, dgam, dbet]
            dh = o.linear_dgrad(dd, W, out_f32=(i == 0))
        return (dh, None, None) + tuple(grads) + (dWl, dbl, _alias(dv, sink), dg)


def dino_head_bn_n(x, bn_states, hidden, last, v, g, stats=None):
    """hidden: [(W, b, bn.weight, bn.bias), ...]; last: (W, b) of the Linear into the bottleneck -> (logits, row_max, row_lse)"""
    flat = [p for h in hidden for p in h]
    return DinoHeadBnFn.apply(x, list(bn_states), stats, *flat, *last, v, g)


def dino_head_bn(x, st1, st2, prm, stats=None):
    """prm = (W1, b1, bn1.weight, bn1.bias, W2, b2, bn2.weight, bn2.bias, W3, b3, weight_v, weight_g) -> (logits, row_max, row_lse)"""
    return DinoHeadBnFn.apply(x, [st1, st2], stats, *prm)


# ------------------------------------------------------------------------------------------------
# CvT (cvt_v4_transformer.py; BASELINE config 5).  Activations stay token-major NHWC, so the reference's
# 'b c h w <-> b h w c' rearranges around every LayerNorm do not exist here.
# ------------------------------------------------------------------------------------------------
CVT_LN_EPS = 1e-5   # get_cls_model: norm_layer=partial(LayerNorm, eps=1e-5)  (cvt_v4_transformer.py:694)
BN_EPS = 1e-5       # nn.BatchNorm2d defaults (cvt_v4_transformer.py:95)
BN_MOMENTUM = 0.1


def _conv_weight_matrix(Wp):
    """conv weight [E, Cin, k, k] -> activation-dtype GEMM operand [E, Kpad], column order (ky, kx, c), zero tail"""
    def make():
        E, Cin, k, _ = Wp.shape
        K = k * k * Cin
        Kpad = -(-K // 8) * 8
        m = torch.zeros((E, Kpad), dtype=torch.float32, device=Wp.device)
        m[:, :K] = Wp.detach().permute(0, 2, 3, 1).reshape(E, K)
        return ops_module().cast_to_act(m)
    if Wp.requires_grad or P.is_managed(Wp):
        return P.cached(Wp, "convk", make)
    return make()


def _pad_tokens(t, nB, H, W, Hp, Wp):
    """[nB*H*W, C] -> [nB*Hp*Wp, C] with zero rows/cols appended bottom/right (F.pad of cvt_v4_transformer.py:173)"""
    if Hp == H and Wp == W:
        return t
    return ops_module().pad_crop_tokens(t, nB, H, W, Hp, Wp)


def _crop_tokens(t, nB, H, W, Hp, Wp):
    if Hp == H and Wp == W:
        return t
    return ops_module().pad_crop_tokens(t, nB, Hp, Wp, H, W)


def _allreduce_stats(t, group):
    """SyncBatchNorm: batch statistics are sums over every rank's positions (main_esvit.py:365-379 converts the BN layers)"""
    import torch.distributed as dist
    if group is not False and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, group=group)
        return dist.get_world_size(group)
    return 1


class ConvEmbedFn(torch.autograd.Function):
    """ConvEmbed (cvt_v4_transformer.py:349-382): conv k x k / stride / pad as im2col + GEMM, then LayerNorm.
    src: fp32 NCHW images (first stage) or fp32 tokens [nB, H*W, Cin]; returns fp32 tokens [nB, Ho*Wo, E]."""

    @staticmethod
    def forward(ctx, src, geo, Wp, bp, g, b):
        o = ops_module()
        nchw, nB, H, W, Cin, k, stride, pad = geo[:8]
        eps = geo[8] if len(geo) > 8 else CVT_LN_EPS  # (Vision Longformer's patch embeddings: eps 1e-6)
        src = src.contiguous()
        if nchw:
            cols = o.conv_im2col(src, True, nB, H, W, Cin, k, stride, pad)
        else:
            cols = o.conv_im2col(o.gather_cast(src.view(nB * H * W, Cin), nB * H * W), False, nB, H, W, Cin, k, stride, pad)
        Wk = _conv_weight_matrix(Wp)
        y = o.linear_fwd(cols, Wk, bp, out_f32=True)
        t, _, mean, rstd = o.layernorm_fwd(y, g, b, eps, dtype=torch.float32)
        ctx.geo = geo
        ctx.wshape = tuple(Wp.shape)
        ctx.save_for_backward(cols, Wk, y, mean, rstd, g)
        Ho, Wo = o.conv_out_size(H, k, stride, pad), o.conv_out_size(W, k, stride, pad)
        return t.view(nB, Ho * Wo, -1)

    @staticmethod
    def backward(ctx, gt):
        o = ops_module()
        cols, Wk, y, mean, rstd, g = ctx.saved_tensors
        nchw, nB, H, W, Cin, k, stride, pad = ctx.geo[:8]
        E = y.shape[1]
        dy, dg, db = o.layernorm_bwd(gt.contiguous().view(-1, E), y, mean, rstd, g)
        dyb = o.gather_cast(dy, dy.shape[0])
        dWk, dbp = o.linear_wgrad(dyb, cols, want_bias=True)
        K = k * k * Cin
        dWp = dWk[:, :K].reshape(E, k, k, Cin).permute(0, 3, 1, 2).contiguous()
        dsrc = None
        if not nchw and ctx.needs_input_grad[0]:
            dcols = o.linear_dgrad(dyb, Wk)
            dsrc = o.conv_col2im(dcols, nB, H, W, Cin, k, stride, pad).view(nB, H * W, Cin)
        return dsrc, None, dWp, dbp, dg, db


class ConvBnReluFn(torch.autograd.Function):
    """one unit of the residual stem (cvt_v4_transformer.py:385-430): Conv2d(3x3, no bias) -> BatchNorm2d -> ReLU as im2col + GEMM,
    per-channel sums, one affine + ReLU pass.  src: fp32 NCHW images or activation-dtype tokens [nB*H*W, Cin]; returns activation-dtype
    tokens [nB*Ho*Wo, E].  BatchNorm as in CvtAttnFn (batch statistics summed over the ranks in train mode, running statistics in eval)."""

    @staticmethod
    def forward(ctx, src, geo, bn_state, Wp, bn_g, bn_b):
        o = ops_module()
        nchw, nB, H, W, Cin, k, stride, pad = geo
        src = src.contiguous()
        cols = o.conv_im2col(src if nchw else src.view(nB * H * W, Cin), nchw, nB, H, W, Cin, k, stride, pad)
        Wk = _conv_weight_matrix(Wp)
        d = o.linear_fwd(cols, Wk, None)
        rows = d.shape[0]
        eval_bn = bool(bn_state.get("eval"))
        gam, bet = bn_g.detach().contiguous(), bn_b.detach().contiguous()
        if eval_bn:
            n = float(rows)
            coef = o.bn_eval_coeffs(bn_state["eval_mean"], bn_state["eval_var"], gam, bet, BN_EPS)
        else:
            sums = o.col_sums2(d, d)
            n = float(rows * _allreduce_stats(sums, bn_state.get("group")))
            coef = o.bn_fwd_coeffs(sums, n, gam, bet, BN_EPS, BN_MOMENTUM, bn_state.get("running_mean"), bn_state.get("running_var"))
            if bn_state.get("num_batches_tracked") is not None:
                bn_state["num_batches_tracked"].add_(1)
        y = o.col_affine2(d, coef[0], coef[1], act=3)
        ctx.geo, ctx.n, ctx.eval_bn, ctx.group, ctx.wshape = geo, n, eval_bn, bn_state.get("group"), tuple(Wp.shape)
        ctx.save_for_backward(cols, Wk, d, coef, gam)
        return y

    @staticmethod
    def backward(ctx, gy):
        o = ops_module()
        cols, Wk, d, coef, gam = ctx.saved_tensors
        nchw, nB, H, W, Cin, k, stride, pad = ctx.geo
        E = d.shape[1]
        gy = gy.contiguous()
        if gy.dtype != d.dtype:
            gy = o.cast_to_act(gy.float())
        dz = o.col_affine2(d, coef[0], coef[1], gy, act=4)        # through the ReLU, its argument rebuilt from the conv output
        red = o.bn_bwd_local(o.col_sums2(dz, d), coef)            # (d beta, d gamma) of this rank
        dbet, dgam = red[0].clone(), red[1].clone()
        if ctx.eval_bn:
            abc = o.bn_bwd_coeffs(None, ctx.n, gam, coef)
        else:
            _allreduce_stats(red, ctx.group)
            abc = o.bn_bwd_coeffs(red, ctx.n, gam, coef)
        dd = o.col_affine2(dz, abc[0], abc[2], d, abc[1])
        dWk = o.linear_wgrad(dd, cols)
        K = k * k * Cin
        dWp = dWk[:, :K].reshape(E, k, k, Cin).permute(0, 3, 1, 2).contiguous()
        dsrc = None
        if not nchw and ctx.needs_input_grad[0]:
            dsrc = o.conv_col2im(o.linear_dgrad(dd, Wk), nB, H, W, Cin, k, stride, pad)
            dsrc = o.gather_cast(dsrc, dsrc.shape[0])
        return dsrc, None, None, dWp, dgam, dbet


class CvtAttnFn(torch.autograd.Function):
    """x + DropPath(Attention(LayerNorm(x)))  (cvt_v4_transformer.py:331-336, 49-58, 108-220): LN -> zero-pad the grid to a
    multiple of the window -> depthwise 3x3 -> BatchNorm (batch statistics, synchronised across ranks) -> 1x1 to q|k|v ->
    windowed attention (w = min(window, H, W), scale = dim ** -0.5) -> crop -> 1x1 proj.  Optional (s1_rpe.yaml / s1_shift.yaml):
    a relative-position bias table (`table_p`, `index`) and the shifted-window mask of a half-window shift on the UNROLLED map
    (`shift`: cvt_v4_transformer.py:291-329 builds the Swin mask, :332 hands it to every block, nothing rolls)."""

    @staticmethod
    def forward(ctx, x, H, W, nH, window, dp, bn_state, g1, b1, dw_w, bn_g, bn_b, pw_Wp, pw_b, proj_Wp, proj_b, table_p=None, index=None,
                shift=False):
        o = ops_module()
        nB, L, C = x.shape
        x = x.contiguous()
        x2d = x.view(nB * L, C)
        w = min(window, H, W)
        if (table_p is not None or shift) and w != window:
            # the reference adds a [window^2, window^2] bias / mask to [w^2, w^2] scores here and fails on the shapes
            raise RuntimeError("CvT relative-position bias / shift mask on a %dx%d map: smaller than the %dx%d window" % (H, W, window, window))
        if shift and (H % w or W % w):
            # the reference's masked branch overwrites its map height with the head count (cvt_v4_transformer.py:201) and then crops
            # the padded output with it: only maps that need no padding come through
            raise RuntimeError("CvT shift mask on a %dx%d map: not a multiple of the %dx%d window" % (H, W, window, window))
        Hp, Wp = -(-H // w) * w, -(-W // w) * w
        xn, _, mean1, rstd1 = o.layernorm_fwd(x2d, g1, b1, CVT_LN_EPS)
        xp = _pad_tokens(xn, nB, H, W, Hp, Wp)
        dw9 = dw_w.detach().reshape(C, 9).contiguous()
        d = o.dwconv3x3(xp, dw9, nB, Hp, Wp)
        rows = nB * Hp * Wp
        eval_bn = bool(bn_state.get("eval"))
        gam, bet = bn_g.detach().contiguous(), bn_b.detach().contiguous()
        if eval_bn:  # inference: the running statistics (nn.BatchNorm2d in eval mode)
            n = float(rows)
            coef = o.bn_eval_coeffs(bn_state["eval_mean"], bn_state["eval_var"], gam, bet, BN_EPS)
        else:        # BatchNorm2d, training statistics over every position of the (padded) map on every rank
            sums = o.col_sums2(d, d)
            n = float(rows * _allreduce_stats(sums, bn_state.get("group")))  # every rank runs the same per-GPU batch
            coef = o.bn_fwd_coeffs(sums, n, gam, bet, BN_EPS, BN_MOMENTUM, bn_state.get("running_mean"), bn_state.get("running_var"))
            if bn_state.get("num_batches_tracked") is not None:
                bn_state["num_batches_tracked"].add_(1)
        bnout = o.col_affine2(d, coef[0], coef[1])
        Wpw, Wproj = _weight(pw_Wp, (3 * C, C)), _weight(proj_Wp, (C, C))
        qkv = o.linear_fwd(bnout, Wpw, pw_b)
        geom = geometry(Hp, Wp, w, 0, x.device)
        table = _zero_table(w, nH, x.device) if table_p is None else table_p.detach()
        regions = geometry(Hp, Wp, w, w // 2, x.device).region_ids if shift else None
        scale = float(C) ** -0.5
        ao, lse = o.window_attn_fwd(qkv, pw_b, geom.win2tok, Hp * Wp, table, w, regions, geom.nW, geom.N, nH, scale)
        aoc = _crop_tokens(ao, nB, H, W, Hp, Wp)
        x1 = o.linear_fwd(aoc, Wproj, proj_b, residual=x2d, rowscale=dp, rows_per_sample=L, out_f32=True)
        ctx.meta = (H, W, Hp, Wp, w, nH, scale, dp, bn_state.get("group"), eval_bn, table_p is not None, shift)
        ctx.n = n
        ctx.save_for_backward(x, mean1, rstd1, g1, xp, dw9, d, coef, gam, bnout, Wpw, pw_b, qkv, ao, aoc, Wproj, lse, table, index)
        return x1.view(nB, L, C)

    @staticmethod
    def backward(ctx, gy):
        o = ops_module()
        x, mean1, rstd1, g1, xp, dw9, d, coef, gam, bnout, Wpw, pw_b, qkv, ao, aoc, Wproj, lse, table, index = ctx.saved_tensors
        n = ctx.n
        H, W, Hp, Wp, w, nH, scale, dp, group, eval_bn, has_table, shift = ctx.meta
        nB, L, C = x.shape
        M = nB * L
        gy = gy.contiguous().view(M, C)
        dyb = o.gather_cast(gy, M, rowscale=dp, rows_per_sample=L)
        dWproj, dbproj = _side_run(lambda: o.linear_wgrad(dyb, aoc, want_bias=True), dyb, aoc)
        dao = _pad_tokens(o.linear_dgrad(dyb, Wproj), nB, H, W, Hp, Wp)
        geom = geometry(Hp, Wp, w, 0, x.device)
        regions = geometry(Hp, Wp, w, w // 2, x.device).region_ids if shift else None
        dqkv, dbias_ws, _ = o.window_attn_bwd(qkv, pw_b, geom.win2tok, Hp * Wp, dao, ao, lse, table, w, regions, geom.nW, geom.N, nH, scale,
                                              **({} if has_table else _no_dbias(o, geom.N, C // nH)))
        dtable = o.relpos_bias_bwd(dbias_ws, index, geom.N, table.shape[0], **_relpos_kw(o)) if has_table else None
        dWpw, dbpw = _side_run(lambda: o.linear_wgrad(dqkv, bnout, want_bias=True), dqkv, bnout)
        dbn = o.linear_dgrad(dqkv, Wpw)
        # BatchNorm backward: d(d) = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)), xhat = (d - mean) rstd
        red = o.bn_bwd_local(o.col_sums2(dbn, d), coef)   # (sum dy, sum dy*xhat) of this rank = (d beta, d gamma)
        dbet, dgam = red[0].clone(), red[1].clone()
        if eval_bn:  # fixed statistics: the normalisation is a per-channel affine map, no batch terms in its gradient
            abc = o.bn_bwd_coeffs(None, n, gam, coef)
        else:
            _allreduce_stats(red, group)
            abc = o.bn_bwd_coeffs(red, n, gam, coef)
        dd = o.col_affine2(dbn, abc[0], abc[2], d, abc[1])
        ddw = _side_run(lambda: o.dwconv3x3_wgrad(xp, dd, nB, Hp, Wp), xp, dd).view(C, 1, 3, 3)
        dxn = _crop_tokens(o.dwconv3x3(dd, dw9, nB, Hp, Wp, flip=True), nB, H, W, Hp, Wp)
        gx, dg1, db1 = o.layernorm_bwd(dxn, x.view(M, C), mean1, rstd1, g1, g_in=gy)
        _side_join()
        return (gx.view(nB, L, C), None, None, None, None, None, None, dg1, db1, ddw, dgam, dbet, dWpw.view(3 * C, C, 1, 1), dbpw,
                dWproj.view(C, C, 1, 1), dbproj, dtable, None, None)


_ZTAB = {}


def _zero_table(w, nH, device):
    key = (w, nH, str(device))
    t = _ZTAB.get(key)
    if t is None:
        t = torch.zeros(((2 * w - 1) ** 2, nH), dtype=torch.float32, device=device)
        _ZTAB[key] = t
    return t


def _cvt_ffn_fwd(ctx, X, rowscale, rows_per_sample, prm):
    """X fp32 [M, C] -> X + DropPath(FeedForward(LayerNorm(X))); keeps on ctx what _cvt_ffn_bwd reads"""
    g2, b2, W1p, bf1, W2p, bf2 = prm
    C, Hd = X.shape[1], W1p.shape[0]
    W1, W2 = _weight(W1p, (Hd, C)), _weight(W2p, (C, Hd))
    y, (mean, rstd, h, a1, a1g) = _mlp_fwd(ops_module(), X, (g2, b2, bf1, bf2), W1, W2, CVT_LN_EPS, rowscale, rows_per_sample, True, quick=True)
    ctx.rowscale, ctx.rows_per_sample, ctx.params = rowscale, rows_per_sample, prm
    ctx.save_for_backward(X, mean, rstd, g2, h, a1, a1g, W1, W2)
    return y


def _cvt_ffn_bwd(ctx, gy):
    """gy fp32 [M, C] -> (gx, d norm.weight, d norm.bias, d fc1.weight, d fc1.bias, d fc2.weight, d fc2.bias)"""
    o = ops_module()
    X, mean, rstd, g2, h, a1, a1g, W1, W2 = ctx.saved_tensors
    g2_p, b2_p, W1p, bf1_p, W2p, bf2_p = ctx.params
    M, C = X.shape
    Hd = W1.shape[0]
    dyb = o.gather_cast(gy, M, rowscale=ctx.rowscale, rows_per_sample=ctx.rows_per_sample)
    dh, dW1, dbf1, dW2, dbf2 = _mlp_bwd(o, dyb, h, a1, a1g, W1, W2, (W1p, bf1_p, W2p, bf2_p), quick=True, shapes2d=((Hd, C), (C, Hd)))
    ln2 = _ln_sinks(g2_p, b2_p)
    gx, dg2, db2 = o.layernorm_bwd(dh, X, mean, rstd, g2, g_in=gy, gb_out=ln2)
    _side_join()
    return gx, _alias(dg2, ln2), _alias(db2, ln2), dW1.view(Hd, C, 1, 1), dbf1, dW2.view(C, Hd, 1, 1), dbf2


class CvtFfnFn(torch.autograd.Function):
    """x + DropPath(FeedForward(LayerNorm(x)))  (cvt_v4_transformer.py:62-72): 1x1 conv -> QuickGELU -> 1x1 conv.  x fp32 [nB, L, C];
    dp: None or the DropPath scale per sample [nB]"""

    @staticmethod
    def forward(ctx, x, dp, g2, b2, W1p, bf1, W2p, bf2):
        nB, L, C = x.shape
        return _cvt_ffn_fwd(ctx, x.contiguous().view(nB * L, C), dp, L, (g2, b2, W1p, bf1, W2p, bf2)).view(nB, L, C)

    @staticmethod
    def backward(ctx, gy):
        gx, *grads = _cvt_ffn_bwd(ctx, gy.contiguous().view(-1, gy.shape[-1]))
        return (gx.view(gy.shape), None) + tuple(grads)


# ---- ragged multi-crop CvT: every resolution group of a step through ONE set of LayerNorm / GEMM launches -----------------------------
# LayerNorm, the 1x1 convolutions (GEMMs) and the residual adds are row-wise, so the token rows of all groups run through them together
# and every parameter receives ONE gradient contribution, written into its bucket slot.  What depends on the grid runs per group: the
# zero-pad / crop around the windows, the depthwise 3x3, the window attention -- and BatchNorm, which keeps the reference's semantics: the
# reference calls the backbone once per group (cvt_v4_transformer.py:625-628), so each group is normalised with ITS OWN batch statistics
# and the running statistics take one momentum update per group, IN GROUP ORDER.  The pad / crop, depthwise and BatchNorm kernels of all
# groups are one launch each where the ops module has the grouped entries (include/esvit_hip.h, "GROUPED MODE"); an ops module without
# them (the CPU restatement) runs the plain calls group by group.
CVT_MAX_GROUPS = 4  # ESVIT_MAX_GRID_GROUPS


def _g_pad_crop(o, srcs, geos, outs):
    """pad_crop_tokens per group (geos: (nB, Hs, Ws, Hd, Wd)) into `outs`"""
    if not srcs:
        return
    if hasattr(o, "pad_crop_tokens_grouped"):
        o.pad_crop_tokens_grouped(srcs, geos, outs=outs)
        return
    for s, g, d in zip(srcs, geos, outs):
        d.copy_(o.pad_crop_tokens(s, *g))


def _g_dwconv(o, xs, w9, geos, flip, outs):
    if hasattr(o, "dwconv3x3_grouped"):
        o.dwconv3x3_grouped(xs, w9, geos, flip=flip, outs=outs)
        return
    for x, (nB, H, W), d in zip(xs, geos, outs):
        d.copy_(o.dwconv3x3(x, w9, nB, H, W, flip=flip))


def _g_col_sums2(o, a_list, b_list):
    """-> fp32 [G, 2, C], row g with the bits of col_sums2(a_list[g], b_list[g])"""
    if hasattr(o, "col_sums2_grouped"):
        return o.col_sums2_grouped(a_list, b_list)
    return torch.stack([o.col_sums2(a, b) for a, b in zip(a_list, b_list)], 0)


def _g_col_affine2(o, x1s, a1s, a3s, x2s, a2s, outs):
    if hasattr(o, "col_affine2_grouped"):
        o.col_affine2_grouped(x1s, a1s, a3s, x2s, a2s, outs=outs)
        return
    for i, (x1, d) in enumerate(zip(x1s, outs)):
        d.copy_(o.col_affine2(x1, a1s[i], a3s[i], None if x2s is None else x2s[i], None if a2s is None else a2s[i]))


def _cvt_group_geometry(segs, window, has_table, shift):
    """segs: (row0, nB, H, W) -> per group (row0, row1, pad0, pad1, nB, H, W, Hp, Wp, w); the refusals of CvtAttnFn.forward, per group"""
    out, p0 = [], 0
    for (r0, nB, H, W) in segs:
        w = min(window, H, W)
        if (has_table or shift) and w != window:
            raise RuntimeError("CvT relative-position bias / shift mask on a %dx%d map: smaller than the %dx%d window" % (H, W, window, window))
        if shift and (H % w or W % w):
            raise RuntimeError("CvT shift mask on a %dx%d map: not a multiple of the %dx%d window" % (H, W, window, window))
        Hp, Wp = -(-H // w) * w, -(-W // w) * w
        out.append((r0, r0 + nB * H * W, p0, p0 + nB * Hp * Wp, nB, H, W, Hp, Wp, w))
        p0 += nB * Hp * Wp
    return out


class CvtAttnMultiFn(torch.autograd.Function):
    """CvtAttnFn over the token rows of several resolution groups.  X fp32 [M, C] (group after group), segs: tuple of (row0, nB, H, W),
    dp_rows: None or the per-row DropPath scale [M].  A group whose grid needs no padding is never copied: its depthwise convolution reads
    the LayerNorm output in place and its attention writes into the rows of the projection's operand."""

    @staticmethod
    def forward(ctx, X, segs, nH, window, dp_rows, bn_state, g1, b1, dw_w, bn_g, bn_b, pw_Wp, pw_b, proj_Wp, proj_b, table_p=None, index=None,
                shift=False):
        o = ops_module()
        X = X.contiguous()
        M, C = X.shape
        geo = _cvt_group_geometry(segs, window, table_p is not None, shift)
        G, Mp, dev = len(geo), geo[-1][3], X.device
        xn, _, mean1, rstd1 = o.layernorm_fwd(X, g1, b1, CVT_LN_EPS)
        dt = xn.dtype
        padded = [i for i, q in enumerate(geo) if (q[7], q[8]) != (q[5], q[6])]
        xps = [xn[q[0]:q[1]] for q in geo]
        for i in padded:
            xps[i] = torch.empty((geo[i][3] - geo[i][2], C), dtype=dt, device=dev)
        _g_pad_crop(o, [xn[geo[i][0]:geo[i][1]] for i in padded], [(geo[i][4], geo[i][5], geo[i][6], geo[i][7], geo[i][8]) for i in padded],
                    [xps[i] for i in padded])
        dw9 = dw_w.detach().reshape(C, 9).contiguous()
        d = torch.empty((Mp, C), dtype=dt, device=dev)
        ds = [d[q[2]:q[3]] for q in geo]
        pgeo = [(q[4], q[7], q[8]) for q in geo]
        _g_dwconv(o, xps, dw9, pgeo, False, ds)
        eval_bn = bool(bn_state.get("eval"))
        gam, bet = bn_g.detach().contiguous(), bn_b.detach().contiguous()
        if eval_bn:  # the running statistics for every group: one coefficient vector
            ns = [float(q[3] - q[2]) for q in geo]
            coefs = [o.bn_eval_coeffs(bn_state["eval_mean"], bn_state["eval_var"], gam, bet, BN_EPS)] * G
        else:        # every group with its own batch statistics; ONE all-reduce of the stacked sums; running statistics in group order
            sums = _g_col_sums2(o, ds, ds)
            world = _allreduce_stats(sums, bn_state.get("group"))
            ns = [float((q[3] - q[2]) * world) for q in geo]
            coefs = [o.bn_fwd_coeffs(sums[i], ns[i], gam, bet, BN_EPS, BN_MOMENTUM, bn_state.get("running_mean"), bn_state.get("running_var"))
                     for i in range(G)]
            if bn_state.get("num_batches_tracked") is not None:
                bn_state["num_batches_tracked"].add_(G)
        bnout = torch.empty_like(d)
        _g_col_affine2(o, ds, [c[0] for c in coefs], [c[1] for c in coefs], None, None, [bnout[q[2]:q[3]] for q in geo])
        Wpw, Wproj = _weight(pw_Wp, (3 * C, C)), _weight(proj_Wp, (C, C))
        qkv = o.linear_fwd(bnout, Wpw, pw_b)
        scale = float(C) ** -0.5
        aoc = torch.empty((M, C), dtype=qkv.dtype, device=dev)
        aos, lses, tables = [], [], []
        for i, (r0, r1, p0, p1, nB, H, W, Hp, Wp, w) in enumerate(geo):
            geom = geometry(Hp, Wp, w, 0, dev)
            table = _zero_table(w, nH, dev) if table_p is None else table_p.detach()
            regions = geometry(Hp, Wp, w, w // 2, dev).region_ids if shift else None
            ao, lse = o.window_attn_fwd(qkv[p0:p1], pw_b, geom.win2tok, Hp * Wp, table, w, regions, geom.nW, geom.N, nH, scale,
                                        out=None if i in padded else aoc[r0:r1])
            aos.append(ao)
            lses.append(lse)
            tables.append(table)
        _g_pad_crop(o, [aos[i] for i in padded], [(geo[i][4], geo[i][7], geo[i][8], geo[i][5], geo[i][6]) for i in padded],
                    [aoc[geo[i][0]:geo[i][1]] for i in padded])
        x1 = o.linear_fwd(aoc, Wproj, proj_b, residual=X, rowscale=dp_rows, rows_per_sample=1, out_f32=True)
        ctx.geo, ctx.padded, ctx.meta = geo, padded, (nH, scale, dp_rows, bn_state.get("group"), eval_bn, table_p is not None, shift)
        ctx.ns, ctx.has_lse = ns, [l is not None for l in lses]
        ctx.params = (g1, b1, pw_Wp, pw_b, proj_Wp, proj_b, table_p)
        ucoefs = coefs[:1] if eval_bn else coefs
        ctx.ncoef = len(ucoefs)
        ctx.save_for_backward(X, mean1, rstd1, g1, dw9, d, gam, bnout, Wpw, pw_b, qkv, aoc, Wproj, index, *xps, *aos, *tables, *ucoefs,
                              *[l for l in lses if l is not None])
        return x1

    @staticmethod
    def backward(ctx, gy):
        o = ops_module()
        t = ctx.saved_tensors
        X, mean1, rstd1, g1, dw9, d, gam, bnout, Wpw, pw_b, qkv, aoc, Wproj, index = t[:14]
        geo, padded = ctx.geo, ctx.padded
        G = len(geo)
        xps, aos, tables = t[14:14 + G], t[14 + G:14 + 2 * G], t[14 + 2 * G:14 + 3 * G]
        coefs = list(t[14 + 3 * G:14 + 3 * G + ctx.ncoef])
        rest = list(t[14 + 3 * G + ctx.ncoef:])
        lses = [rest.pop(0) if h else None for h in ctx.has_lse]
        nH, scale, dp_rows, group, eval_bn, has_table, shift = ctx.meta
        if eval_bn:
            coefs = coefs * G
        g1_p, b1_p, pw_Wp, pw_b_p, proj_Wp, proj_b_p, table_p = ctx.params
        M, C = X.shape
        Mp, dev = geo[-1][3], X.device
        gy = gy.contiguous()
        dyb = o.gather_cast(gy, M, rowscale=dp_rows, rows_per_sample=1)
        dWproj, dbproj = _side_run(lambda: _wgrad(dyb, aoc, proj_Wp, (C, C), want_bias=True, bias_param=proj_b_p), dyb, aoc)
        daoc = o.linear_dgrad(dyb, Wproj)
        daos = [daoc[q[0]:q[1]] for q in geo]
        for i in padded:
            daos[i] = torch.empty((geo[i][3] - geo[i][2], C), dtype=daoc.dtype, device=dev)
        _g_pad_crop(o, [daoc[geo[i][0]:geo[i][1]] for i in padded], [(geo[i][4], geo[i][5], geo[i][6], geo[i][7], geo[i][8]) for i in padded],
                    [daos[i] for i in padded])
        dqkv = torch.empty_like(qkv)
        dtable, tsink = None, P.grad_out(table_p) if has_table else None
        for i, (r0, r1, p0, p1, nB, H, W, Hp, Wp, w) in enumerate(geo):
            geom = geometry(Hp, Wp, w, 0, dev)
            regions = geometry(Hp, Wp, w, w // 2, dev).region_ids if shift else None
            _, dbias_ws, _ = o.window_attn_bwd(qkv[p0:p1], pw_b, geom.win2tok, Hp * Wp, daos[i], aos[i], lses[i], tables[i], w, regions, geom.nW, geom.N,
                                               nH, scale, dqkv_out=dqkv[p0:p1], **({} if has_table else _no_dbias(o, geom.N, C // nH)))
            if has_table:  # the first group writes the table gradient (its bucket slot when there is one), later groups add to it
                if i == 0:
                    dtable = o.relpos_bias_bwd(dbias_ws, index, geom.N, tables[i].shape[0], out=tsink, accumulate=False if tsink is not None else None,
                                                  **_relpos_kw(o))
                else:
                    o.relpos_bias_bwd(dbias_ws, index, geom.N, tables[i].shape[0], out=dtable, accumulate=True, **_relpos_kw(o))
        if has_table:
            dtable = _alias(dtable, tsink)
        dWpw, dbpw = _side_run(lambda: _wgrad(dqkv, bnout, pw_Wp, (3 * C, C), want_bias=True, bias_param=pw_b_p), dqkv, bnout)
        dbn = o.linear_dgrad(dqkv, Wpw)
        # BatchNorm backward per group (CvtAttnFn.backward); d gamma / d beta: the sum of the groups' local reductions
        ds, dbns = [d[q[2]:q[3]] for q in geo], [dbn[q[2]:q[3]] for q in geo]
        sums = _g_col_sums2(o, dbns, ds)
        red = torch.stack([o.bn_bwd_local(sums[i], coefs[i]) for i in range(G)], 0)  # [G, 2, C]
        dgb = red.sum(0)
        if eval_bn:
            abcs = [o.bn_bwd_coeffs(None, ctx.ns[i], gam, coefs[i]) for i in range(G)]
        else:
            _allreduce_stats(red, group)  # ONE all-reduce for all groups
            abcs = [o.bn_bwd_coeffs(red[i], ctx.ns[i], gam, coefs[i]) for i in range(G)]
        dd = torch.empty_like(d)
        dds = [dd[q[2]:q[3]] for q in geo]
        _g_col_affine2(o, dbns, [a[0] for a in abcs], [a[2] for a in abcs], ds, [a[1] for a in abcs], dds)
        pgeo = [(q[4], q[7], q[8]) for q in geo]

        def dw_wgrad():
            acc = o.dwconv3x3_wgrad(xps[0], dds[0], *pgeo[0])
            for i in range(1, G):
                acc = acc.add_(o.dwconv3x3_wgrad(xps[i], dds[i], *pgeo[i]))
            return acc

        ddw = _side_run(dw_wgrad, dd, *xps).view(C, 1, 3, 3)
        dxn = torch.empty((M, C), dtype=dd.dtype, device=dev)
        dxps = [dxn[q[0]:q[1]] for q in geo]
        for i in padded:
            dxps[i] = torch.empty((geo[i][3] - geo[i][2], C), dtype=dd.dtype, device=dev)
        _g_dwconv(o, dds, dw9, pgeo, True, dxps)
        _g_pad_crop(o, [dxps[i] for i in padded], [(geo[i][4], geo[i][7], geo[i][8], geo[i][5], geo[i][6]) for i in padded],
                    [dxn[geo[i][0]:geo[i][1]] for i in padded])
        ln1 = _ln_sinks(g1_p, b1_p)
        gx, dg1, db1 = o.layernorm_bwd(dxn, X, mean1, rstd1, g1, g_in=gy, gb_out=ln1)
        _side_join()
        return (gx, None, None, None, None, None, _alias(dg1, ln1), _alias(db1, ln1), ddw, dgb[1], dgb[0], dWpw.view(3 * C, C, 1, 1), dbpw,
                dWproj.view(C, C, 1, 1), dbproj, dtable, None, None)


class CvtFfnMultiFn(torch.autograd.Function):
    """CvtFfnFn over the token rows of all groups: X fp32 [M, C]; dp_rows: None or the per-row DropPath scale [M]"""

    @staticmethod
    def forward(ctx, X, dp_rows, g2, b2, W1p, bf1, W2p, bf2):
        return _cvt_ffn_fwd(ctx, X.contiguous(), dp_rows, 1, (g2, b2, W1p, bf1, W2p, bf2))

    @staticmethod
    def backward(ctx, gy):
        gx, *grads = _cvt_ffn_bwd(ctx, gy.contiguous())
        return (gx, None) + tuple(grads)


def cvt_block_multi(X, segs, nH, window, dp_rows, bn_state, attn_prm, ffn_prm, table_p=None, index=None, shift=False):
    """one CvT block (attention + feed-forward) over the token rows of several resolution groups; X fp32 [M, C].
    attn_prm = (norm.w, norm.b, dw.w, bn.w, bn.b, pw.w, pw.b, proj.w, proj.b), ffn_prm = (norm.w, norm.b, fc1.w, fc1.b, fc2.w, fc2.b);
    dp_rows: None or (attention branch [M], feed-forward branch [M])"""
    dp1, dp2 = (None, None) if dp_rows is None else dp_rows
    X = CvtAttnMultiFn.apply(X, segs, nH, window, dp1, bn_state, *attn_prm, table_p, index, shift)
    return CvtFfnMultiFn.apply(X, dp2, *ffn_prm)


class ConvEmbedMultiFn(torch.autograd.Function):
    """ConvEmbed of several resolution groups: im2col per piece into ONE column matrix, one projection GEMM + LayerNorm over all rows (one
    gradient contribution per parameter), col2im per group.  geo = (nchw, Cin, k, stride, pad, pieces), pieces: (nB, H, W) per piece.
    nchw: srcs = the fp32 image batches, one per piece (read where they lie); else srcs = (X,) fp32 token rows [M, Cin], piece after piece.
    -> fp32 token rows [sum nB Ho Wo, E]"""

    @staticmethod
    def forward(ctx, geo, Wp, bp, g, b, *srcs):
        o = ops_module()
        nchw, Cin, k, stride, pad, pieces = geo
        outs = [(nB, o.conv_out_size(H, k, stride, pad), o.conv_out_size(W, k, stride, pad)) for (nB, H, W) in pieces]
        rows = [nB * Ho * Wo for (nB, Ho, Wo) in outs]
        Wk = _conv_weight_matrix(Wp)
        cols = torch.empty((sum(rows), Wk.shape[1]), dtype=Wk.dtype, device=srcs[0].device)
        if not nchw:
            X = srcs[0].contiguous()
            xa = o.gather_cast(X, X.shape[0])
        r0 = q0 = 0
        for i, (nB, H, W) in enumerate(pieces):
            src = srcs[i].contiguous() if nchw else xa[q0:q0 + nB * H * W]
            if getattr(o, "IM2COL_OUT", False):
                o.conv_im2col(src, nchw, nB, H, W, Cin, k, stride, pad, out=cols[r0:r0 + rows[i]])
            else:
                cols[r0:r0 + rows[i]].copy_(o.conv_im2col(src, nchw, nB, H, W, Cin, k, stride, pad))
            r0 += rows[i]
            q0 += nB * H * W
        y = o.linear_fwd(cols, Wk, bp, out_f32=True)
        t, _, mean, rstd = o.layernorm_fwd(y, g, b, CVT_LN_EPS, dtype=torch.float32)
        ctx.geo, ctx.rows, ctx.nsrc = geo, rows, len(srcs)
        ctx.params = (Wp, bp, g, b)
        ctx.save_for_backward(cols, Wk, y, mean, rstd, g)
        return t

    @staticmethod
    def backward(ctx, gt):
        o = ops_module()
        cols, Wk, y, mean, rstd, g = ctx.saved_tensors
        nchw, Cin, k, stride, pad, pieces = ctx.geo
        Wp, bp_p, g_p, b_p = ctx.params
        E = y.shape[1]
        ln = _ln_sinks(g_p, b_p)
        dy, dg, db = o.layernorm_bwd(gt.contiguous(), y, mean, rstd, g, gb_out=ln)
        dyb = o.gather_cast(dy, dy.shape[0])
        bsink = P.grad_out(bp_p)
        dWk, dbp = _side_run(lambda: o.linear_wgrad(dyb, cols, want_bias=True, db_out=bsink), dyb, cols)
        dX = None
        if not nchw and ctx.needs_input_grad[5]:
            dcols = o.linear_dgrad(dyb, Wk)
            dX = torch.empty((sum(nB * H * W for (nB, H, W) in pieces), Cin), dtype=torch.float32, device=dcols.device)
            r0 = q0 = 0
            for i, (nB, H, W) in enumerate(pieces):
                dst = dX[q0:q0 + nB * H * W]
                if getattr(o, "IM2COL_OUT", False):
                    o.conv_col2im(dcols[r0:r0 + ctx.rows[i]], nB, H, W, Cin, k, stride, pad, out=dst)
                else:
                    dst.copy_(o.conv_col2im(dcols[r0:r0 + ctx.rows[i]], nB, H, W, Cin, k, stride, pad))
                r0 += ctx.rows[i]
                q0 += nB * H * W
        _side_join()
        # the GEMM's column order is (ky, kx, c): the parameter's layout is one permuting copy away, written into its bucket slot if there is one
        K = k * k * Cin
        wsink = P.grad_out(Wp)
        src = dWk[:, :K].reshape(E, k, k, Cin).permute(0, 3, 1, 2)
        dWp = _alias(wsink.copy_(src), wsink) if wsink is not None else src.contiguous()
        return (None, dWp, _alias(dbp, bsink), _alias(dg, ln), _alias(db, ln)) + ((dX,) if not nchw else (None,) * ctx.nsrc)


# ------------------------------------------------------------------------------------------------
# monolithic ViT (models/vision_transformer.py:96-381): patch embedding without a norm, blocks with global attention
# ------------------------------------------------------------------------------------------------
class VitPatchEmbedFn(torch.autograd.Function):
    """PatchEmbed (vision_transformer.py:121-139): Conv2d(k = stride = patch) as im2col + GEMM, fp32 tokens out.  img [nB, 3, H, W], both
    sides multiples of the patch size -> [nB, (H / patch) * (W / patch), E], patch rows first.  An ops module whose patch_im2col takes
    square images only (the CPU restatement) gets the columns of a rectangle from F.unfold, which has the same (c, ph, pw) order."""

    @staticmethod
    def forward(ctx, img, Wp, bp, patch):
        o = ops_module()
        E = Wp.shape[0]
        Kc = Wp.shape[1] * patch * patch
        nB, _, H, Wd = img.shape
        if H == Wd or getattr(o, "PATCH_IM2COL_RECT", False):
            cols = o.patch_im2col(img.contiguous(), patch, Kc)
        else:
            if H % patch or Wd % patch:
                raise ValueError("VitPatchEmbedFn: image %dx%d is not made of whole %d-pixel patches" % (H, Wd, patch))
            cols = o.cast_to_act(torch.nn.functional.unfold(img.float(), patch, stride=patch).transpose(1, 2).reshape(-1, Kc).contiguous())
        y = o.linear_fwd(cols, _weight(Wp, (E, Kc)), bp, out_f32=True)
        ctx.save_for_backward(cols)
        ctx.wparam, ctx.bparam, ctx.wshape = Wp, bp, tuple(Wp.shape)
        return y.view(nB, (H // patch) * (Wd // patch), E)

    @staticmethod
    def backward(ctx, gx):
        o = ops_module()
        (cols,) = ctx.saved_tensors
        M = cols.shape[0]
        dyb = o.gather_cast(gx.contiguous().view(M, -1), M)
        # (no bucket slots here: the embedding runs once per resolution group, so its parameters receive two contributions per
        # backward -- autograd sums them and the reducer's hook packs the sum)
        dW, dbp = o.linear_wgrad(dyb, cols, want_bias=True)
        return None, dW.view(ctx.wshape), dbp, None


# position embedding on an (h, w) patch grid (vision_transformer.py:296-312)
_VIT_POS = {}
_CUBIC_A = -0.75


def vit_pos_axis_matrix(S, n_base, g, sf=None):
    """one axis of torch's F.interpolate(mode="bicubic", scale_factor=g / sqrt(n_base)) from S lines to g, as a matrix: fp64 [g, S].
    sf: the scale factor where the caller computes it another way (the square call's sqrt(g * g / n_base)).
    Output line d < floor(S * sf) reads the source coordinate x = s (d + 0.5) - 0.5 with s the FLOAT32 value of 1 / sf (torch hands the
    kernel the scale factor, not the size ratio; align_corners False), four taps around floor(x) weighted by the cubic convolution
    kernel with A = -0.75, taps outside the grid clamped to the border.  Lines floor(S * sf) .. g - 1 are zero rows."""
    import numpy as np
    if sf is None:
        sf = g / math.sqrt(n_base)
    n_out = min(g, int(math.floor(S * sf)))
    s = float(np.float32(1.0 / sf))
    R = np.zeros((g, S), dtype=np.float64)
    A = _CUBIC_A
    for d in range(n_out):
        x = s * (d + 0.5) - 0.5
        ix = math.floor(x)
        t = x - ix
        w = (((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A,
             ((A + 2) * t - (A + 3)) * t * t + 1,
             ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1,
             ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A)
        for k in range(4):
            R[d, min(max(ix - 1 + k, 0), S - 1)] += w[k]
    return R


def vit_pos_matrices(n_base, gh, gw, device, square=False):
    """(Ry fp32 [gh, S], Rx fp32 [gw, S]) of vit_pos_resample, built on the host in fp64 once per (S, gh, gw, device).
    square: gh == gw and both axes take the scale factor of the square call, sqrt(gh * gw / n_base) (interpolate_pos_encoding)"""
    S = int(math.sqrt(n_base))
    key = (S, n_base, gh, gw, str(device), bool(square))
    m = _VIT_POS.get(key)
    if m is None:
        sf = math.sqrt(gh * gw / n_base) if square else None
        m = _VIT_POS[key] = tuple(torch.from_numpy(vit_pos_axis_matrix(S, n_base, g, sf)).float().to(device) for g in (gh, gw))
    return m


def vit_pos_resample(pos_embed, gh, gw, square=False):
    """the position embedding [1, 1 + N, C] of an S x S patch grid (S = int(sqrt(N))) on a gh x gw grid -> [1, 1 + gh * gw, C], patch
    rows first, the class-token entry passed through.  The reference's forward_selfattention (vision_transformer.py:296-312): bicubic
    F.interpolate with the scale-factor tuple (gh / sqrt(N), gw / sqrt(N)), then zero rows / columns where floor(S * sf) falls short of
    the grid (at side 61 from S = 14 or 28, and nowhere else up to 80).  The reference's second pad (:308-310, short columns) assigns
    its result to a name nobody reads and then fails in the add; what it evidently means, zero columns, is built here.

    The map is separable, pos_r = Ry pos Rx^T per channel, so forward and backward are two small fp32 matrix products each, without
    atomics: the gradient of pos_embed comes out with the same bits on every pass.

    square (gh == gw): the scalar-scale call of a square crop instead, F.interpolate(scale_factor=sqrt(gh * gw / N)), which the
    deterministic mode routes here (torch's bicubic backward scatters with atomics)."""
    N, C = pos_embed.shape[1] - 1, pos_embed.shape[2]
    S = int(math.sqrt(N))
    assert not square or gh == gw, (gh, gw)
    Ry, Rx = vit_pos_matrices(N, gh, gw, pos_embed.device, square=square)
    rows = torch.matmul(Ry, pos_embed[0, 1:].reshape(S, S * C)).view(gh, S, C)   # [gh, S, C]
    grid = torch.matmul(Rx, rows)                                                # [gw, S] @ [gh, S, C] -> [gh, gw, C]
    return torch.cat((pos_embed[:, :1], grid.reshape(1, gh * gw, C)), dim=1)


VIT_WINDOW_TOKENS = 224  # crops of at most this many tokens run through the fused windowed kernels (one "window" per image)
_VIT_WIN = {}
# longer crops (patch 8, evaluation above 224^2): "gemm" = the batched-GEMM route of ops.vit_attn_fwd, which keeps P [B nH, N, N] for
# the backward; "flash" = the fused kernels of flash_attn.hip (ops.global_attn_fwd), linear in N.  The speed of the two is compared by
# tools/bench_vit_attn.py; until that A/B has been read the default stays "gemm".
VIT_LONG_ATTENTION = os.environ.get("ESVIT_VIT_LONG_ATTN", "gemm")
if VIT_LONG_ATTENTION not in ("gemm", "flash"):
    raise ValueError("ESVIT_VIT_LONG_ATTN: gemm or flash, not %r" % VIT_LONG_ATTENTION)


def _vit_window(N, nH, device):
    """the geometry a crop of N tokens presents to the windowed kernels: one window per image holding tokens 0..N-1, no bias (a zero
    table over the smallest grid that has N positions -- the kernels mask the slots beyond N), no shift mask"""
    key = (N, nH, str(device))
    g = _VIT_WIN.get(key)
    if g is None:
        ws = 1
        while ws * ws < N:
            ws += 1
        g = (torch.arange(N, dtype=torch.int32, device=device), ws, _zero_table(ws, nH, device))
        _VIT_WIN[key] = g
    return g


def _vit_fused_route(N, hd, dtype):
    """window_attn.hip takes <= 64 tokens at head_dim 32 / 64; window_attn_big.hip <= 224 tokens at head_dim 32, or 64 in bf16"""
    if N <= 64:
        return hd in (32, 64)
    return N <= VIT_WINDOW_TOKENS and (hd == 32 or (hd == 64 and dtype == torch.bfloat16))


def _vit_flash_route(o, N, hd, dtype):
    """does this crop take the flash kernels?  Asked for with VIT_LONG_ATTENTION = "flash"; an ops module without the entry (the CPU
    restatement, oracle/ops_ref.py) or an unsupported shape (fp32 parity mode, other head dims) keeps the batched-GEMM route."""
    if VIT_LONG_ATTENTION != "flash" or N <= VIT_WINDOW_TOKENS or not hasattr(o, "global_attn_fwd"):
        return False
    sup = getattr(o, "global_attn_supported", None)
    return sup is not None and bool(sup(dtype, hd))


def _chunk_fused(o, chunk, dtype, hd):
    """does this sliding-chunk stage take the fused kernels (ops.sliding_chunk_attn_fwd)?  The model asks for them with a fourth tuple
    entry, the chunk side (MsViT._stage under CHUNK_ATTENTION = "fused"); an ops module without the entry (the CPU restatement,
    oracle/ops_ref.py) or an unsupported shape (fp32 parity mode, other head dims) keeps the dense route."""
    if not isinstance(chunk, tuple) or len(chunk) < 4:
        return False
    sup = getattr(o, "sliding_chunk_attn_supported", None)
    return sup is not None and bool(sup(dtype, hd, chunk[3], chunk[1]))


def _chunk3(chunk):
    return chunk[:3] if isinstance(chunk, tuple) else chunk


# the routes of the attention between the projections and the tensors each keeps for its backward, by name.  "gemm" and "chunk_gemm"
# keep what ops.vit_attn_fwd returned (`att`) and hand it back whole
_ATT_KEPT = {"window": ("qkv", "ao", "frag", "lse"), "flash": ("qkv", "ao", "lse"), "gemm": ("att",),
             "chunk_fused": ("qkv", "ao", "lse"), "chunk_gemm": ("att",)}


def _att_saved(route, chunk, **tensors):
    """what vit_attention hands to vit_attention_bwd: the route's name, Vision Longformer's chunk layout (host-side both) and the
    route's tensors as attributes"""
    assert tuple(tensors) == _ATT_KEPT[route]
    return types.SimpleNamespace(route=route, chunk=_chunk3(chunk), **tensors)


def vit_attention(o, qkv, bqkv, nB, N, nH, scale, save, out=None, chunk=None):
    """Attention.forward between the projections (vision_transformer.py:76-83) -> (out, _att_saved for vit_attention_bwd or None).  A
    crop is ONE window of the fused MFMA kernels: the 37 tokens of a 96^2 crop in the 64-slot kernels of window_attn.hip, the 197
    tokens of a 224^2 crop in the 224-slot flash-style kernels of window_attn_big.hip (head_dim 64 in bf16), which also keep a
    log-sum-exp -- no score matrix in HBM ("window").  What does not fit (fp32 parity mode at head_dim 64, longer sequences) takes the
    batched-GEMM route of ops.vit_attn_fwd ("gemm"), or, for longer sequences under VIT_LONG_ATTENTION = "flash", the any-length kernels
    of flash_attn.hip ("flash").  chunk: the sliding-chunk layout of a Vision Longformer stage -- the fused kernels of chunk_attn.hip
    ("chunk_fused") or the masked batched GEMMs ("chunk_gemm").  The route is chosen HERE, once: the backward goes by its name."""
    hd = qkv.shape[1] // 3 // nH
    if chunk is None and _vit_fused_route(N, hd, qkv.dtype):
        win2tok, ws, table = _vit_window(N, nH, qkv.device)
        frag = o.new_bias_frag(nH, N, qkv.device) if save else None
        ao, lse = o.window_attn_fwd(qkv, bqkv, win2tok, N, table, ws, None, 1, N, nH, scale, out=out, bias_frag=frag)
        return ao, (_att_saved("window", None, qkv=qkv, ao=ao, frag=frag, lse=lse) if save else None)
    if chunk is None and _vit_flash_route(o, N, hd, qkv.dtype):
        ao, (_, _, lse) = o.global_attn_fwd(qkv, nB, N, nH, scale, out=out)
        return ao, (_att_saved("flash", None, qkv=qkv, ao=ao, lse=lse) if save else None)
    lse = att = None
    if chunk is None:
        route, (ao, att) = "gemm", o.vit_attn_fwd(qkv, nB, N, nH, scale)
    elif _chunk_fused(o, chunk, qkv.dtype, hd):
        route, (ao, (_, _, lse)) = "chunk_fused", o.sliding_chunk_attn_fwd(qkv, nB, N, nH, scale, chunk[:3])
    else:
        route, (ao, att) = "chunk_gemm", o.vit_attn_fwd(qkv, nB, N, nH, scale, chunk=_chunk3(chunk))
    if out is not None:
        out.copy_(ao)
        ao = out
    if not save:
        return ao, None
    return ao, (_att_saved(route, chunk, qkv=qkv, ao=ao, lse=lse) if route == "chunk_fused" else _att_saved(route, chunk, att=att))


def vit_attention_bwd(o, dao, saved, bqkv, nB, N, nH, scale, dqkv_out=None):
    route = saved.route
    if route == "window":
        win2tok, ws, _ = _vit_window(N, nH, saved.qkv.device)
        return o.window_attn_bwd(saved.qkv, bqkv, win2tok, N, dao, saved.ao, saved.lse, None, ws, None, 1, N, nH, scale, dqkv_out=dqkv_out,
                                 bias_frag=saved.frag, **_no_dbias(o, N, saved.qkv.shape[1] // 3 // nH))[0]
    if route == "flash":
        return o.global_attn_bwd(dao, (saved.qkv, saved.ao, saved.lse), nB, N, nH, scale, dqkv=dqkv_out)
    if route == "gemm":
        dqkv = o.vit_attn_bwd(dao, saved.att, nB, N, nH, scale)
    elif route == "chunk_fused":
        dqkv = o.sliding_chunk_attn_bwd(dao, (saved.qkv, saved.ao, saved.lse), nB, N, nH, scale, saved.chunk)
    elif route == "chunk_gemm":
        dqkv = o.vit_attn_bwd(dao, saved.att, nB, N, nH, scale, chunk=saved.chunk)
    else:
        raise ValueError("vit_attention_bwd: no attention route %r" % (route,))
    if dqkv_out is not None:
        dqkv_out.copy_(dqkv)
        dqkv = dqkv_out
    return dqkv


def _vit_mlp_fwd(o, x1, prm, W1, W2, rowscale, rows_per_sample, save, one_kernel=True):
    """the MLP branch of a ViT block -> (x2, what the backward reads or None).  Inference pass (the EMA teacher, the eval consumers): the
    branch in one kernel (deit_tiny / deit_small widths, whose fused kernels take the plain weight cast) -- unless the caller rules
    it out (one_kernel = False: Vision Longformer, whose inference pass has not been timed on it)"""
    C = x1.shape[1]
    if one_kernel and not save and C in (192, 384) and _mlp_fused_infer(W1, C):
        g2, b2, bfc1, bfc2 = prm
        return o.mlp_fused_fwd(x1, g2, b2, LN_EPS, W1, bfc1, W2, bfc2, rowscale=_per_row(rowscale, rows_per_sample)), None
    return _mlp_fwd(o, x1, prm, W1, W2, LN_EPS, rowscale, rows_per_sample, save)


# ---- ONE block body for the monolithic ViT, its ragged multi-crop form and Vision Longformer: Block.forward (vision_transformer.py:
# 110-116) on token ROWS.  LayerNorm, the four GEMMs and the residual adds are row-wise, so the rows of every resolution group of a step
# run through them together; only the attention depends on a crop's token count and is launched once per group on its row range
# (cf. SwinBlockMultiFn).  Compared with one pass per group (vision_transformer.py:186-233): half the launches, ONE gradient
# contribution per parameter (no accumulation adds; the data-parallel reducer can overlap), half the split-K partial traffic of the
# weight gradients.  The three entry points below differ in their arguments only:
#   segs             tuple of (row0, nB, N): one for vit_block / vil_block (the attention then writes its own output: no `out=`,
#                    no copy on the GEMM routes), one per resolution group for vit_block_multi
#   rows_per_sample  N with per-sample DropPath factors, 1 with per-row ones (ragged)
#   chunk            Vision Longformer's sliding-chunk layout, None otherwise
#   Wkv / bkv        Vision Longformer's `kv` Linear beside `query` (None: one qkv Linear)
#   mlp_one_kernel   may the inference pass take the one-kernel MLP branch (_vit_mlp_fwd)?
def _vit_body_params(prm_list):
    """(norm1.w, norm1.b, Wq | Wqkv, bq | bqkv, Wkv | None, bkv | None, Wproj, bproj, norm2.w, norm2.b, W1, b1, W2, b2) ->
    (vectors, weight parameters, their activation-dtype copies) as _vit_body_fwd takes them"""
    g1, b1, Wq_p, bq, Wkv_p, bkv, Wproj_p, bproj, g2, b2, W1_p, bfc1, W2_p, bfc2 = prm_list
    wts = (_weight(Wq_p), _weight(Wkv_p) if Wkv_p is not None else None, _weight(Wproj_p), _weight(W1_p), _weight(W2_p))
    return (g1, b1, bq, bkv, bproj, g2, b2, bfc1, bfc2), (Wq_p, Wkv_p, Wproj_p, W1_p, W2_p), wts


def _vit_body_fwd(X, segs, rows_per_sample, nH, dp, chunk, mlp_one_kernel, prm, wts, save):
    """X fp32 [M, C]; dp: None or the DropPath factors of (attention branch, MLP branch), one per `rows_per_sample` rows -> (y,
    tensors for the backward by name or None, every segment's _att_saved)"""
    o = ops_module()
    (g1, b1, bq, bkv, bproj, g2, b2, bfc1, bfc2) = prm
    (Wq, Wkv, Wproj, W1, W2) = wts
    M, C = X.shape
    scale = (C // nH) ** -0.5
    dp1, dp2 = (None, None) if dp is None else dp
    xw, _, mean1, rstd1 = o.layernorm_fwd(X, g1, b1, LN_EPS)
    if Wkv is None:   # one qkv Linear
        qkv, bqkv = o.linear_fwd(xw, Wq, bq), bq
    else:             # query | kv Linears: the same [q | k | v] column layout (longformer2d.py:160-162)
        qkv = torch.cat((o.linear_fwd(xw, Wq, bq), o.linear_fwd(xw, Wkv, bkv)), dim=1)
        bqkv = torch.cat((bq.detach(), bkv.detach()))
    if len(segs) == 1:
        (_, nB, N), = segs
        ao, att = vit_attention(o, qkv, bqkv, nB, N, nH, scale, save, chunk=chunk)
        atts = [att]
    else:
        ao = torch.empty((M, C), dtype=qkv.dtype, device=X.device)
        atts = [vit_attention(o, qkv[r0:r0 + nB * N], bqkv, nB, N, nH, scale, save, out=ao[r0:r0 + nB * N], chunk=chunk)[1] for (r0, nB, N) in segs]
    x1 = o.linear_fwd(ao, Wproj, bproj, residual=X, rowscale=dp1, rows_per_sample=rows_per_sample, out_f32=True)
    x2, mlp_saved = _vit_mlp_fwd(o, x1, (g2, b2, bfc1, bfc2), W1, W2, dp2, rows_per_sample, save, one_kernel=mlp_one_kernel)
    saved = dict(mean1=mean1, rstd1=rstd1, xw=xw, ao=ao, x1=x1, bqkv=bqkv, **dict(zip(_MLP_SAVED, mlp_saved))) if save else None
    return x2, saved, atts


class VitBodyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, segs, rows_per_sample, nH, dp, chunk, mlp_one_kernel, *prm_list):
        prm, ctx.wparams, wts = _vit_body_params(prm_list)
        Wq, Wkv, Wproj, W1, W2 = wts
        g1, b1, bq, bkv, bproj, g2, b2, bfc1, bfc2 = prm
        y, saved, atts = _vit_body_fwd(X, segs, rows_per_sample, nH, dp, chunk, mlp_one_kernel, prm, wts, True)
        ctx.segs, ctx.rows_per_sample, ctx.nH, ctx.dp = segs, rows_per_sample, nH, dp
        ctx.bparams = (bq, bkv, bproj, bfc1, bfc2)
        ctx.nparams = (g1, b1, g2, b2)
        ctx.att_host = [(a.route, a.chunk) for a in atts]  # the tensors of segment i go under "att<i>_<name>"
        _save_named(ctx, X=X, g1=g1, g2=g2, Wq=Wq, Wkv=Wkv, Wproj=Wproj, W1=W1, W2=W2, **saved,
                    **{"att%d_%s" % (i, k): getattr(a, k) for i, a in enumerate(atts) for k in _ATT_KEPT[a.route]})
        return y

    @staticmethod
    def backward(ctx, gy):
        o = ops_module()
        segs, rps, nH, dp = ctx.segs, ctx.rows_per_sample, ctx.nH, ctx.dp
        s = _load_named(ctx)
        X, xw, ao = s.X, s.xw, s.ao
        atts = [_att_saved(route, chunk, **{k: getattr(s, "att%d_%s" % (i, k)) for k in _ATT_KEPT[route]}) for i, (route, chunk) in enumerate(ctx.att_host)]
        M, C = X.shape
        scale = (C // nH) ** -0.5
        dp1, dp2 = (None, None) if dp is None else dp
        gy = gy.contiguous()
        Wq_p, Wkv_p, Wproj_p, W1_p, W2_p = ctx.wparams
        bq_p, bkv_p, bproj_p, bfc1_p, bfc2_p = ctx.bparams
        g1_p, b1_p, g2_p, b2_p = ctx.nparams
        dyb = o.gather_cast(gy, M, rowscale=dp2, rows_per_sample=rps)
        dh, dW1, dbfc1, dW2, dbfc2 = _mlp_bwd(o, dyb, s.h, s.a1, s.a1g, s.W1, s.W2, (W1_p, bfc1_p, W2_p, bfc2_p))
        sink1, sink2 = _ln_sinks(g1_p, b1_p), _ln_sinks(g2_p, b2_p)
        gx1, dyw, dg2, db2 = o.layernorm_bwd_cast(dh, s.x1, s.mean2, s.rstd2, s.g2, g_in=gy, rowscale=dp1, rows_per_sample=rps, gb_out=sink2)
        dWproj, dbproj = _side_run(lambda: _wgrad(dyw, ao, Wproj_p, want_bias=True, bias_param=bproj_p), dyw, ao)
        dao = o.linear_dgrad(dyw, s.Wproj)
        if len(segs) == 1:
            (_, nB, N), = segs
            dqkv = vit_attention_bwd(o, dao, atts[0], s.bqkv, nB, N, nH, scale)
        else:
            dqkv = torch.empty((M, 3 * C), dtype=dao.dtype, device=dao.device)
            for (r0, nB, N), att in zip(segs, atts):
                r1 = r0 + nB * N
                vit_attention_bwd(o, dao[r0:r1], att, s.bqkv, nB, N, nH, scale, dqkv_out=dqkv[r0:r1])
        if Wkv_p is None:
            dWq, dbq = _side_run(lambda: _wgrad(dqkv, xw, Wq_p, want_bias=True, bias_param=bq_p), dqkv, xw)
            dWkv, dbkv = None, None
            dxw = o.linear_dgrad(dqkv, s.Wq)
        else:
            dq, dkv = dqkv[:, :C].contiguous(), dqkv[:, C:].contiguous()
            dWq, dbq = _side_run(lambda: _wgrad(dq, xw, Wq_p, want_bias=True, bias_param=bq_p), dq, xw)
            dWkv, dbkv = _side_run(lambda: _wgrad(dkv, xw, Wkv_p, want_bias=True, bias_param=bkv_p), dkv, xw)
            dxw = o.linear_dgrad(dqkv, torch.cat((s.Wq, s.Wkv), 0))  # dq Wq + dkv Wkv as one product over the stacked (tiny) weights
        gx, dg1, db1 = o.layernorm_bwd(dxw, X, s.mean1, s.rstd1, s.g1, g_in=gx1, gb_out=sink1)
        _side_join()
        return (gx, None, None, None, None, None, None, _alias(dg1, sink1), _alias(db1, sink1), dWq, dbq, dWkv, dbkv, dWproj, dbproj,
                _alias(dg2, sink2), _alias(db2, sink2), dW1, dbfc1, dW2, dbfc2)


def _vit_body(X, segs, rows_per_sample, nH, dp, chunk, mlp_one_kernel, prm_list):
    """X fp32 [M, C] through one block; the inference pass keeps nothing and builds no node"""
    X = X.contiguous()
    if torch.is_grad_enabled() and (X.requires_grad or any(p is not None and p.requires_grad for p in prm_list)):
        return VitBodyFn.apply(X, segs, rows_per_sample, nH, dp, chunk, mlp_one_kernel, *prm_list)
    prm, _, wts = _vit_body_params(prm_list)
    return _vit_body_fwd(X, segs, rows_per_sample, nH, dp, chunk, mlp_one_kernel, prm, wts, False)[0]


def vit_block(x, nH, dp, prm_list):
    """x fp32 [nB, N, C]; dp: None or the per-sample DropPath factors of the two branches"""
    nB, N, C = x.shape
    return _vit_body(x.contiguous().view(nB * N, C), ((0, nB, N),), N, nH, dp, None, True, (*prm_list[:4], None, None, *prm_list[4:])).view(nB, N, C)


def vit_block_multi(X, segs, nH, dp_rows, prm_list):
    """one ViT block over the token rows of several resolution groups; X fp32 [M, C]; segs: tuple of (row0, nB, N); dp_rows: None or
    (per-row DropPath scale of the attention branch [M], MLP branch [M])"""
    return _vit_body(X, segs, 1, nH, dp_rows, None, True, (*prm_list[:4], None, None, *prm_list[4:]))


def _vit_block_qkv(o, x, nH, prm_list):
    """LayerNorm and the qkv projection of a block recomputed on its input x fp32 [nB, N, C] -> (qkv, nB, N, scale)"""
    g1, b1, Wqkv_p, bqkv = prm_list[:4]
    nB, N, C = x.shape
    xw = o.layernorm_fwd(x.contiguous().view(nB * N, C), g1, b1, LN_EPS)[0]
    return o.linear_fwd(xw, _weight(Wqkv_p), bqkv), nB, N, (C // nH) ** -0.5


def vit_block_attention(x, nH, prm_list):
    """the attention probabilities [nB, nH, N, N] of a block (Block.forward(return_attention=True), vision_transformer.py:112)"""
    o = ops_module()
    qkv, nB, N, scale = _vit_block_qkv(o, x, nH, prm_list)
    p = o.vit_attn_fwd(qkv, nB, N, nH, scale)[1][-1]  # (evaluation hook: the batched-GEMM route keeps P in memory)
    return p.reshape(nB, nH, p.shape[-2], p.shape[-1])[:, :, :N, :N].float()


def _vit_stats_route(o, hd, dtype):
    """do the attention statistics take the kernels of flash_attn.hip (ops.global_attn_stats)?  For every N (37 and 197 tokens
    included: one kernel serves all crops) when the ops module has the entry and supports the shape; an ops module without it (the CPU
    restatement, oracle/ops_ref.py) or an unsupported shape (fp32 parity mode, other head dims) reduces P of the batched-GEMM route."""
    if not hasattr(o, "global_attn_stats"):
        return False
    sup = getattr(o, "global_attn_stats_supported", None)
    return sup is not None and bool(sup(dtype, hd))


class _long_attention:
    """with _long_attention("flash"): ... -- VIT_LONG_ATTENTION for the duration of a block of code (the analysis pass of
    esvit_amd/analysis.py asks for the flash forward, so that no N x N tensor exists while it advances through the blocks either)"""

    def __init__(self, route):
        assert route in ("gemm", "flash")
        self.route = route

    def __enter__(self):
        global VIT_LONG_ATTENTION
        self.old, VIT_LONG_ATTENTION = VIT_LONG_ATTENTION, self.route

    def __exit__(self, *exc):
        global VIT_LONG_ATTENTION
        VIT_LONG_ATTENTION = self.old


_STATS_SLICE_ELEMS = 1 << 26  # fall-back route: at most this many probabilities (256 MB in fp32) at a time


def _dense_attention_stats(o, who, qkv, nB, N, nH, scale, queries, fp32=False, **route):
    """the fall-back of the statistics: P of o.vit_attn_fwd(..., **route) for a slice of the batch at a time, reduced in torch.  fp32: the
    slice's qkv enters the route as fp32, so that scores and P are not rounded to bf16 on the way to an fp32 result"""
    idx = None
    if queries is not None:
        idx = torch.as_tensor(queries, device=qkv.device).reshape(-1).long()
        if idx.numel() and not (0 <= int(idx.min()) and int(idx.max()) < N):
            raise ValueError("%s: query indices must lie in [0, %d)" % (who, N))
    step = max(1, _STATS_SLICE_ELEMS // (nH * N * N))
    ents, rows = [], []
    for b0 in range(0, nB, step):
        nb = min(step, nB - b0)
        part = qkv[b0 * N:(b0 + nb) * N]
        p = o.vit_attn_fwd(part.float() if fp32 else part, nb, N, nH, scale, **route)[1][-1]
        p = p.reshape(nb, nH, p.shape[-2], p.shape[-1])[:, :, :N, :N].float()
        ents.append(torch.special.entr(p).sum(-1))
        if idx is not None:
            rows.append(p.index_select(2, idx))
    return torch.cat(ents), (torch.cat(rows) if idx is not None else None)


def vit_attention_stats(o, qkv, nB, N, nH, scale, queries=None):
    """what an attention analysis reads of a block's softmax(scale q k^T), qkv [nB * N, 3C] -> (entropy fp32 [nB, nH, N] in nats with
    0 log 0 = 0, rows fp32 [nB, nH, nq, N] of the listed query tokens or None).  The kernels of flash_attn.hip never form P; the
    fall-back forms P of o.vit_attn_fwd for a slice of the batch at a time and reduces it in torch."""
    hd = qkv.shape[1] // 3 // nH
    if _vit_stats_route(o, hd, qkv.dtype):
        ent, rows, _ = o.global_attn_stats(qkv, nB, N, nH, scale, queries=queries)
        return ent, rows
    return _dense_attention_stats(o, "vit_attention_stats", qkv, nB, N, nH, scale, queries)


def vit_block_attention_stats(x, nH, prm_list, queries=None):
    """vit_attention_stats of a block's attention on its input x fp32 [nB, N, C] (LayerNorm and the qkv projection are recomputed, as
    vit_block_attention does)"""
    o = ops_module()
    qkv, nB, N, scale = _vit_block_qkv(o, x, nH, prm_list)
    return vit_attention_stats(o, qkv, nB, N, nH, scale, queries)


# ------------------------------------------------------------------------------------------------
# Vision Longformer (models/vision_longformer.py:406-770): an AttnBlock followed by its MlpBlock is one autograd node: the body of a ViT
# block (_vit_body).  'full' stages project with one qkv Linear (vision_longformer.py:36-118); 'longformerhand' stages (layers/longformer2d.py)
# with `query` and `kv` Linears -- shared by local and global tokens (sharew) -- and restrict every local query to the global tokens
# plus its own and the eight adjacent w x w chunks (`chunk`, esvit_softmax_rows_chunked_fwd).  rpe off (the ape = 1 default of
# the reference's yaml files): no bias tables.
# ------------------------------------------------------------------------------------------------
def vil_block(x, nH, dp, chunk, prm_list):
    """prm_list = (norm.w, norm.b, Wq | Wqkv, bq | bqkv, Wkv | None, bkv | None, Wproj, bproj, norm2.w, norm2.b, W1, b1, W2, b2).  The
    inference pass keeps the unfused MLP branch at every width"""
    nB, N, C = x.shape
    return _vit_body(x.contiguous().view(nB * N, C), ((0, nB, N),), N, nH, dp, chunk, False, prm_list).view(nB, N, C)


def _vil_stats_route(o, chunk, dtype, hd):
    """do the statistics of a sliding-chunk stage take the kernels of chunk_attn.hip (ops.chunk_attn_stats)?  When the ops module has the
    entry and supports the shape; an ops module without it (the CPU restatement, oracle/ops_ref.py) or an unsupported shape (fp32 parity
    mode, other head dims or chunk sides) reduces P of the dense route."""
    if not hasattr(o, "chunk_attn_stats") or not isinstance(chunk, tuple) or len(chunk) < 3:
        return False
    sup = getattr(o, "chunk_attn_stats_supported", None)
    w = chunk[3] if len(chunk) > 3 else getattr(o, "CHUNK_W", 7)
    return sup is not None and bool(sup(dtype, hd, w, chunk[1]))


def vil_attention_stats(o, qkv, nB, N, nH, scale, chunk, queries=None):
    """what an attention analysis reads of a sliding-chunk block's softmax, qkv [nB * N, 3C] (tokens [globals | (x, y) row-major]) ->
    (entropy fp32 [nB, nH, N] in nats with 0 log 0 = 0, every row over the keys it sees; rows fp32 [nB, nH, nq, N] of the listed query
    tokens over all N tokens, zero where the query does not see, or None).  chunk: (table, nglo, tokens per chunk row[, w]).  The
    kernels of chunk_attn.hip never form P; the fall-back forms P of o.vit_attn_fwd(..., chunk=) for a slice of the batch at a time
    and reduces it in torch.  It runs that route in fp32 whatever the activation dtype: the kernels keep scores and probabilities in
    fp32, and the dense route in bf16 rounds both (2^-8 relative each; 0.015 - 0.027 nats in the entropy at the stage shapes), so the
    two routes of this function would otherwise return different numbers for the same block depending on the shape alone."""
    hd = qkv.shape[1] // 3 // nH
    if _vil_stats_route(o, chunk, qkv.dtype, hd):
        return o.chunk_attn_stats(qkv, nB, N, nH, scale, chunk, queries=queries)
    return _dense_attention_stats(o, "vil_attention_stats", qkv, nB, N, nH, scale, queries, fp32=True, chunk=_chunk3(chunk))


def _vil_block_qkv(o, x, nH, prm_list):
    """LayerNorm and the `query | kv` (sliding-chunk stages) or `qkv` (full stages) projection of a block pair recomputed on its input
    x fp32 [nB, N, C], as _vit_body_fwd forms them -> (qkv, nB, N, scale)"""
    g1, b1, Wq_p, bq, Wkv_p, bkv = prm_list[:6]
    nB, N, C = x.shape
    xw = o.layernorm_fwd(x.contiguous().view(nB * N, C), g1, b1, LN_EPS)[0]
    if Wkv_p is None:
        qkv = o.linear_fwd(xw, _weight(Wq_p), bq)
    else:
        qkv = torch.cat((o.linear_fwd(xw, _weight(Wq_p), bq), o.linear_fwd(xw, _weight(Wkv_p), bkv)), dim=1)
    return qkv, nB, N, (C // nH) ** -0.5


def vil_block_attention_stats(x, nH, chunk, prm_list, queries=None):
    """the statistics of a Vision Longformer block pair's attention on its input x fp32 [nB, N, C]; prm_list and chunk as vil_block takes
    them (chunk = None: a full-attention stage, vit_attention_stats)"""
    o = ops_module()
    qkv, nB, N, scale = _vil_block_qkv(o, x, nH, prm_list)
    if chunk is None:
        return vit_attention_stats(o, qkv, nB, N, nH, scale, queries)
    return vil_attention_stats(o, qkv, nB, N, nH, scale, chunk, queries)
