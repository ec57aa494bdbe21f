"""The qkv-tail mode of esvit_layernorm_bwd, host side (no GPU): its torch restatement against fp64 autograd of LayerNorm -> linear, the
header / binding constants, the query's answers without a device, the argument checks that precede any launch, and the routing of
functional: off on the CPU stand-in (which has no such op), on with an ops module that offers it."""
import ctypes
import os
import re
import types

import pytest
import torch

from tests import attn_tail_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 96
NAMES = ("gx", "dx_act", "dWqkv", "dbqkv", "dgamma", "dbeta")


@pytest.mark.parametrize("M,rs", [(1, False), (49, True), (64 * 3 + 37, True)])
def test_restatement_against_fp64_autograd(M, rs):
    i = AR.inputs(M, C, 11 + M, torch.device("cpu"))
    rowscale = None
    if rs:
        rowscale = (torch.rand(M, generator=torch.Generator().manual_seed(3)) > 0.3).float().div(0.7)
        rowscale[0] = 0.0
    got = AR.attn_tail_bwd(i["dqkv"], i["x"], i["mean"], i["rstd"], i["gamma"], i["beta"], i["Wqkv"], i["g_in"], rowscale, 1, True, wide=torch.float64)
    ex = AR.exact(i["dqkv"], i["x"], i["gamma"], i["beta"], i["Wqkv"], i["g_in"], i["eps"], rowscale, 1)
    # the two bf16 roundings (dxw, xw) are 2^-9 of a value each; sums of M such errors stay below 2^-8 of the largest output
    for name, g in zip(NAMES, got):
        e = ex[name]
        err = (g.double() - e).abs().max().item() / (e.abs().max().item() + 1e-12)
        assert err <= 2.0 ** -7, (name, err)
    if rs:
        assert bool((got[1][0] == 0).all())  # a dropped row's copy is zero


def test_constants_and_binding_match_the_header(lib_built):
    from esvit_amd import _lib, ops
    raw = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "#define ESVIT_Q_ATTN_TAIL_WS %d" % ops.Q_ATTN_TAIL_WS in raw
    assert "#define ESVIT_ATTN_TAIL_PARTIAL_FLOATS %d" % ops.ATTN_TAIL_PARTIAL_FLOATS in raw
    assert "#define ESVIT_LN_BWD_QKV_TAIL (%d)" % ops.LN_BWD_QKV_TAIL in raw
    assert ops.ATTN_TAIL_PARTIAL_FLOATS == 288 * 96 + 288 + 96 + 96
    rec = re.search(r"typedef struct esvit_ln_qkv_tail \{(.*?)\} esvit_ln_qkv_tail;", re.sub(r"/\*.*?\*/", "", raw, flags=re.S), flags=re.S).group(1)
    fields = [f.split()[-1].lstrip("*") for f in rec.split(";") if f.strip()]
    assert fields == [n for n, _ in ops.LnQkvTail._fields_] and ctypes.sizeof(ops.LnQkvTail) == 8 * len(fields)
    # the mode rides on an existing entry point: the boundary does not grow
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert set(re.findall(r"\b(esvit_[a-z0-9_]+)\s*\(", hdr)) == set(_lib.SIGNATURES)


def test_query_answers_without_a_device(lib_built):
    from esvit_amd import ops
    per = 4 * ops.ATTN_TAIL_PARTIAL_FLOATS
    assert ops.query(ops.Q_ATTN_TAIL_WS, 1, 96, 1) == per and ops.query(ops.Q_ATTN_TAIL_WS, 1, 96, 64) == per
    assert ops.query(ops.Q_ATTN_TAIL_WS, 1, 96, 64 * 3 + 1) == 4 * per
    big = ops.query(ops.Q_ATTN_TAIL_WS, 1, 96, 1 << 30)
    assert big % per == 0 and 0 < big // per <= 1024
    assert big // per == ops.mlp_fused_dw_grid(torch.bfloat16, 96, 1 << 30)  # the same walk as the MLP kernel's
    for dt, Cc in ((0, 96), (1, 192), (1, 128), (1, 384)):
        assert ops.query(ops.Q_ATTN_TAIL_WS, dt, Cc, 4096) == 0
    assert ops.query(ops.Q_ATTN_TAIL_WS, 1, 96, 0) == 0
    assert ops.attn_tail_bwd_supported(torch.bfloat16, 96) and not ops.attn_tail_bwd_supported(torch.bfloat16, 192)
    assert not ops.attn_tail_bwd_supported(torch.float32, 96) and not ops.attn_tail_bwd_supported(torch.float16, 96)


def test_misuse_is_refused_before_any_launch(lib_built):
    """fake (aligned, never dereferenced) addresses: every refusal precedes the first launch, so this runs without a GPU"""
    from esvit_amd import ops
    from esvit_amd._lib import lib
    f = ctypes.c_void_p(0x10000)
    rec = ops.LnQkvTail(0x20000, 0x30000, 0x40000, 0x50000)
    rp = ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p)

    def call(dtype=1, Cc=96, rows=77, dy=f, g_in=f, dx=f, ws=f, r=rp, tokens=0, dx_act=None, act=0, rowscale=None, rps=0):
        return lib.esvit_layernorm_bwd(dtype, dy, f, f, f, f, g_in, rows, Cc, dx, f, f, ws, r, tokens, ops.LN_BWD_QKV_TAIL, dx_act, act, rowscale, rps, None)

    ARG = -1
    assert call(dtype=0) == ARG and call(Cc=192) == ARG and call(Cc=128) == ARG and call(dtype=7) == ARG
    assert call(rows=0) == ARG and call(g_in=None) == ARG and call(dx=None) == ARG and call(ws=None) == ARG and call(r=None) == ARG
    assert call(tokens=49) == ARG
    assert call(dy=ctypes.c_void_p(0x10008)) == ARG and call(dx_act=ctypes.c_void_p(0x10004), act=1) == ARG
    assert call(dx_act=f, act=0) == ARG and call(rowscale=f, rps=1) == ARG and call(dx_act=f, act=1, rowscale=f, rps=0) == ARG
    for k in range(4):
        bad = ops.LnQkvTail(*[None if j == k else 0x20000 + 0x10000 * j for j in range(4)])
        assert call(r=ctypes.cast(ctypes.pointer(bad), ctypes.c_void_p)) == ARG
    assert b"qkv tail" in lib.esvit_last_error()


def test_cpu_stand_in_keeps_the_present_chain(lib_built):
    from esvit_amd import functional as F
    from oracle import ops_ref
    assert F.ATTN_TAIL_FUSED and not hasattr(ops_ref, "attn_tail_bwd")
    assert not F._attn_tail_fused(ops_ref, torch.bfloat16, 96)


def test_routing_follows_the_ops_module_and_the_switch(lib_built, monkeypatch):
    from esvit_amd import functional as F
    from esvit_amd import params as P
    seen = {}
    M = 37

    def attn_tail_bwd(dqkv, x, mean, rstd, gamma, beta, Wqkv, g_in, *, rowscale=None, rows_per_sample=0, want_act=False, out=None, db_out=None, gb_out=None):
        seen.update(out=out, db_out=db_out, gb_out=gb_out, rowscale=rowscale, want_act=want_act)
        dW = out if out is not None else torch.empty(3 * C, C)
        db = db_out if db_out is not None else torch.empty(3 * C)
        dg, dbt = gb_out if gb_out is not None else (torch.empty(C), torch.empty(C))
        dW.fill_(1.0), db.fill_(2.0), dg.fill_(3.0), dbt.fill_(4.0)
        return torch.full_like(x, 5.0), (torch.full((M, C), 6.0, dtype=torch.bfloat16) if want_act else None), dW, db, dg, dbt

    def colsum(t, out=None, accumulate=False):
        assert accumulate
        out += t.sum(0)
        return out

    stub = types.SimpleNamespace(attn_tail_bwd=attn_tail_bwd, attn_tail_bwd_supported=lambda dt, C_: dt == torch.bfloat16 and C_ == 96, colsum=colsum)
    assert F._attn_tail_fused(stub, torch.bfloat16, 96) and not F._attn_tail_fused(stub, torch.bfloat16, 192)
    assert not F._attn_tail_fused(stub, torch.float32, 96)
    monkeypatch.setattr(F, "ATTN_TAIL_FUSED", False)
    assert not F._attn_tail_fused(stub, torch.bfloat16, 96)  # ESVIT_ATTN_TAIL_FUSED=0
    monkeypatch.setattr(F, "ATTN_TAIL_FUSED", True)
    prm = [torch.nn.Parameter(t) for t in (torch.ones(C), torch.zeros(C), torch.zeros(3 * C, C), torch.zeros(3 * C))]
    sinks = {id(p): torch.zeros_like(p) for p in prm}
    pads = (torch.ones(5, 2 * C), torch.ones(3, 2 * C))
    rs = torch.rand(M)
    args = (torch.zeros(M, 3 * C, dtype=torch.bfloat16), torch.zeros(M, C), torch.zeros(M), torch.ones(M), prm[0].detach(), torch.zeros(3 * C, C, dtype=torch.bfloat16),
            torch.zeros(M, C), pads, tuple(prm))
    P.set_grad_sink(sinks)
    try:
        gx, gxb, dg1, db1, dW, db = F._attn_tail_bwd(stub, *args, rs, 1, True)
    finally:
        P.set_grad_sink(None)
    assert seen["out"] is sinks[id(prm[2])] and seen["db_out"] is sinks[id(prm[3])] and seen["gb_out"][0] is sinks[id(prm[0])] and seen["gb_out"][1] is sinks[id(prm[1])]
    assert seen["rowscale"] is rs and seen["want_act"] and float(gx[0, 0]) == 5.0 and float(gxb[0, 0]) == 6.0
    for got, p in ((dg1, prm[0]), (db1, prm[1]), (dW, prm[2]), (db, prm[3])):  # every gradient lives in its slot, handed on as a fresh alias
        assert got.data_ptr() == sinks[id(p)].data_ptr() and got is not sinks[id(p)]
    assert bool((db[:C] == 2).all()) and bool((db[C:] == 2 + 8).all())  # the pad slots' column sums land behind the reduce, on k / v only
    # without a reader for the copy no row scale is passed on; without armed slots the op allocates
    F._attn_tail_bwd(stub, *args, rs, 1, False)
    assert seen["rowscale"] is None and not seen["want_act"] and seen["out"] is None and seen["db_out"] is None and seen["gb_out"] is None
