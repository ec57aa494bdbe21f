"""The on-chip weight-gradient mode of esvit_mlp_fused_bwd, host side: the boundary keeps its 60 symbols, the binding matches the
header, and functional._mlp_branch_bwd routes by what the ops module offers (no GPU)."""
import os
import re
import subprocess
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esvit_hip.h")).read(), flags=re.S)


def test_boundary_is_unchanged_in_size_and_the_binding_matches(lib_built):
    from esvit_amd import _lib, ops
    hdr = _header()
    declared = set(re.findall(r"\b(esvit_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 60 and declared == set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("esvit_")}
    assert exported == declared
    decl = re.search(r"int esvit_mlp_fused_bwd\((.*?)\);", hdr, flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    res, argtypes = _lib.SIGNATURES["esvit_mlp_fused_bwd"]
    assert len(args) == len(argtypes) == 25
    assert [a.split()[-1].lstrip("*") for a in args[-6:]] == ["stream", "dW2", "G", "db1", "db2", "partials_ws"]
    for a, t in zip(args, argtypes):  # pointers and the stream handle are void pointers; eps is the one float; M the one 64-bit integer
        want = _lib.vp if ("*" in a or "esvit_stream_t" in a) else (_lib.f32 if a.startswith("float") else (_lib.i64 if a.startswith("int64_t") else _lib.C.c_int))
        assert t is want, (a, t)
    raw = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "#define ESVIT_Q_MLP_DW_WS %d" % ops.Q_MLP_DW_WS in raw and "#define ESVIT_MLP_DW_PARTIAL_FLOATS %d" % ops.MLP_DW_PARTIAL_FLOATS in raw
    assert ops.MLP_DW_PARTIAL_FLOATS == 2 * 96 * 384 + 384 + 96


def test_query_answers_without_a_device(lib_built):
    from esvit_amd import ops
    per = 4 * ops.MLP_DW_PARTIAL_FLOATS
    assert ops.query(ops.Q_MLP_DW_WS, 1, 96, 1) == per  # one tile, one workgroup
    assert ops.query(ops.Q_MLP_DW_WS, 1, 96, 64 * 3 + 1) == 4 * per
    big = ops.query(ops.Q_MLP_DW_WS, 1, 96, 1 << 30)
    assert big % per == 0 and 0 < big // per <= 1024 and big == ops.query(ops.Q_MLP_DW_WS, 1, 96, 1 << 31)  # capped by the chip, not by M
    for dt, C in ((0, 96), (1, 192), (1, 128), (1, 384)):
        assert ops.query(ops.Q_MLP_DW_WS, dt, C, 4096) == 0
    assert ops.query(ops.Q_MLP_DW_WS, 1, 96, 0) == 0
    assert ops.mlp_fused_dw_supported(torch.bfloat16, 96) and not ops.mlp_fused_dw_supported(torch.bfloat16, 192)
    assert not ops.mlp_fused_dw_supported(torch.float32, 96)


def _branch_inputs(C=96, M=37):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x1, gy = r(M, C), r(M, C) * 0.5
    prm = [torch.nn.Parameter(t) for t in (1 + 0.1 * r(C), 0.1 * r(C), 0.08 * r(4 * C, C), 0.1 * r(4 * C), 0.05 * r(C, 4 * C), 0.1 * r(C))]
    return x1, gy, prm


def test_cpu_stand_in_keeps_the_present_route(lib_built, monkeypatch):
    from esvit_amd import functional as F
    from oracle import ops_ref
    assert F.MLP_DW_ONCHIP and not hasattr(ops_ref, "mlp_fused_bwd_dw")
    monkeypatch.setattr(F, "ops", ops_ref)
    x1, gy, prm = _branch_inputs()
    g2, b2, W1_p, bfc1, W2_p, bfc2 = prm
    dt = torch.bfloat16
    W1 = W1_p.detach().to(dt)
    assert not F._mlp_dw_onchip(ops_ref, W1, 96)
    calls = []
    real = ops_ref.mlp_fused_bwd
    monkeypatch.setattr(ops_ref, "mlp_fused_bwd", lambda *a, **k: (calls.append("bwd"), real(*a, **k))[1])
    real_wg = ops_ref.linear_wgrad
    monkeypatch.setattr(ops_ref, "linear_wgrad", lambda *a, **k: (calls.append("wgrad"), real_wg(*a, **k))[1])
    dyb = gy.to(dt)
    out = F._mlp_branch_bwd(ops_ref, x1, gy, dyb, g2.detach(), b2.detach(), W1, bfc1.detach(), tuple(prm), None, None)
    assert calls == ["bwd", "wgrad", "wgrad"] and len(out) == 8
    assert out[4].shape == (384, 96) and out[6].shape == (96, 384)


def test_new_route_hands_the_sinks_over(lib_built, monkeypatch):
    from esvit_amd import functional as F
    from esvit_amd import params as P
    from oracle import ops_ref
    x1, gy, prm = _branch_inputs()
    g2, b2, W1_p, bfc1, W2_p, bfc2 = prm
    M, C = x1.shape
    seen = {}

    def mlp_fused_bwd_dw(x, gyy, gamma, beta, eps, W1, W2T, W1T, b1, *, rowscale_mlp=None, rowscale_out=None, out=None, db_out=None):
        seen.update(out=out, db_out=db_out, rs=(rowscale_mlp, rowscale_out), shapes=(W1.shape, W2T.shape, W1T.shape))
        dW2, G = out
        db2, db1 = db_out
        dW2 = dW2 if dW2 is not None else torch.empty(C, 4 * C)
        G = G if G is not None else torch.empty(4 * C, C)
        db2 = db2 if db2 is not None else torch.empty(C)
        db1 = db1 if db1 is not None else torch.empty(4 * C)
        dW2.fill_(1.0), G.fill_(2.0), db2.fill_(3.0), db1.fill_(4.0)
        return torch.full_like(x, 5.0), torch.full((M, C), 6.0, dtype=torch.bfloat16), dW2, db2, G, db1

    def forbidden(*a, **k):
        raise AssertionError("the present route was taken")

    stub = types.SimpleNamespace(mlp_fused_bwd_dw=mlp_fused_bwd_dw, mlp_fused_dw_supported=lambda dt, C_: dt == torch.bfloat16 and C_ == 96,
                                 mlp_fused_bwd=forbidden, linear_wgrad=forbidden, mlp_fused_weight=ops_ref.mlp_fused_weight,
                                 ln_fold_finish=ops_ref.ln_fold_finish, MLP_W1_BWD=ops_ref.MLP_W1_BWD, MLP_W2T_BWD=ops_ref.MLP_W2T_BWD,
                                 MLP_W1T_BWD=ops_ref.MLP_W1T_BWD)
    monkeypatch.setattr(F, "ops", stub)
    W1 = W1_p.detach().to(torch.bfloat16)
    assert F._mlp_dw_onchip(stub, W1, 96) and not F._mlp_dw_onchip(stub, W1, 192) and not F._mlp_dw_onchip(stub, W1.float(), 96)
    monkeypatch.setattr(F, "MLP_DW_ONCHIP", False)
    assert not F._mlp_dw_onchip(stub, W1, 96)  # ESVIT_MLP_DW_ONCHIP=0
    monkeypatch.setattr(F, "MLP_DW_ONCHIP", True)
    sinks = {id(p): torch.zeros_like(p) for p in prm}
    P.set_grad_sink(sinks)
    try:
        rs_mlp, rs_out = torch.rand(M), torch.rand(M)
        gx1, dyw, dg2, db2, dW1, dbfc1, dW2, dbfc2 = F._mlp_branch_bwd(stub, x1, gy, None, g2.detach(), b2.detach(), W1, bfc1.detach(), tuple(prm), rs_mlp, rs_out)
    finally:
        P.set_grad_sink(None)
    assert seen["out"][0] is sinks[id(W2_p)] and seen["out"][1] is sinks[id(W1_p)]
    assert seen["db_out"][0] is sinks[id(bfc2)] and seen["db_out"][1] is sinks[id(bfc1)]
    assert seen["rs"][0] is rs_mlp and seen["rs"][1] is rs_out and seen["shapes"] == ((4 * C, C), (4 * C, C), (C, 4 * C))
    assert float(gx1[0, 0]) == 5.0 and float(dyw[0, 0]) == 6.0
    # every gradient lives in its slot and is handed on as a fresh alias of it
    for got, p in ((dW1, W1_p), (dbfc1, bfc1), (dW2, W2_p), (dbfc2, bfc2), (dg2, g2), (db2, b2)):
        assert got.data_ptr() == sinks[id(p)].data_ptr() and got is not sinks[id(p)]
    assert bool((dW2 == 1).all()) and bool((dbfc2 == 3).all()) and bool((dbfc1 == 4).all())
    # the fold ran on G = 2, db1 = 4:  dW1 = G o gamma + db1 (x) beta,  dgamma = sum_j W G,  dbeta = db1 W
    W = W1_p.detach()
    assert torch.allclose(dW1, 2.0 * g2.detach()[None, :] + 4.0 * b2.detach()[None, :].expand(4 * C, C))
    assert torch.allclose(dg2, (W * 2.0).sum(0), atol=1e-5) and torch.allclose(db2, 4.0 * W.sum(0), atol=1e-5)
    # without armed slots the op allocates
    seen.clear()
    F._mlp_branch_bwd(stub, x1, gy, None, g2.detach(), b2.detach(), W1, bfc1.detach(), tuple(prm), None, None)
    assert seen["out"] == (None, None) and seen["db_out"] == (None, None)
