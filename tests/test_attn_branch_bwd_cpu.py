"""The backward mode of the fused attention branch, host side (no GPU): the boundary keeps its 60 names and the binding, the descriptor's
layout and the constants match the header; the grid query answers without a device; every misuse is refused before anything is
launched; the fp64 statement the GPU tests compare against (tests/attn_branch_bwd_ref.py) agrees with the chain the oracle already
pins; functional routes by the switch and by what the ops module offers."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import attn_branch_bwd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, NH, WS, N = 96, 3, 7, 49


def _raw_header():
    return open(os.path.join(ROOT, "include", "esvit_hip.h")).read()


def test_boundary_binding_and_descriptor_layout(lib_built):
    from esvit_amd import _lib, ops
    raw = _raw_header()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(esvit_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 60 and declared == set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("esvit_")} == declared
    decl = re.search(r"int esvit_attn_branch_fwd\((.*?)\);", hdr, flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    res, argtypes = _lib.SIGNATURES["esvit_attn_branch_fwd"]
    assert len(args) == len(argtypes) == 29
    assert [a.split()[-1].lstrip("*") for a in args[-2:]] == ["stream", "bwd"] and "esvit_attn_bwd_desc" in args[-1]
    for a, t in zip(args, argtypes):
        want = _lib.vp if ("*" in a or "esvit_stream_t" in a) else (_lib.f32 if a.startswith("float") else _lib.C.c_int)
        assert t is want, (a, t)
    # the struct of the header, field by field, against the ctypes Structure and the offsets the header documents
    body = re.search(r"typedef struct esvit_attn_bwd_desc \{(.*?)\} esvit_attn_bwd_desc;", hdr, flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    names = [f.split()[-1].lstrip("*") for f in fields]
    assert names == [n for n, _ in ops.AttnBwdDesc._fields_]
    for f, (n, t) in zip(fields, ops.AttnBwdDesc._fields_):
        assert t is (ctypes.c_void_p if "*" in f else ctypes.c_int32), f
    documented = {m.group(2): int(m.group(1)) for m in re.finditer(r"(?:\*|,)?\s+(\d+) ([A-Za-z_]+)\b", " ".join(
        l for l in raw.splitlines() if re.match(r" \*\s+\d+ [a-zA-Z]", l)))}
    for n in names:
        assert getattr(ops.AttnBwdDesc, n).offset == documented[n], (n, getattr(ops.AttnBwdDesc, n).offset, documented.get(n))
    assert ctypes.sizeof(ops.AttnBwdDesc) == 136
    assert "#define ESVIT_Q_ATTN_BWD_FUSED_GRID %d" % ops.Q_ATTN_BWD_FUSED_GRID in raw
    assert "#define ESVIT_ATTN_BWD_PARTIAL_FLOATS %d" % ops.ATTN_BWD_PARTIAL_FLOATS in raw
    assert ops.ATTN_BWD_PARTIAL_FLOATS == 3 * C * C + C * C + 3 * C + 3 * C and ops.Q_ATTN_BWD_FUSED_GRID == 18


def test_grid_query_answers_without_a_device(lib_built):
    from esvit_amd import ops
    q = lambda dt, Cc, w: ops.query(ops.Q_ATTN_BWD_FUSED_GRID, dt, Cc, w)  # noqa: E731
    assert q(1, 96, 1) == 1 and q(1, 96, 7) == 7  # one workgroup per window ...
    big = q(1, 96, 1 << 20)
    assert 0 < big <= 1024 and big == q(1, 96, 1 << 21) and q(1, 96, big + 1) == big  # ... capped by the chip, not by the window count
    for dt, Cc in ((0, 96), (1, 192), (1, 128), (1, 64)):
        assert q(dt, Cc, 64) == 0
    assert q(1, 96, 0) == 0 and q(1, 96, 1 << 22) == 0
    assert ops.attn_branch_bwd_grid(torch.bfloat16, 96, 5) == 5 and ops.attn_branch_bwd_grid(torch.float32, 96, 5) == 0
    assert ops.attn_branch_bwd_supported(torch.bfloat16, 96, 3, 49, 49 * 4, 4)
    assert not ops.attn_branch_bwd_supported(torch.float32, 96, 3, 49, 196, 4)     # fp32 activations
    assert not ops.attn_branch_bwd_supported(torch.bfloat16, 192, 6, 49, 196, 4)   # C = 192
    assert not ops.attn_branch_bwd_supported(torch.bfloat16, 192, 3, 49, 196, 4)   # head_dim 64
    assert not ops.attn_branch_bwd_supported(torch.bfloat16, 96, 3, 196, 196, 1)   # 14x14 windows
    assert not ops.attn_branch_bwd_supported(torch.bfloat16, 96, 3, 49, 1 << 24, 4)  # rows beyond the 2 GiB buffer ranges


def test_every_misuse_is_refused_before_any_launch(lib_built):
    """on a host without a GPU: ESVIT_ERR_ARG for each argument check, the sentinel-filled outputs untouched (a call that passed its
    checks would launch, so only refused calls are made here)"""
    from esvit_amd import ops
    from esvit_amd._lib import lib
    nB, nW, L = 2, 4, 196
    rows = nB * L
    f32 = lambda *s: torch.full(s, 7.0)  # noqa: E731
    b16 = lambda *s: torch.full(s, 7.0, dtype=torch.bfloat16)  # noqa: E731
    t = dict(x=f32(rows, C), g1=f32(C), b1=f32(C), Wq=b16(3 * C, C), bqkv=f32(3 * C), Wp=b16(C, C), w2t=torch.zeros(nW * N, dtype=torch.int32),
             frag=f32(2, NH, 4096), table=f32(169, NH), y=f32(rows, C), xw=b16(rows, C))
    grid = nB * nW
    d = dict(gin=f32(rows, C), rowscale_out=None, gx=f32(rows, C), gx_act=b16(rows, C), WqkvT=b16(C, 3 * C), dWqkv=f32(3 * C, C), dbqkv=f32(3 * C),
             dWproj=f32(C, C), dbproj=f32(C), dgamma=f32(C), dbeta=f32(C), dbias_ws=f32(grid, NH, 4096), partials_ws=f32(grid, ops.ATTN_BWD_PARTIAL_FLOATS),
             first_partial=0, finish=grid, index=torch.zeros(N * N, dtype=torch.int64), dtable=f32(169, NH), table_rows=169)
    keep = [v for v in list(t.values()) + list(d.values()) if torch.is_tensor(v) and v.is_floating_point()]
    p = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())  # noqa: E731

    def call(**kw):
        a = dict(dtype=1, nH=NH, N=N, ws=WS, table=None, y=None, xw=None)
        a.update({k: v for k, v in kw.items() if k in a})
        f = dict(d)
        f.update({k: v for k, v in kw.items() if k in d})
        desc = ops.AttnBwdDesc(*[(f[n] if isinstance(f[n], int) else (None if f[n] is None else f[n].data_ptr())) for n, _ in ops.AttnBwdDesc._fields_])
        return lib.esvit_attn_branch_fwd(a["dtype"], p(t["x"]), p(t["g1"]), p(t["b1"]), 1e-6, p(t["Wq"]), p(t["bqkv"]), p(t["Wp"]), None, p(t["w2t"]), L,
                                         p(a["table"]), a["ws"], p(t["frag"]), None, nW, nB, a["N"], a["nH"], 32 ** -0.5, None, p(a["y"]), p(a["xw"]), None,
                                         None, None, None, None, ctypes.byref(desc))

    bad = [{k: None} for k in ("gin", "gx", "WqkvT", "dWqkv", "dbqkv", "dWproj", "dbproj", "dgamma", "dbeta", "dbias_ws", "partials_ws")]
    bad += [dict(y=t["y"]), dict(xw=t["xw"]), dict(table=t["table"]), dict(dtype=0), dict(nH=6), dict(nH=2), dict(N=36, ws=6), dict(N=196, ws=14), dict(N=49, ws=6),
            dict(finish=grid - 1), dict(first_partial=1), dict(first_partial=-1), dict(finish=-1), dict(index=None), dict(table_rows=0),
            dict(partials_ws=d["partials_ws"].view(-1)[1:]), dict(dbias_ws=d["dbias_ws"].view(-1)[1:]), dict(gx=d["gx"].view(-1)[1:]),
            dict(gin=d["gin"].view(-1)[1:]), dict(gx_act=d["gx_act"].view(-1)[1:]), dict(WqkvT=d["WqkvT"].view(-1)[1:])]
    for kw in bad:
        assert call(**kw) == -1, kw  # ESVIT_ERR_ARG
        assert lib.esvit_last_error()
    for v in keep:
        assert bool((v.float() == 7.0).all())


def _oracle_chain(ref, x, gin, g1, b1, Wqkv, bqkv, Wproj, bproj, table, nB, H, shift, rs):
    """the present chain, composed from oracle.ops_ref in fp32 mode (what functional runs on the CPU stand-in)"""
    L = H * H
    w2t = torch.from_numpy(ref.window_maps(H, H, WS, shift)[0])
    reg = torch.from_numpy(ref.shift_region_ids(H, H, WS, shift)) if shift else None
    nW = w2t.numel() // N
    index = torch.from_numpy(ref.relative_position_index(WS))
    scale = 32 ** -0.5
    xw, _, mean, rstd = ref.layernorm_fwd(x, g1, b1, 1e-6)
    qkv = ref.linear_fwd(xw, Wqkv, bqkv)
    ao, lse = ref.window_attn_fwd(qkv, bqkv, w2t, L, table, WS, reg, nW, N, NH, scale)
    dyw = gin if rs is None else gin * rs[:, None]
    dWproj, dbproj = ref.linear_wgrad(dyw, ao, want_bias=True)
    dao = ref.linear_dgrad(dyw, Wproj)
    dqkv, dbias_ws, dpad = ref.window_attn_bwd(qkv, bqkv, w2t, L, dao, ao, lse, table, WS, reg, nW, N, NH, scale)
    dtable = ref.relpos_bias_bwd(dbias_ws, index, N, table.shape[0])
    dWqkv, dbqkv = ref.linear_wgrad(dqkv, xw, want_bias=True)
    ref.colsum(dpad, out=dbqkv[C:], accumulate=True)
    dxw = ref.linear_dgrad(dqkv, Wqkv)
    gx, dg1, db1 = ref.layernorm_bwd(dxw, x, mean, rstd, g1, g_in=gin)
    return dict(gx=gx, dgamma=dg1, dbeta=db1, dWqkv=dWqkv, dbqkv=dbqkv, dWproj=dWproj, dbproj=dbproj, dtable=dtable)


@pytest.mark.parametrize("H,shift,nB", [(7, 0, 2), (14, 3, 2), (12, 3, 3)])
def test_fp64_statement_agrees_with_the_pinned_chain(lib_built, H, shift, nB):
    """fp32 mode; bound: 1e-3 of each tensor's maximum, the relative bound tests/test_composition_cpu.py:285 holds the oracle step's
    gradients to against the reference's"""
    from oracle import ops_ref as ref
    ref.set_act_dtype(torch.float32)
    g = torch.Generator().manual_seed(40 + H)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    rows = nB * H * H
    x, gin = r(rows, C) + 0.1 * r(1, C), 0.5 * r(rows, C)
    g1, b1 = 1 + 0.1 * r(C), 0.1 * r(C)
    Wqkv, bqkv, Wproj, bproj, table = r(3 * C, C) * C ** -0.5, 0.5 * r(3 * C), r(C, C) * C ** -0.5, 0.5 * r(C), 0.5 * r(169, NH)
    rs = ((torch.rand(nB, generator=g) > 0.4).float() / 0.6).repeat_interleave(H * H)
    rs[:H * H] = 0.0
    for scale_rows in (None, rs):
        want = R.branch_grads(x, gin, g1, b1, Wqkv, bqkv, Wproj, bproj, table, nB, H, H, WS, shift, NH, scale_rows)
        got = _oracle_chain(ref, x, gin, g1, b1, Wqkv, bqkv, Wproj, bproj, table, nB, H, shift, scale_rows)
        assert set(got) == set(R.NAMES)
        for k in R.NAMES:
            sc = want[k].abs().max().item() + 1e-12
            err = (got[k].double() - want[k]).abs().max().item() / sc
            assert err <= 1e-3, (k, err)


class _Stub:
    """an ops module: oracle.ops_ref with some functions replaced and some forbidden"""

    def __init__(self, ref, **over):
        self._ref, self._over = ref, over

    def __getattr__(self, name):
        if name in self._over:
            v = self._over[name]
            if v is None:
                raise AttributeError(name)
            return v
        return getattr(self._ref, name)


def _block_setup(monkeypatch, fused, offer, emit_shadow=True):
    """a ragged stage-0 block over a 14-map (shifted) and a 12-map (padded) on the CPU stand-in, bf16 activations; the stub records
    the attention-branch calls.  -> (calls, run) where run() does forward + backward and returns (parameter list, sinks, gradients)"""
    import esvit_amd.functional as Fn
    import esvit_amd.params as P
    from oracle import ops_ref as ref
    calls = []
    chain = ("window_attn_bwd", "relpos_bias_bwd", "layernorm_bwd", "layernorm_bwd_cast", "colsum")

    def rec(name, fn):
        return lambda *a, **k: (calls.append((name, a, k)), fn(*a, **k))[1]

    def attn_branch_bwd(x, gin, gamma, beta, eps, weights, bqkv, win2tok, L, ws, region_ids, nW, N_, nH, scale, *, bias_frag, rowscale=None, rowscale_out=None,
                        out=None, workspaces=None, first_partial=0, finish=True, gx_out=None, gx_act_out=None, index=None, dtable=None,
                        table_rows=0):
        calls.append(("attn_branch_bwd", (x, gin), dict(out=out, first_partial=first_partial, finish=finish, gx_act_out=gx_act_out, rowscale=rowscale,
                                                         rowscale_out=rowscale_out, dtable=dtable, workspaces=workspaces, shapes=[tuple(w.shape) for w in weights])))
        outs = [o_ if o_ is not None else torch.zeros(s) for o_, s in zip(out, ((3 * C, C), (3 * C,), (C, C), (C,), (C,), (C,)))]
        if finish:
            for k, o_ in enumerate(outs):
                o_.fill_(float(k + 1))
            dtable = dtable if dtable is not None else torch.zeros(table_rows, nH)
            dtable.fill_(9.0)
        gx_out.fill_(5.0)
        if gx_act_out is not None:
            gx_act_out.fill_(6.0)
        return gx_out, gx_act_out, tuple(outs), workspaces[1], (dtable if finish else None)

    over = {n: rec(n, getattr(ref, n)) for n in chain + ("attn_branch_fwd", "linear_wgrad", "linear_dgrad")}
    if offer:
        over.update(attn_branch_bwd=attn_branch_bwd,
                    attn_branch_bwd_supported=lambda dt, Cc, nH, N_, rows=0, windows=1: dt == torch.bfloat16 and Cc == 96 and nH == 3 and N_ == 49 and rows < 10 ** 6,
                    attn_branch_bwd_workspaces=lambda windows, nH, dev: (torch.zeros(sum(windows), 4), torch.zeros(sum(windows), nH, 8),
                                                                        [sum(windows[:i]) for i in range(len(windows))]))
    stub = _Stub(ref, **over)
    for mod in (Fn, P):
        monkeypatch.setattr(mod, "ops", stub)
    monkeypatch.setattr(Fn, "ATTN_BWD_FUSED", fused)
    ref.set_act_dtype(torch.bfloat16)
    P.clear()
    Fn._GEOM.clear()
    g = torch.Generator().manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    prm = [torch.nn.Parameter(t) for t in (1 + 0.1 * r(C), 0.1 * r(C), 0.2 * r(169, NH), r(3 * C, C) * C ** -0.5, 0.1 * r(3 * C), r(C, C) * C ** -0.5, 0.1 * r(C),
                                           1 + 0.1 * r(C), 0.1 * r(C), 0.08 * r(4 * C, C), 0.1 * r(4 * C), 0.05 * r(C, 4 * C), 0.1 * r(C))]
    segs = ((0, 2, 196, Fn.geometry(14, 14, WS, 3, torch.device("cpu"))), (392, 1, 144, Fn.geometry(12, 12, WS, 3, torch.device("cpu"))))
    M = 392 + 144
    X = r(M, C).requires_grad_(True)
    index = torch.from_numpy(ref.relative_position_index(WS))
    dp_rows = ((torch.rand(M, generator=g) > 0.2).float() / 0.8, (torch.rand(M, generator=g) > 0.2).float() / 0.8)
    prev_scale = torch.rand(M, generator=g)

    def run():
        sinks = {id(p_): torch.zeros_like(p_) for p_ in prm}
        P.set_grad_sink(sinks)
        try:
            saved = []
            with torch.autograd.graph.saved_tensors_hooks(lambda t_: (saved.append(t_), t_)[1], lambda t_: t_):
                shadow = torch.empty(M, C, dtype=torch.bfloat16, requires_grad=True) if emit_shadow else None
                y, ysh, _ = Fn.swin_block_multi(X, segs, NH, index, dp_rows, prm, shadow, prev_scale if emit_shadow else None)
            grads = torch.autograd.grad((y * r(M, C)).sum(), [X] + ([shadow] if emit_shadow else []) + prm, allow_unused=True)
        finally:
            P.set_grad_sink(None)
            ref.set_act_dtype(torch.float32)
            P.clear()
            Fn._GEOM.clear()
        return prm, sinks, grads, saved
    return calls, run


def _names(calls):
    return [c[0] for c in calls]


@pytest.mark.parametrize("fused,offer", [(False, True), (True, False)])
def test_switch_off_or_cpu_stand_in_keeps_the_chain(lib_built, monkeypatch, fused, offer):
    from oracle import ops_ref
    assert not hasattr(ops_ref, "attn_branch_bwd")
    calls, run = _block_setup(monkeypatch, fused, offer)
    prm, sinks, grads, saved = run()
    names = _names(calls)
    fwd = [c for c in calls if c[0] == "attn_branch_fwd"]
    assert len(fwd) == 2 and all(c[2]["save"] for c in fwd)  # side outputs on
    assert "attn_branch_bwd" not in names and names.count("window_attn_bwd") == 2 and "relpos_bias_bwd" in names and "layernorm_bwd_cast" in names
    assert any(t_.dtype == torch.bfloat16 and tuple(t_.shape) == (536, 3 * C) for t_ in saved)  # qkv is saved


def test_default_is_off():
    import importlib
    import esvit_amd.functional as Fn
    if "ESVIT_ATTN_BWD_FUSED" not in os.environ:
        assert Fn.ATTN_BWD_FUSED is False
    src = open(os.path.join(ROOT, "esvit_amd", "functional.py")).read()
    assert 'ATTN_BWD_FUSED = os.environ.get("ESVIT_ATTN_BWD_FUSED", "0") == "1"' in src
    assert importlib.util.find_spec("oracle.ops_ref") is not None


@pytest.mark.parametrize("emit_shadow", [True, False])
def test_new_route_replaces_the_chain_and_hands_over_the_slots(lib_built, monkeypatch, emit_shadow):
    calls, run = _block_setup(monkeypatch, True, True, emit_shadow)
    prm, sinks, grads, saved = run()
    names = _names(calls)
    fwd = [c for c in calls if c[0] == "attn_branch_fwd"]
    assert len(fwd) == 2 and not any(c[2]["save"] for c in fwd)  # no side outputs
    for forbidden in ("window_attn_bwd", "relpos_bias_bwd", "layernorm_bwd", "layernorm_bwd_cast", "colsum"):
        assert forbidden not in names, forbidden
    bwd = [c[2] for c in calls if c[0] == "attn_branch_bwd"]
    assert len(bwd) == 2
    # the groups stack their partials and share one reduce; the weight copies are the plain cast, its transpose, the transposed proj
    assert [b["first_partial"] for b in bwd] == [0, 8] and [b["finish"] for b in bwd] == [False, True]
    assert bwd[0]["workspaces"][0] is bwd[1]["workspaces"][0] and bwd[0]["shapes"] == [(3 * C, C), (C, 3 * C), (C, C)]
    g1_p, b1_p, table_p, Wqkv_p, bqkv_p, Wproj_p, bproj_p = prm[:7]
    for b in bwd:
        for got, p_ in zip(b["out"], (Wqkv_p, bqkv_p, Wproj_p, bproj_p, g1_p, b1_p)):
            assert got is sinks[id(p_)]
        assert b["rowscale"] is not None and b["rowscale"].shape[0] in (392, 144)
        assert (b["gx_act_out"] is not None) == emit_shadow and (b["rowscale_out"] is not None) == emit_shadow  # the shadow copy only when wanted
    assert bwd[1]["dtable"] is sinks[id(table_p)]
    # every gradient is handed over as a fresh alias of its armed slot
    off = 2 if emit_shadow else 1
    assert bool((grads[0] == 5.0).all()) and (not emit_shadow or bool((grads[1].float() == 6.0).all()))
    for k, (p_, val) in enumerate(((Wqkv_p, 1.0), (bqkv_p, 2.0), (Wproj_p, 3.0), (bproj_p, 4.0), (g1_p, 5.0), (b1_p, 6.0), (table_p, 9.0))):
        got = grads[off + [id(q) for q in prm].index(id(p_))]
        assert got.data_ptr() == sinks[id(p_)].data_ptr() and got is not sinks[id(p_)] and bool((got == val).all()), k
    # nothing of the side outputs is saved
    assert not any(t_.dtype == torch.bfloat16 and tuple(t_.shape) == (536, 3 * C) for t_ in saved)


def test_unsupported_shapes_fall_back(lib_built, monkeypatch):
    import esvit_amd.functional as Fn
    from oracle import ops_ref as ref
    stub = _Stub(ref, attn_branch_bwd=lambda *a, **k: None,
                 attn_branch_bwd_supported=lambda dt, Cc, nH, N_, rows=0, windows=1: dt == torch.bfloat16 and Cc == 96 and nH == 3 and N_ == 49 and rows < 1000)
    monkeypatch.setattr(Fn, "ATTN_BWD_FUSED", True)
    g7 = Fn.geometry(14, 14, 7, 0, torch.device("cpu"))
    g14 = Fn.geometry(14, 14, 14, 0, torch.device("cpu"))
    Fn._GEOM.clear()
    ok = lambda dt, Cc, nH, gs, sizes: Fn._attn_bwd_fused(stub, dt, Cc, nH, gs, sizes)  # noqa: E731
    assert ok(torch.bfloat16, 96, 3, (g7,), [(392, 8)])
    assert not ok(torch.float32, 96, 3, (g7,), [(392, 8)])       # fp32 mode
    assert not ok(torch.bfloat16, 192, 6, (g7,), [(392, 8)])     # C = 192
    assert not ok(torch.bfloat16, 96, 3, (g14,), [(392, 2)])     # W = 14
    assert not ok(torch.bfloat16, 96, 3, (g7, g7), [(392, 8), (5000, 100)])  # an oversized call
    assert not Fn._attn_bwd_fused(ref, torch.bfloat16, 96, 3, (g7,), [(392, 8)])  # the CPU stand-in offers no such op
    monkeypatch.setattr(Fn, "ATTN_BWD_FUSED", False)
    assert not ok(torch.bfloat16, 96, 3, (g7,), [(392, 8)])
