"""-m gpu: the qkv-tail mode of esvit_layernorm_bwd (ops.attn_tail_bwd; bf16, C = 96) against the present chain of the same build
(linear_wgrad + linear_dgrad + layernorm_bwd[_cast], with xw from layernorm_fwd) and fp64 autograd of LayerNorm -> linear on the same
bf16-rounded dqkv and Wqkv.  Row counts: below one tile, a window, the tile edge, ragged tiles, fewer tiles than workgroups, and two
tiles per workgroup plus a ragged tail (the grid is asked of the library).  Every row count runs with and without row scales (zero
factors among them) and with and without the activation-dtype copy."""
import ctypes
import json
import math
import os

import pytest
import torch

from tests import attn_tail_ref as AR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 96
DT = torch.bfloat16
NAMES = ("gx", "dx_act", "dWqkv", "dbqkv", "dgamma", "dbeta")
_OBSERVED = []


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _write_observed():
    yield
    _CACHE.clear()  # (the cases' tensors: later test modules of the same process measure allocator peaks)
    torch.cuda.empty_cache()
    if _OBSERVED:
        try:
            with open(os.path.join(ROOT, "profiles", "attn_tail_parity_observed.jsonl"), "w") as f:
                for rec in _OBSERVED:
                    f.write(json.dumps(rec) + "\n")
        except OSError:
            pass  # (a read-only checkout: the figures are in the assertion messages)


def _row_counts(ops):
    G = ops.attn_tail_bwd_grid(DT, C, 1 << 40)  # the grid of a launch with more tiles than workgroups
    assert G > 0
    return [1, 49, 63, 64, 65, 64 * 3 + 37, 64 * (2 * G) + 77], G


CASES = [(i, rs, act) for i in range(7) for rs in (False, True) for act in (False, True)]
_CACHE = {}


def _case(ops, i, rs, act):
    """inputs, the new route (three launches), the present chain and the fp64 reference of one case, computed once.  Without the copy a
    row scale has nothing to scale: that case runs the chain's layernorm_bwd, the one with the copy its layernorm_bwd_cast"""
    key = (i, rs, act)
    if key in _CACHE:
        return _CACHE[key]
    dev = _dev()
    Ms, G = _row_counts(ops)
    M = Ms[i]
    a = AR.inputs(M, C, 90 + i, dev)
    rowscale = None
    if rs and act:  # DropPath row factors, rows with factor 0 among them
        rowscale = (torch.rand(M, generator=torch.Generator().manual_seed(77)) > 0.3).float().div(0.7).to(dev)
        rowscale[0] = 0.0
    # the statistics and xw as the forward's LayerNorm launch leaves them
    xw, _, mean, rstd = ops.layernorm_fwd(a["x"], a["gamma"], a["beta"], a["eps"], dtype=DT)
    runs = []
    for _ in range(3):
        out = ops.attn_tail_bwd(a["dqkv"], a["x"], mean, rstd, a["gamma"], a["beta"], a["Wqkv"], a["g_in"], rowscale=rowscale, rows_per_sample=1, want_act=act)
        runs.append(tuple(None if t is None else t.clone() for t in out))
    new = dict(zip(NAMES, runs[0]))
    # the present chain of the same build
    dW, db = ops.linear_wgrad(a["dqkv"], xw, want_bias=True)
    dxw = ops.linear_dgrad(a["dqkv"], a["Wqkv"])
    if act:
        gx, gxa, dg, dbt = ops.layernorm_bwd_cast(dxw, a["x"], mean, rstd, a["gamma"], g_in=a["g_in"], rowscale=rowscale, rows_per_sample=1)
    else:
        gx, dg, dbt = ops.layernorm_bwd(dxw, a["x"], mean, rstd, a["gamma"], g_in=a["g_in"])
        gxa = None
    old = dict(gx=gx, dx_act=gxa, dWqkv=dW, dbqkv=db, dgamma=dg.clone(), dbeta=dbt.clone())
    ex = AR.exact(a["dqkv"], a["x"], a["gamma"], a["beta"], a["Wqkv"], a["g_in"], a["eps"], rowscale, 1)
    want = AR.attn_tail_bwd(a["dqkv"], a["x"], mean, rstd, a["gamma"], a["beta"], a["Wqkv"], a["g_in"], rowscale, 1, act)
    out = dict(M=M, G=G, runs=runs, new=new, old=old, exact=ex, want=dict(zip(NAMES, want)), rowscale=rowscale)
    _CACHE[key] = out
    return out


@pytest.mark.parametrize("i,rs,act", CASES)
def test_against_fp64_and_the_present_chain(ops, i, rs, act):
    c = _case(ops, i, rs, act)
    pairs = {}
    for name in NAMES:
        if c["new"][name] is None:
            assert name == "dx_act" and not act
            continue
        ex = c["exact"][name]
        scale = ex.abs().max().item() + 1e-300
        e_new = (c["new"][name].double() - ex).abs().max().item() / scale
        e_old = (c["old"][name].double() - ex).abs().max().item() / scale
        pairs[name] = (e_new, e_old)
    _OBSERVED.append(dict(M=c["M"], grid=c["G"], rowscale=rs, dx_act=act,
                          rel_err_new_vs_present={k: [float("%.4e" % a_), float("%.4e" % b_)] for k, (a_, b_) in pairs.items()}))
    print("M=%d rs=%s act=%s" % (c["M"], rs, act), {k: "%.3e / %.3e" % v for k, v in pairs.items()})
    for name, (e_new, e_old) in pairs.items():
        # both routes round the same quantities to bf16 and sum the same products in fp32: they differ in summation order only.  The
        # floor is for outputs where the chain sits at fp32 round-off
        assert math.isfinite(e_new) and e_new <= max(1.5 * e_old, 1e-6), "%s: rel err %.3e fused vs %.3e on the present chain (M=%d)" % (name, e_new, e_old, c["M"])
    if c["rowscale"] is not None:
        assert bool((c["new"]["dx_act"][0] == 0).all())  # a dropped row's copy is zero


@pytest.mark.parametrize("i,rs,act", CASES)
def test_three_launches_are_identical(ops, i, rs, act):
    c = _case(ops, i, rs, act)
    for k in (1, 2):
        for name, a_, r_ in zip(NAMES, c["runs"][k], c["runs"][0]):
            assert (a_ is None and r_ is None) or torch.equal(a_, r_), "%s differs between launch 0 and launch %d" % (name, k)


@pytest.mark.parametrize("i", [0, 4, 6])
def test_outputs_stay_inside_their_buffers(ops, i):
    """every output in the middle of a larger buffer of sentinels: the margins (and, past M, nothing) are untouched"""
    from esvit_amd._lib import lib
    dev = _dev()
    Ms, G = _row_counts(ops)
    M = Ms[i]
    a = AR.inputs(M, C, 90 + i, dev)
    _, _, mean, rstd = ops.layernorm_fwd(a["x"], a["gamma"], a["beta"], a["eps"], dtype=DT)
    PAD = 1024  # elements on either side (a multiple of 16 bytes in both dtypes)
    nws = ops.query(ops.Q_ATTN_TAIL_WS, 1, C, M) // 4
    sizes = dict(gx=(M * C, torch.float32), dx_act=(M * C, DT), dWqkv=(3 * C * C, torch.float32), dbqkv=(3 * C, torch.float32), dgamma=(C, torch.float32),
                 dbeta=(C, torch.float32), ws=(nws, torch.float32))
    bufs = {k: torch.full((n + 2 * PAD,), -77.0, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    inner = {k: bufs[k][PAD:PAD + sizes[k][0]] for k in sizes}
    rec = ops.LnQkvTail(a["Wqkv"].data_ptr(), a["beta"].data_ptr(), inner["dWqkv"].data_ptr(), inner["dbqkv"].data_ptr())
    rc = lib.esvit_layernorm_bwd(1, p(a["dqkv"]), p(a["x"]), p(mean), p(rstd), p(a["gamma"]), p(a["g_in"]), M, C, p(inner["gx"]), p(inner["dgamma"]),
                                 p(inner["dbeta"]), p(inner["ws"]), ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p), 0, ops.LN_BWD_QKV_TAIL, p(inner["dx_act"]), 1,
                                 None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[:PAD] == -77.0).all()) and bool((b[-PAD:] == -77.0).all()), "%s: a margin was written" % k
    ref = ops.attn_tail_bwd(a["dqkv"], a["x"], mean, rstd, a["gamma"], a["beta"], a["Wqkv"], a["g_in"], want_act=True)
    for name, r_ in zip(NAMES, ref):
        assert torch.equal(inner[name].view(r_.shape), r_), name
    assert nws == ops.attn_tail_bwd_grid(DT, C, M) * ops.ATTN_TAIL_PARTIAL_FLOATS and not bool((inner["ws"] == -77.0).any())  # every partial word is written


def test_the_restatement_holds_on_the_device(ops):
    """the torch restatement (tests/attn_tail_ref.py) states the same rounding points: within bf16 rounding of the row outputs and fp32
    summation error of the sums"""
    c = _case(ops, 5, True, True)
    for name, tol in (("gx", 2.0 ** -8), ("dx_act", 2.0 ** -7), ("dWqkv", 1e-3), ("dbqkv", 1e-5), ("dgamma", 1e-3), ("dbeta", 1e-3)):
        w = c["want"][name].double()
        err = (c["new"][name].double() - w).abs().max().item() / (w.abs().max().item() + 1e-300)
        assert err <= tol, (name, err)


def test_argument_checks_launch_nothing(ops):
    from esvit_amd._lib import lib
    dev = _dev()
    M = 77
    a = AR.inputs(M, C, 5, dev)
    outs = [torch.full(s, 7.0, device=dev) for s in ((M, C), (C,), (C,), (3 * C, C), (3 * C,))]
    ws = torch.full((ops.ATTN_TAIL_PARTIAL_FLOATS * 2,), 7.0, device=dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rec = ops.LnQkvTail(a["Wqkv"].data_ptr(), a["beta"].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr())
    rp = ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p)

    def call(dtype=1, Cc=C, tokens=0, g_in=a["g_in"]):
        return lib.esvit_layernorm_bwd(dtype, p(a["dqkv"]), p(a["x"]), p(a["mean"]), p(a["rstd"]), p(a["gamma"]), p(g_in), M, Cc, p(outs[0]), p(outs[1]), p(outs[2]),
                                       p(ws), rp, tokens, ops.LN_BWD_QKV_TAIL, None, 0, None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call(dtype=0) == -1 and call(Cc=192) == -1 and call(tokens=7) == -1 and call(g_in=None) == -1  # ESVIT_ERR_ARG
    torch.cuda.synchronize()
    for t in outs + [ws]:
        assert bool((t == 7.0).all())  # nothing ran
