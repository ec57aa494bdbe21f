"""-m gpu: the backward mode of the fused attention branch (esvit_attn_branch_fwd with a descriptor; bf16, C = 96, 7x7 windows) against
fp64 autograd of the branch (tests/attn_branch_bwd_ref.py), with the present chain of the same build on the same inputs as the yardstick
of what a bf16 pipeline loses.  Geometries: one window, shifted, padded, padded + shifted, the 96^2 crop's stage-0 map, 128 windows,
more windows than twice the grid with a ragged last pass (the grid is asked of the library), and two resolution groups that stack
their partials and finish once.  Each with and without DropPath row factors that contain zeros."""
import ctypes
import json
import math
import os

import pytest
import torch

from tests import attn_branch_bwd_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, NH, WS, N = 96, 3, 7, 49
SCALE = 32 ** -0.5
DT = torch.bfloat16
OUTS = ("gx", "dWqkv", "dbqkv", "dWproj", "dbproj", "dgamma", "dbeta", "dtable", "gx_act")
# sums of bf16-rounded rows in fp32: where the present route is itself at summation noise the ratio of two such errors means nothing; the
# fixed bound is the one tests/test_kernels_gpu.py:178 ("wgrad(+bias) db", bf16: 2e-3 of the tensor's maximum) holds a bias sum to
BIAS_SUMS = {"dbqkv": 2e-3, "dbproj": 2e-3, "dbeta": 2e-3}
# every output of either bf16 pipeline, against fp64: the bound tests/test_kernels_gpu.py:530-532 holds dqkv and dtable to
ABS_BOUND = 3e-2
_OBSERVED = []


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops as o
    old = o.act_dtype()
    o.set_act_dtype(DT)
    yield o
    o.set_act_dtype(old)


@pytest.fixture(scope="module", autouse=True)
def _write_observed():
    yield
    if _OBSERVED:
        try:
            with open(os.path.join(ROOT, "profiles", "attn_bwd_parity_observed.jsonl"), "w") as f:
                for rec in _OBSERVED:
                    f.write(json.dumps(rec) + "\n")
        except OSError:
            pass  # (a read-only checkout: the figures are in the assertion messages)


def _groups(ops, case):
    """(H, shift, nB) of every resolution group of a case"""
    if case == "ragged":
        G = ops.attn_branch_bwd_grid(DT, C, 1 << 20)  # the grid of a launch with more windows than workgroups
        assert G > 0
        return [(12, 3, (2 * G) // 4 + 1)]  # 4 windows per image: every workgroup loops at least twice, the last pass is ragged
    if case == "two":
        return [(56, 0, 1), (24, 3, 2)]
    return [case]


CASES = [(7, 0, 1), (14, 3, 3), (12, 0, 2), (12, 3, 5), (24, 3, 9), (56, 0, 2), "ragged", "two"]
PARAMS = [(i, dp) for i in range(len(CASES)) for dp in (False, True)]
_CACHE = {}


def _present_chain(ops, X, gin, segs, prm, rs, rs_out, frag, index):
    """the chain SwinBlockMultiFn.backward runs today, from ops.*: side outputs of the fused forward, then proj weight- and data-gradient
    GEMMs, window_attn_bwd per group, ONE relpos_bias_bwd, the qkv weight gradient with the pad rows' column sums, the qkv data
    gradient, layernorm_bwd_cast"""
    g1, b1, Wqkv, bqkv, Wproj, bproj, table = prm
    M = X.shape[0]
    dev = X.device
    Wq_p, Wp_p = ops.cast_weight(Wqkv, perm32=True), ops.cast_weight(Wproj, perm32=True)
    xw, qkv, ao = (torch.empty((M, k * C), dtype=DT, device=dev) for k in (1, 3, 1))
    mean, rstd = torch.empty((M,), device=dev), torch.empty((M,), device=dev)
    y = torch.empty_like(X)
    for (r0, nB, L, w2t, reg, nW) in segs:
        r1 = r0 + nB * L
        ops.attn_branch_fwd(X[r0:r1], g1, b1, 1e-6, Wq_p, bqkv, Wp_p, bproj, w2t, L, None, WS, reg, nW, N, NH, SCALE, rowscale=None if rs is None else rs[r0:r1],
                            out=y[r0:r1], bias_frag=frag, save=(xw[r0:r1], mean[r0:r1], rstd[r0:r1], qkv[r0:r1], ao[r0:r1]))
    dyw = (gin if rs is None else gin * rs[:, None]).to(DT)
    dWproj, dbproj = ops.linear_wgrad(dyw, ao, want_bias=True)
    dao = ops.linear_dgrad(dyw, Wproj.to(DT))
    dqkv = torch.empty_like(qkv)
    dbuf, dslabs = ops.attn_dbias_slabs(N, [nB * nW for (_, nB, _, _, _, nW) in segs], NH, dev)
    pads = []
    for (r0, nB, L, w2t, reg, nW), dslab in zip(segs, dslabs):
        r1 = r0 + nB * L
        _, _, pad = ops.window_attn_bwd(qkv[r0:r1], bqkv, w2t, L, dao[r0:r1], ao[r0:r1], None, None, WS, reg, nW, N, NH, SCALE, dqkv_out=dqkv[r0:r1],
                                        bias_frag=frag, dbias_out=dslab)
        pads.append(pad)
    dtable = ops.relpos_bias_bwd(dbuf, index, N, table.shape[0])
    dWqkv, dbqkv = ops.linear_wgrad(dqkv, xw, want_bias=True)
    for pad in pads:
        ops.colsum(pad, out=dbqkv[C:], accumulate=True)
    dxw = ops.linear_dgrad(dqkv, Wqkv.to(DT))
    gx, gxb, dg1, db1 = ops.layernorm_bwd_cast(dxw, X, mean, rstd, g1, g_in=gin, rowscale=rs_out, rows_per_sample=1)
    return dict(gx=gx, dWqkv=dWqkv, dbqkv=dbqkv, dWproj=dWproj, dbproj=dbproj, dgamma=dg1, dbeta=db1, dtable=dtable, gx_act=gxb), y


def _new_route(ops, X, gin, segs, prm, rs, rs_out, frag, index):
    g1, b1, Wqkv, bqkv, Wproj, bproj, table = prm
    dev = X.device
    weights = ops.attn_branch_bwd_weights(Wqkv, Wproj)
    part, dbias, firsts = ops.attn_branch_bwd_workspaces([nB * nW for (_, nB, _, _, _, nW) in segs], NH, dev)
    gx, gxa = torch.empty_like(X), torch.empty(X.shape, dtype=DT, device=dev)
    outs = None
    for i, (r0, nB, L, w2t, reg, nW) in enumerate(segs):
        r1 = r0 + nB * L
        _, _, outs, _, dtable = ops.attn_branch_bwd(X[r0:r1], gin[r0:r1], g1, b1, 1e-6, weights, bqkv, w2t, L, WS, reg, nW, N, NH, SCALE, bias_frag=frag,
                                            rowscale=None if rs is None else rs[r0:r1], rowscale_out=None if rs_out is None else rs_out[r0:r1], out=outs,
                                            workspaces=(part, dbias), first_partial=firsts[i], finish=i == len(segs) - 1, gx_out=gx[r0:r1],
                                            gx_act_out=gxa[r0:r1], index=index, table_rows=table.shape[0])
    dWqkv, dbqkv, dWproj, dbproj, dg1, db1 = outs
    return dict(gx=gx, dWqkv=dWqkv, dbqkv=dbqkv, dWproj=dWproj, dbproj=dbproj, dgamma=dg1, dbeta=db1, dtable=dtable, gx_act=gxa)


def _case(ops, i, dp):
    """inputs, three launches of the new route, the present chain and the fp64 reference of one case, computed once"""
    key = (i, dp)
    if key in _CACHE:
        return _CACHE[key]
    dev = _dev()
    groups = _groups(ops, CASES[i])
    segs, geo, r0 = [], [], 0
    for (H, shift, nB) in groups:
        w2t = torch.from_numpy(ops.window_maps(H, H, WS, shift)[0]).to(dev)
        reg = torch.from_numpy(ops.shift_region_ids(H, H, WS, shift)).to(dev) if shift else None
        segs.append((r0, nB, H * H, w2t, reg, w2t.numel() // N))
        geo.append((r0, nB, H, shift))
        r0 += nB * H * H
    M = r0
    X = _rand((M, C), dev, 60) + 0.1 * _rand((1, C), dev, 61)
    gin = _rand((M, C), dev, 59, 0.5)
    g1, b1 = 1.0 + 0.1 * _rand((C,), dev, 62), 0.1 * _rand((C,), dev, 63)
    # (weights that bf16 holds exactly: both routes and the fp64 reference see the same numbers)
    Wqkv, bqkv = (_rand((3 * C, C), dev, 64) * C ** -0.5).to(DT).float(), _rand((3 * C,), dev, 65) * 0.5
    Wproj, bproj = (_rand((C, C), dev, 66) * C ** -0.5).to(DT).float(), _rand((C,), dev, 67) * 0.5
    table = _rand(((2 * WS - 1) ** 2, NH), dev, 68) * 0.5
    index = torch.from_numpy(ops.relative_position_index(WS)).to(dev)
    rs = rs_out = None
    if dp:  # DropPath row factors per image, images with factor 0 among them; a group of ONE image gets zeros on the first third of its rows
        gen = torch.Generator().manual_seed(69)
        per, per_out = [], []
        for (_, nB, L, _, _, _) in segs:
            k = (torch.rand(nB, generator=gen) > 0.3).float() / 0.7
            k[0], k[-1] = 0.0, 1.0 / 0.7
            k = k.repeat_interleave(L)
            if nB == 1:
                k[:L // 3] = 0.0
            assert bool((k == 0).any()) and bool((k > 0).any())
            per.append(k)
            per_out.append(((torch.rand(nB, generator=gen) > 0.2).float() / 0.8).repeat_interleave(L))
        rs, rs_out = torch.cat(per).to(dev), torch.cat(per_out).to(dev)
    prm = (g1, b1, Wqkv, bqkv, Wproj, bproj, table)
    frag = ops.new_bias_frag(NH, N, dev)
    s0 = segs[0]
    ops.attn_branch_fwd(X[:s0[1] * s0[2]], g1, b1, 1e-6, ops.cast_weight(Wqkv, perm32=True), bqkv, ops.cast_weight(Wproj, perm32=True), bproj, s0[3], s0[2],
                        table, WS, s0[4], s0[5], N, NH, SCALE, bias_frag=frag)  # (fills the fragment-order bias)
    runs = [{k: v.clone() for k, v in _new_route(ops, X, gin, segs, prm, rs, rs_out, frag, index).items()} for _ in range(3)]
    old, _ = _present_chain(ops, X, gin, segs, prm, rs, rs_out, frag, index)
    torch.cuda.synchronize()
    exact = None
    for (q0, nB, H, shift) in geo:
        q1 = q0 + nB * H * H
        gr = R.branch_grads(X[q0:q1], gin[q0:q1], g1, b1, Wqkv, bqkv, Wproj, bproj, table, nB, H, H, WS, shift, NH, None if rs is None else rs[q0:q1])
        if exact is None:
            exact = gr
        else:
            exact = {k: (torch.cat([exact[k], v]) if k == "gx" else exact[k] + v) for k, v in gr.items()}
    exact["gx_act"] = exact["gx"] if rs_out is None else exact["gx"] * rs_out.double().cpu()[:, None]
    out = dict(runs=runs, old=old, exact=exact, M=M, windows=[s[1] * s[5] for s in segs])
    _CACHE[key] = out
    return out


@pytest.mark.parametrize("i,dp", PARAMS)
def test_gradients_against_fp64_and_the_present_chain(ops, i, dp):
    c = _case(ops, i, dp)
    pairs = {}
    for name in OUTS:
        ex = c["exact"][name]
        scale = ex.abs().max().item() + 1e-12
        new, old = c["runs"][0][name].double().cpu(), c["old"][name].double().cpu()
        assert new.shape == ex.shape and bool(torch.isfinite(new).all()), name
        pairs[name] = ((new - ex).abs().max().item() / scale, (old - ex).abs().max().item() / scale)
    _OBSERVED.append(dict(case=str(CASES[i]), rows=c["M"], windows=c["windows"], droppath=dp,
                          rel_err_new_vs_present={k: [float("%.4e" % a), float("%.4e" % b)] for k, (a, b) in pairs.items()}))
    print("case=%s dp=%s" % (CASES[i], dp), {k: "%.3e / %.3e" % v for k, v in pairs.items()})
    for name, (e_new, e_old) in pairs.items():
        assert math.isfinite(e_new) and e_new <= ABS_BOUND, "%s: rel err %.3e > %.1e vs fp64" % (name, e_new, ABS_BOUND)
    for name, (e_new, e_old) in pairs.items():
        # the margin tests/test_mlp_dw_gpu.py uses for a changed summation order
        bound = max(1.5 * e_old, BIAS_SUMS.get(name, 0.0))
        assert e_new <= bound, "%s: rel err %.3e in one kernel vs %.3e on the present chain (case %s)" % (name, e_new, e_old, CASES[i])


@pytest.mark.parametrize("i,dp", PARAMS)
def test_three_launches_are_identical(ops, i, dp):
    c = _case(ops, i, dp)
    for k in (1, 2):
        for name in OUTS:
            assert torch.equal(c["runs"][k][name], c["runs"][0][name]), "%s differs between launch 0 and launch %d" % (name, k)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _raw(ops, a, desc):
    """the raw entry over the argument dict a; desc: an ops.AttnBwdDesc or None"""
    from esvit_amd._lib import lib
    return lib.esvit_attn_branch_fwd(a.get("dtype", 1), _p(a["x"]), _p(a["g1"]), _p(a["b1"]), 1e-6, _p(a["Wq"]), _p(a["bqkv"]), _p(a["Wp"]), _p(a.get("bproj")),
                                     _p(a["w2t"]), a["L"], _p(a.get("table")), WS, _p(a["frag"]), None, a["nW"], a["nB"], a.get("N", N), a.get("nH", NH), SCALE,
                                     None, _p(a.get("y")), _p(a.get("xw")), None, None, None, None,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None if desc is None else ctypes.byref(desc))


def _raw_inputs(ops, H=14, nB=2):
    dev = _dev()
    w2t = torch.from_numpy(ops.window_maps(H, H, WS, 0)[0]).to(dev)
    L = H * H
    x = _rand((nB * L, C), dev, 80)
    g1, b1 = 1.0 + 0.1 * _rand((C,), dev, 81), 0.1 * _rand((C,), dev, 82)
    Wqkv, bqkv = _rand((3 * C, C), dev, 83) * C ** -0.5, _rand((3 * C,), dev, 84) * 0.5
    Wproj, bproj = _rand((C, C), dev, 85) * C ** -0.5, _rand((C,), dev, 86) * 0.5
    table = _rand(((2 * WS - 1) ** 2, NH), dev, 87) * 0.5
    frag = ops.new_bias_frag(NH, N, dev)
    return dict(x=x, g1=g1, b1=b1, Wqkv=Wqkv, bqkv=bqkv, Wproj=Wproj, bproj=bproj, table=table, frag=frag, w2t=w2t, L=L, nW=w2t.numel() // N, nB=nB)


def test_null_descriptor_is_the_forward(ops):
    a = _raw_inputs(ops)
    a["Wq"], a["Wp"] = ops.cast_weight(a["Wqkv"], perm32=True), ops.cast_weight(a["Wproj"], perm32=True)
    want = ops.attn_branch_fwd(a["x"], a["g1"], a["b1"], 1e-6, a["Wq"], a["bqkv"], a["Wp"], a["bproj"], a["w2t"], a["L"], a["table"], WS, None, a["nW"], N, NH, SCALE,
                               bias_frag=a["frag"])
    a["y"] = torch.zeros_like(a["x"])
    assert _raw(ops, a, None) == 0
    assert torch.equal(a["y"], want)


def test_argument_checks_launch_nothing(ops):
    a = _raw_inputs(ops)
    dev = _dev()
    a["Wq"], WqT, a["Wp"] = ops.attn_branch_bwd_weights(a["Wqkv"], a["Wproj"])
    ops.attn_branch_fwd(a["x"], a["g1"], a["b1"], 1e-6, ops.cast_weight(a["Wqkv"], perm32=True), a["bqkv"], ops.cast_weight(a["Wproj"], perm32=True), a["bproj"],
                        a["w2t"], a["L"], a["table"], WS, None, a["nW"], N, NH, SCALE, bias_frag=a["frag"])
    a.pop("bproj")
    tbl = a.pop("table")
    grid = ops.attn_branch_bwd_grid(DT, C, a["nB"] * a["nW"])
    assert grid == a["nB"] * a["nW"]
    part, dbias, _ = ops.attn_branch_bwd_workspaces([a["nB"] * a["nW"]], NH, dev)
    part.fill_(7.0), dbias.fill_(7.0)
    gin = _rand(a["x"].shape, dev, 88)
    gx, gxa = torch.full_like(a["x"], 7.0), torch.full(a["x"].shape, 7.0, dtype=DT, device=dev)
    grads = [torch.full(s, 7.0, device=dev) for s in ((3 * C, C), (3 * C,), (C, C), (C,), (C,), (C,))]
    y = torch.full_like(a["x"], 7.0)

    def desc(**kw):
        f = dict(gin=gin, rowscale_out=None, gx=gx, gx_act=gxa, WqkvT=WqT, dWqkv=grads[0], dbqkv=grads[1], dWproj=grads[2], dbproj=grads[3], dgamma=grads[4],
                 dbeta=grads[5], dbias_ws=dbias, partials_ws=part, first_partial=0, finish=grid, index=None, dtable=None, table_rows=0)
        f.update(kw)
        return ops.AttnBwdDesc(*[(f[n] if isinstance(f[n], int) else (None if f[n] is None else f[n].data_ptr())) for n, _ in ops.AttnBwdDesc._fields_])

    bad = [(a, desc(**{k: None})) for k in ("gin", "gx", "WqkvT", "dWqkv", "dbqkv", "dWproj", "dbproj", "dgamma", "dbeta", "dbias_ws", "partials_ws")]
    bad.append((dict(a, y=y), desc()))                       # a forward output together with the descriptor
    bad.append((dict(a, xw=gxa), desc()))                    # a side output together with the descriptor
    bad.append((dict(a, table=tbl), desc()))                # the bias fragments must already be filled
    bad.append((dict(a, dtype=0), desc()))                   # fp32 activations
    bad.append((dict(a, nH=6), desc()))                      # C = 192
    bad.append((dict(a, N=36), desc()))                      # not 7x7
    bad.append((a, desc(finish=grid - 1)))                   # finish leaves out partials of this call
    bad.append((a, desc(first_partial=1, finish=grid)))
    bad.append((a, desc(first_partial=-1)))
    bad.append((a, desc(dtable=grads[3])))                   # the table's gradient without its index
    bad.append((a, desc(partials_ws=part.view(-1)[1:])))     # unaligned workspaces
    bad.append((a, desc(dbias_ws=dbias.view(-1)[1:])))
    bad.append((a, desc(gx=gx.view(-1)[1:])))
    for args, d in bad:
        assert _raw(ops, args, d) == -1  # ESVIT_ERR_ARG
    torch.cuda.synchronize()
    for t in [gx, gxa, y, part, dbias] + grads:
        assert bool((t.float() == 7.0).all())  # nothing ran
    assert _raw(ops, a, desc()) == 0
    torch.cuda.synchronize()
    assert not bool((gx == 7.0).all()) and bool(torch.isfinite(gx).all())
    for cfg in ((0, 96), (1, 192), (1, 128)):
        assert ops.query(ops.Q_ATTN_BWD_FUSED_GRID, cfg[0], cfg[1], 64) == 0


def _step(dev, ragged, fused, monkeypatch):
    """one training step of a two-stage Swin (stage 0 at C = 96) on 2 x 112^2 + 2 x 48^2 crops: stage-0 maps 28 and 12 (padded)"""
    import esvit_amd.functional as Fn
    import esvit_amd.params as P
    from esvit_amd import models
    from oracle import ref_loader as RL
    from tests import golden_utils as GU
    monkeypatch.setattr(Fn, "ATTN_BWD_FUSED", fused)
    P.clear()
    cfg = RL.swin_config(embed_dim=96, depths=(2, 2), heads=(3, 6), window=7, drop_path=0.1)
    m = models.build_model(cfg, is_teacher=False, use_dense_prediction=True)
    m.head = models.DINOHead(m.num_features, 128, norm_last_layer=True, hidden_dim=64, bottleneck_dim=32)
    m.head_dense = models.DINOHead(m.num_features, 128, norm_last_layer=False, hidden_dim=64, bottleneck_dim=32)
    GU.fill_state_dict(m.state_dict(), 3)
    m.head.last_layer.weight_g.data.fill_(1)
    m = m.to(dev).train()
    m.ragged_multi_crop = ragged
    crops = [c.to(dev) for c in GU.make_crops(2, n_local=2, seed=11, sizes=(112, 48))]
    saved = []

    def pack(t):
        saved.append((tuple(t.shape), t.dtype))
        return t

    torch.manual_seed(17)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = m(crops)
    w = [_rand(tuple(o_.shape), dev, 90 + k) for k, o_ in enumerate(out[:2])]
    loss = sum((o_.float() * w_).sum() for o_, w_ in zip(out[:2], w))
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}, saved


# Largest (new route's error + present chain's error) against fp64 per output kind over the sixteen cases above, as recorded in
# profiles/attn_bwd_parity_observed.jsonl (rounded up): by the triangle inequality the two routes differ by at most this on the same inputs.
REC = dict(gx=1.25e-2, dWqkv=1.43e-2, dbqkv=7.4e-3, dWproj=8.3e-3, dbproj=4.3e-3, dgamma=1.69e-2, dbeta=1.27e-2, dtable=1.35e-2)
KIND = {"norm1.weight": "dgamma", "norm1.bias": "dbeta", "attn.relative_position_bias_table": "dtable", "attn.qkv.weight": "dWqkv",
        "attn.qkv.bias": "dbqkv", "attn.proj.weight": "dWproj", "attn.proj.bias": "dbproj"}
MARGIN = 1.5  # the step's activations and incoming gradients are not the kernel cases' inputs


def _step_bound(n):
    """bound on |on - off| / max|off| of parameter n of stage 0 / the patch embedding, or None where the two routes must agree to the bit.
    The backward runs downsample -> block 1 -> block 0 -> patch embedding; only the attention branches of blocks 1 and 0 differ between
    the routes.  Block 1's attention parameters see identical inputs: the recorded sum of their kind.  Everything upstream of block 1's
    attention branch receives a dL/dx that differs by at most REC[gx] of its maximum, and every later operator is the same linear map of
    that gradient in both routes, so its outputs differ by that relative amount (weight and bias gradients sum thousands of rows of
    independent rounding errors: far below it): block 0's MLP and norm2 parameters REC[gx], block 0's attention parameters their own kind's
    sum on top of it, the patch embedding the errors of both blocks' dL/dx."""
    if n.startswith("layers.0.downsample.") or (n.startswith("layers.0.blocks.1.") and not any(n.endswith(k) for k in KIND)):
        return None
    kind = next((v for k, v in KIND.items() if n.endswith(k)), None)
    if n.startswith("layers.0.blocks.1."):
        return MARGIN * REC[kind]
    if n.startswith("layers.0.blocks.0."):
        return MARGIN * (REC["gx"] + (REC[kind] if kind else 0.0))
    assert n.startswith("patch_embed.")
    return MARGIN * 2 * REC["gx"]


@pytest.mark.parametrize("ragged", [True, False])
def test_step_with_the_switch_on_against_off(ops, ragged, monkeypatch):
    import esvit_amd
    esvit_amd.set_precision("bf16")
    dev = _dev()
    l0, g0, s0 = _step(dev, ragged, False, monkeypatch)
    l1, g1, s1 = _step(dev, ragged, True, monkeypatch)
    # the forward's y does not depend on its side outputs (tests/test_kernels_gpu.py: test_attn_branch_fwd_is_bit_reproducible)
    assert l0 == l1
    assert g0.keys() == g1.keys()
    touched = 0
    for n in g0:
        early = n.startswith(("layers.0.", "patch_embed."))
        if not early and n.endswith("relative_position_bias_table"):
            # esvit_relpos_bias_bwd scatters with atomicAdd: two runs of the SAME route already differ in the last bits of a later stage's
            # table gradient (observed here with the switch off twice), so these tensors cannot be held to the bit by anything this file
            # tests.  Bound: <= 49 terms per entry summed in another order, 49 * 2^-24 = 3e-6 of the largest sum
            err = (g0[n] - g1[n]).abs().max().item() / (g0[n].abs().max().item() + 1e-12)
            assert err <= 3e-6, "%s: %.3e" % (n, err)
            continue
        bound = _step_bound(n) if early else None
        if bound is None:
            assert torch.equal(g0[n], g1[n]), n
            continue
        touched += 1
        scale = g0[n].abs().max().item() + 1e-12
        err = (g0[n] - g1[n]).abs().max().item() / scale
        print("%s: on vs off %.3e of the maximum (bound %.3e)" % (n, err, bound))
        assert math.isfinite(err) and bool(torch.isfinite(g1[n]).all()), n
        assert err <= bound, "%s: switch on vs off differ by %.3e of the tensor's maximum (bound %.3e)" % (n, err, bound)
    assert touched == 7 + 13 + 4  # block 1's attention parameters, block 0, the patch embedding
    # stage 0's side outputs over stage-0 rows -- bf16 [rows, 3C] (qkv), bf16 [rows, C] (LayerNorm output, attention output), fp32 [rows]
    # (mean, rstd) -- are saved with the switch off and gone with it on
    rows0 = {2 * 28 * 28 * 2, 2 * 12 * 12 * 2, 2 * 28 * 28 * 2 + 2 * 12 * 12 * 2}
    wide = lambda s: [x for x in s if x[1] == DT and len(x[0]) == 2 and x[0][0] in rows0 and x[0][1] == 3 * C]  # noqa: E731
    narrow = lambda s: [x for x in s if x[1] == DT and len(x[0]) == 2 and x[0][0] in rows0 and x[0][1] == C]  # noqa: E731
    stats = lambda s: [x for x in s if x[1] == torch.float32 and len(x[0]) == 1 and x[0][0] in rows0]  # noqa: E731
    print("saved off / on: qkv %d / %d, [rows, C] bf16 %d / %d, [rows] fp32 %d / %d" % (len(wide(s0)), len(wide(s1)), len(narrow(s0)), len(narrow(s1)),
                                                                                         len(stats(s0)), len(stats(s1))))
    blocks = len(wide(s0))  # one qkv per stage-0 block (ragged) or per block and group
    assert blocks > 0 and len(wide(s1)) == 0
    assert len(narrow(s0)) - len(narrow(s1)) == 2 * blocks and len(stats(s0)) - len(stats(s1)) == 2 * blocks
