"""Swin backbones on H x W images on the MI355X: the pad mode of the PatchMerging kernels (ESVIT_MERGE_PAD, csrc/norm.hip) against the
fp64 merge of tests/norm_ref.py applied to the zero-padded grid, under that file's derived bounds, with its exact properties; the model
against the fp64 statement tests/swin_rect_ref.py under both settings of functional.MERGE_PAD; the ragged multi-crop route on
rectangular and on odd maps; the attention entropies of a rectangular image put back on the picture.  Observed figures go to
golden_utils.record_parity; the device run is committed as profiles/swin_rect_parity_observed.jsonl, a record only."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref
from tests import golden_utils as GU
from tests import norm_ref as NR
from tests import swin_rect_ref as SR
from tests.test_swin_rect_cpu import build, inputs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS = 1e-6
GRIDS = [(1, 1), (1, 9), (9, 1), (7, 5), (15, 25), (8, 13), (14, 14)]
WIDTHS = (32, 96, 512)  # 4 C = 128, 384, 2048: ln kernels <32,1>, <32,3>, <64,8>
BATCHES = (1, 3)
OUT = {"fp32": 2e-5, "bf16": 3e-2}  # tests/test_variants.py:test_odd_patch_merging_gpu; five times that for gradients


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


# ---- the merge kernels in pad mode ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def merge_case(nB, H, W, Cin, dt):
    """inputs on the CPU and the fp64 merge of norm_ref on the zero-padded grid, with norm_ref's bounds: the derived ones, or 3 x the error
    of the fp32 restatement (oracle/ops_ref on the padded grid) where that is larger (tests/norm_ref.py, "Device rsqrtf ...")"""
    key = ("swin_rect", nB, H, W, Cin)
    C, Hp, Wp = 4 * Cin, H + H % 2, W + W % 2
    rows, tokens = nB * (Hp // 2) * (Wp // 2), nB * H * W
    x = NR.data(key + ("x",), (nB, H, W, Cin)) * 1.5 + 0.3
    xp = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H))
    live = F.pad(torch.ones(nB, H, W), (0, Wp - W, 0, Hp - H)).bool().reshape(-1)
    src = NR.merge_rows(nB, Hp, Wp)
    xg = xp.reshape(-1, Cin).double()[src].reshape(rows, C)
    rs = NR.data(key + ("rs",), (tokens,)).abs() + 0.5
    if nB > 1:
        rs[(nB - 1) * H * W:] = 0.0  # one sample with the factor 0
    else:
        rs[0] = 0.0
    mean = xg.mean(1)
    rstd = (((xg - mean[:, None]) ** 2).mean(1) + NR._f32(EPS)) ** -0.5
    i = dict(x=x.reshape(nB, H * W, Cin).contiguous(), xp=xp.reshape(nB, Hp * Wp, Cin).contiguous(), gamma=1.0 + NR.data(key + ("g",), (C,), scale=0.2),
             beta=NR.data(key + ("b",), (C,), scale=0.1), dy=NR.data(key + ("dy",), (rows, C), dt), dy2=NR.data(key + ("dy2",), (rows, C), dt),
             mean=mean.float(), rstd=rstd.float(), rowscale=rs, gb_prev=NR.data(key + ("gbp",), (2, C)), live=live)
    f64 = lambda t: t.double()  # noqa: E731
    ref = {}
    fw = NR.ln_forward(xg, f64(i["gamma"]), f64(i["beta"]), NR._f32(EPS), C, dt)
    NR._put(ref, fw, ("mean", "rstd", "y"))
    bw = NR.ln_backward(xg, f64(i["dy"]), f64(i["mean"]), f64(i["rstd"]), f64(i["gamma"]), C)
    b2 = NR.ln_backward(xg, f64(i["dy2"]), f64(i["mean"]), f64(i["rstd"]), f64(i["gamma"]), C, accumulate=True)
    NR._put(ref, bw, ("dgamma", "dbeta"))
    for p in ("", "ab_", "bd_"):  # the scatter to the padded token rows, then the crop: every live token is written once
        buf = torch.zeros(nB * Hp * Wp, Cin, dtype=torch.float64)
        buf[src.reshape(-1)] = bw[p + "dx"].reshape(rows * 4, Cin)
        ref[p + "dx"] = buf[live]
    one = torch.ones(tokens, 1, dtype=torch.float64)
    ref["act"], ref["bd_act"] = NR.act_copy(ref["dx"], ref["bd_dx"], one, dt)
    ref["act_rs"], ref["bd_act_rs"] = NR.act_copy(ref["dx"], ref["bd_dx"], f64(rs).view(-1, 1), dt)
    for k in ("dgamma", "dbeta"):
        ref["acc_" + k] = bw[k] + b2[k]
        ref["bd_acc_" + k] = bw["bd_" + k] + b2["bd_" + k] + NR.U * (bw[k].abs() + b2[k].abs())
    # the restatement's error on the padded grid (fp32 activations), as tests/norm_ref.py:_reference takes it
    o, st = ops_ref, (i["xp"], i["mean"], i["rstd"], i["gamma"], Hp, Wp)
    got = {}
    got["y"], got["mean"], got["rstd"] = o.merge_ln_fwd(i["xp"], i["gamma"], i["beta"], EPS, Hp, Wp, dtype=torch.float32)
    act = torch.zeros(nB * Hp * Wp, Cin)
    dxp, got["dgamma"], got["dbeta"] = o.merge_ln_bwd(i["dy"].float(), *st, act_out=act)
    got["dx"], got["act"] = dxp.reshape(-1, Cin)[live], act[live].clone()
    rsp = torch.zeros(nB * Hp * Wp)
    rsp[live] = rs
    o.merge_ln_bwd(i["dy"].float(), *st, act_out=act, rowscale=rsp)
    got["act_rs"] = act[live].clone()
    gb = i["gb_prev"].clone()
    o.merge_ln_bwd(i["dy"].float(), *st, gb_out=gb, accumulate=False)
    o.merge_ln_bwd(i["dy2"].float(), *st, gb_out=gb, accumulate=True)
    got["acc_dgamma"], got["acc_dbeta"] = gb[0], gb[1]
    for k, v in got.items():
        err = (v.double() - ref[k]).abs()
        err = torch.where(torch.isfinite(err), err, torch.zeros_like(err))
        if err.dim() == 2:
            err = err.amax(1, keepdim=True).expand_as(err)
        ref["bd_" + k] = torch.maximum(ref["bd_" + k], 3 * err)
    return i, ref


def _moated(t, moat, fill=float("nan")):
    """t [n, C] inside a buffer with `moat` rows of `fill` on both sides -> (buffer, view)"""
    n, Cc = t.shape
    buf = torch.full((n + 2 * moat, Cc), fill, dtype=t.dtype, device=DEV)
    buf[moat:moat + n] = t.to(DEV)
    return buf, buf[moat:moat + n]


def _moat_ok(buf, moat):
    return bool((buf[:moat] == NR.SENTINEL).all()) and bool((buf[-moat:] == NR.SENTINEL).all())


def _pad_mode_run(ops, i, nB, H, W, Cin, dt, rowscale=None, x=None):
    """forward and backward in pad mode, every output inside sentinel moats -> dict of device tensors + moats intact"""
    C = 4 * Cin
    rows, tokens, M = nB * ((H + 1) // 2) * ((W + 1) // 2), nB * H * W, 2 * W + 4
    x = i["x"].to(DEV) if x is None else x
    ybuf = torch.full((rows + 4, C), NR.SENTINEL, dtype=dt, device=DEV)
    sbuf = torch.full((2, rows + 4), NR.SENTINEL, dtype=torch.float32, device=DEV)
    ops.merge_ln_fwd(x, i["gamma"].to(DEV), i["beta"].to(DEV), EPS, H, W, dtype=dt, out=(ybuf[2:-2], sbuf[0, 2:-2], sbuf[1, 2:-2]), pad=True)
    dxb = torch.full((tokens + 2 * M, Cin), NR.SENTINEL, dtype=torch.float32, device=DEV)
    acb = torch.full((tokens + 2 * M, Cin), NR.SENTINEL, dtype=dt, device=DEV)
    gb = torch.full((4, C), NR.SENTINEL, dtype=torch.float32, device=DEV)
    gb[1:3] = i["gb_prev"].to(DEV)
    ops.merge_ln_bwd(i["dy"].to(DEV), x, i["mean"].to(DEV), i["rstd"].to(DEV), i["gamma"].to(DEV), H, W, dx_out=dxb[M:-M], gb_out=gb[1:3],
                     act_out=acb[M:-M], rowscale=rowscale, pad=True)
    torch.cuda.synchronize()
    ok = (_moat_ok(ybuf, 2) and bool((sbuf[:, :2] == NR.SENTINEL).all()) and bool((sbuf[:, -2:] == NR.SENTINEL).all()) and _moat_ok(dxb, M)
          and _moat_ok(acb, M) and bool((gb[0] == NR.SENTINEL).all()) and bool((gb[3] == NR.SENTINEL).all()))
    return dict(y=ybuf[2:-2].clone(), mean=sbuf[0, 2:-2].clone(), rstd=sbuf[1, 2:-2].clone(), dx=dxb[M:-M].clone(), act=acb[M:-M].clone(),
                dgamma=gb[1].clone(), dbeta=gb[2].clone(), gb=gb), ok


@pytest.mark.parametrize("dt", NR.DTYPES, ids=NR.dt_name)
@pytest.mark.parametrize("hw", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("Cin", WIDTHS)
def test_merge_pad_mode(ops, Cin, hw, dt):
    H, W = hw
    Hp, Wp = H + H % 2, W + W % 2
    for nB in BATCHES:
        i, ref = merge_case(nB, H, W, Cin, dt)
        tokens = nB * H * W
        # x in a NaN moat on both sides: a read of a pad quadrant of the last sample's bottom row shows in the statistics
        _, xv = _moated(i["x"].reshape(tokens, Cin), 2 * W + 4)
        x = xv.view(nB, H * W, Cin)
        got, moats = _pad_mode_run(ops, i, nB, H, W, Cin, dt, x=x)
        again, _ = _pad_mode_run(ops, i, nB, H, W, Cin, dt, x=x)
        rsd, _ = _pad_mode_run(ops, i, nB, H, W, Cin, dt, rowscale=i["rowscale"].to(DEV), x=x)
        got["act_rs"] = rsd["act"]
        gb = got.pop("gb")
        ops.merge_ln_bwd(i["dy2"].to(DEV), x, i["mean"].to(DEV), i["rstd"].to(DEV), i["gamma"].to(DEV), H, W, gb_out=gb[1:3], accumulate=True, pad=True)
        got["acc_dgamma"], got["acc_dbeta"] = gb[1].clone(), gb[2].clone()
        m = {"ratio_" + k: NR.ratio(got[k].detach().cpu().double(), ref[k], ref["bd_" + k]) for k in NR.outputs(ref)}
        m["equal_moats"] = float(moats)
        m["equal_repeat"] = float(all(torch.equal(got[k], again[k]) for k in again if k != "gb"))
        zero = slice((nB - 1) * H * W, None) if nB > 1 else slice(0, 1)
        m["equal_rowscale_zero"] = float(bool((got["act_rs"][zero] == 0).all()))
        # the same kernel with zeros substituted at the load: the bits of pad_crop_tokens + the plain call (on an even grid: of the plain call)
        d = {k: i[k].to(DEV) for k in ("dy", "mean", "rstd", "gamma", "beta")}
        xp = x if (Hp, Wp) == (H, W) else ops.pad_crop_tokens(x.reshape(tokens, Cin), nB, H, W, Hp, Wp).view(nB, Hp * Wp, Cin)
        y, mean, rstd = ops.merge_ln_fwd(xp, d["gamma"], d["beta"], EPS, Hp, Wp, dtype=dt)
        actp = torch.empty((nB * Hp * Wp, Cin), dtype=dt, device=DEV)
        dxp, dg, db = ops.merge_ln_bwd(d["dy"], xp, d["mean"], d["rstd"], d["gamma"], Hp, Wp, act_out=actp)
        dxp = dxp.reshape(-1, Cin)
        if (Hp, Wp) != (H, W):
            dxp, actp = ops.pad_crop_tokens(dxp, nB, Hp, Wp, H, W), ops.pad_crop_tokens(actp, nB, Hp, Wp, H, W)
        plain = dict(y=y, mean=mean, rstd=rstd, dx=dxp, act=actp, dgamma=dg, dbeta=db)
        m["equal_plain_route"] = float(all(torch.equal(got[k], plain[k]) for k in plain))
        tag = dict(test="swin_rect_merge_pad", Cin=Cin, grid=[H, W], nB=nB, dtype=NR.dt_name(dt))
        GU.record_parity(**tag, **m)
        bad = NR.failures(m)
        assert not bad, (tag, bad)


@pytest.mark.parametrize("dt", NR.DTYPES, ids=NR.dt_name)
def test_merge_pad_mode_refusals_write_nothing(ops, dt):
    def sent(*shape, dtype=torch.float32):
        return torch.full(shape, NR.SENTINEL, dtype=dtype, device=DEV)

    def refused(fn, *tensors):
        with pytest.raises(RuntimeError, match="failed"):
            fn()
        torch.cuda.synchronize()
        for t in tensors:
            assert bool((t == NR.SENTINEL).all())
    ops.workspace(1 << 20, DEV, slot=1)
    for (nB, H, W, Cin) in ((1, 32768, 1, 4), (1, 1, 32768, 4), (1, 7, 5, 6)):  # a side past the packed form's range; C % 4 != 0
        rows, C = nB * ((H + 1) // 2) * ((W + 1) // 2), 4 * Cin
        x = torch.ones(nB, H * W, Cin, device=DEV)
        gamma, st = torch.ones(C, device=DEV), torch.ones(rows, device=DEV)
        y, mean, rstd = sent(rows, C, dtype=dt), sent(rows), sent(rows)
        refused(lambda: ops.merge_ln_fwd(x, gamma, gamma, EPS, H, W, dtype=dt, out=(y, mean, rstd), pad=True), y, mean, rstd)
        dy = torch.ones(rows, C, dtype=dt, device=DEV)
        dx, gb, act = sent(nB * H * W, Cin), sent(2, C), sent(nB * H * W, Cin, dtype=dt)
        refused(lambda: ops.merge_ln_bwd(dy, x, st, st, gamma, H, W, dx_out=dx, gb_out=gb, act_out=act, pad=True), dx, gb, act)


# ---- the model against the fp64 statement -----------------------------------------------------------------------------------------------
def _model_errors(cfg, name, H, W, prec, mode, monkeypatch):
    """relative L2 error of cls, region and every parameter gradient against the statement -> dict"""
    import esvit_amd
    import esvit_amd.functional as Fn
    monkeypatch.setattr(Fn, "MERGE_PAD", mode)
    esvit_amd.set_precision(prec)
    try:
        m = build(cfg)
        x, pr = inputs(H, W, m.num_features)
        want = SR.run((name, H, W, None), m.state_dict(), x, cfg, pr)
        m = m.to(DEV)
        cls, region = m.forward_features(x.to(DEV))
        assert region.shape == want["region"].shape and m.feature_grid(H, W) == want["grids"]
        SR.loss_of(cls, region, pr.to(DEV)).backward()
        torch.cuda.synchronize()
        errs = dict(cls=SR.rel(cls, want["cls"]), region=SR.rel(region, want["region"]))
        grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        assert set(grads) == set(want["grads"])
        g = {n: SR.rel(v, want["grads"][n]) for n, v in grads.items()}
        errs["grad_name"] = max(g, key=g.get)
        errs["grad"] = g[errs["grad_name"]]
        return errs
    finally:
        esvit_amd.set_precision("bf16")


_SQUARE = {}


def _check_model(cfg, name, H, W, prec, mode, monkeypatch, square):
    """the project's figures; a quantity that needs more is allowed at most twice what the square case of the same model, precision and
    setting shows (both numbers are recorded)"""
    e = _model_errors(cfg, name, H, W, prec, mode, monkeypatch)
    bound = dict(cls=OUT[prec], region=OUT[prec], grad=5 * OUT[prec])
    rec = dict(test="swin_rect_model", model=name, image=[H, W], prec=prec, merge_pad=mode, worst_grad=e["grad_name"],
               **{"ratio_" + k: e[k] / bound[k] for k in bound})
    over = [k for k in bound if not e[k] < bound[k]]
    if over:
        key = (name, prec, mode)
        if key not in _SQUARE:
            _SQUARE[key] = _model_errors(cfg, name, square, square, prec, mode, monkeypatch)
        sq = _SQUARE[key]
        rec.update(square_image=[square, square], **{"observed_" + k: e[k] for k in over}, **{"square_observed_" + k: sq[k] for k in over})
    GU.record_parity(**rec)
    for k in over:
        assert e[k] <= 2 * _SQUARE[(name, prec, mode)][k], (k, e[k], bound[k], _SQUARE[(name, prec, mode)][k])


@pytest.mark.parametrize("mode", ["copy", "kernel"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("hw", [(112, 80), (60, 100), (4, 36)], ids=lambda g: "%dx%d" % g)
def test_nano_model_matches_statement(lib_built, monkeypatch, hw, prec, mode):
    _check_model(GU.NANO, "nano", hw[0], hw[1], prec, mode, monkeypatch, square=112)


@pytest.mark.parametrize("mode", ["copy", "kernel"])
def test_two_stage_96_model_matches_statement_bf16(lib_built, monkeypatch, mode):
    """the fused attention-branch and fused MLP kernels (C = 96 / 192) on a padded, shifted, rectangular grid: 14 x 21, then 7 x 11"""
    _check_model(SR.NANO2_96, "two_stage_96", 56, 84, "bf16", mode, monkeypatch, square=56)


# ---- the ragged multi-crop route ------------------------------------------------------------------------------------------------------------
def _forward_backward(m, crops, pr):
    m.zero_grad()
    seen = []
    orig = m.forward_feature_maps_multi
    m.forward_feature_maps_multi = lambda groups: (seen.append([len(g) for g in groups]), orig(groups))[1]
    try:
        cls, fea_head, fea, npatch = m(crops)
    finally:
        m.forward_feature_maps_multi = orig
    ((cls * pr).sum() + fea.sum() * 0.01).backward()
    torch.cuda.synchronize()
    return (cls.detach(), fea.detach()), npatch, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}, seen


def _crops(spec, B=2):
    g = torch.Generator().manual_seed(77)
    return [torch.randn(B, 3, H, W, generator=g).to(DEV) for (n, H, W) in spec for _ in range(n)]


def _ragged_case(monkeypatch, spec, mode, tol=2e-5):
    """fp32, the bounds of tests/test_step_gpu.py:test_ragged_multi_crop_equals_reference_schedule_gpu (check_ragged_equals_reference_schedule):
    outputs tol of their range, gradients 20 tol.  -> the groups each forward handed to the ragged route ([] : per-group schedule)"""
    import esvit_amd
    import esvit_amd.functional as Fn
    monkeypatch.setattr(Fn, "MERGE_PAD", mode)
    esvit_amd.set_precision("fp32")
    try:
        m = build(GU.NANO).to(DEV)
        m.head = m.head_dense = torch.nn.Identity()
        crops = _crops(spec)
        pr = torch.randn(sum(c.shape[0] for c in crops), m.num_features, generator=torch.Generator().manual_seed(5)).to(DEV)
        res = []
        for ragged in (True, False):
            m.ragged_multi_crop = ragged
            res.append(_forward_backward(m, crops, pr))
        (oa, na, ga, sa), (ob, nb, gb, sb) = res
        assert na == nb and sb == []
        worst = dict(out=0.0, grad=0.0)
        for a, b in zip(oa, ob):
            assert a.shape == b.shape
            worst["out"] = max(worst["out"], (a - b).abs().max().item() / (tol * (b.abs().max().item() + 1e-12)))
        assert ga.keys() == gb.keys()
        for n in ga:
            worst["grad"] = max(worst["grad"], (ga[n] - gb[n]).abs().max().item() / (20 * tol * (gb[n].abs().max().item() + 1e-12)))
        GU.record_parity(test="swin_rect_ragged", crops=[list(s) for s in spec], merge_pad=mode, route=sa, **{"ratio_" + k: v for k, v in worst.items()})
        assert worst["out"] <= 1 and worst["grad"] <= 1, worst
        return sa, na
    finally:
        esvit_amd.set_precision("bf16")


def test_ragged_route_on_rectangular_crops(lib_built, monkeypatch):
    """[2 x (64, 96), 6 x (32, 48)]: the local crops' 8 x 12 grid reaches 2 x 3 at the four-stage model's last merge, an odd map, so this
    list rides the ragged route under "kernel"; under the default "copy" a list whose maps stay even does ([2 x (64, 96), 3 x (32, 96)],
    the list of tests/test_swin_rect_cpu.py: 16 x 24 and 8 x 24)"""
    route, npatch = _ragged_case(monkeypatch, [(2, 64, 96), (6, 32, 48)], "kernel")
    assert route == [[2, 6]] and npatch == [2 * 3, 1 * 2]
    route, npatch = _ragged_case(monkeypatch, [(2, 64, 96), (3, 32, 96)], "copy")
    assert route == [[2, 3]] and npatch == [2 * 3, 1 * 3]
    route, npatch = _ragged_case(monkeypatch, [(2, 64, 96), (6, 32, 48)], "copy")
    assert route == [] and npatch == [2 * 3, 1 * 2]


def test_ragged_route_takes_odd_maps_in_kernel_mode(lib_built, monkeypatch):
    route, npatch = _ragged_case(monkeypatch, [(2, 60, 100), (4, 28, 44)], "kernel")
    assert route == [[2, 4]] and npatch == [2 * 4, 1 * 2]  # 15 x 25 -> 8 x 13 -> 4 x 7 -> 2 x 4;  7 x 11 -> 4 x 6 -> 2 x 3 -> 1 x 2


def test_odd_maps_keep_the_per_group_schedule_in_copy_mode(lib_built, monkeypatch):
    route, npatch = _ragged_case(monkeypatch, [(2, 60, 100), (4, 28, 44)], "copy")
    assert route == [] and npatch == [2 * 4, 1 * 2]


# ---- analysis -----------------------------------------------------------------------------------------------------------------------------
def test_swin_entropy_of_rectangular_images_on_the_grid(lib_built):
    """fp32 precision.  (1) as tests/test_attn_stats_gpu.py holds the square case: the entropies ARE the reduction of the model's own
    window maps, bit for bit.  (2) put back on the picture with swin_window_to_grid they meet the entropies of the statement's fp64
    maps (put back by the statement's own reverse / roll / crop): an attention probability of the fp32 path is held to 3e-4 relative
    (tests/test_step_gpu.py, "last_attn"); p -> p (1 + e) moves -p log2 p by at most e p (|log2 p| + log2 e), so a row's entropy moves
    by at most 3e-4 (H + log2 e) bits"""
    import esvit_amd
    from esvit_amd import analysis as A
    esvit_amd.set_precision("fp32")
    try:
        m = build(GU.NANO)
        sd = SR.to64(m.state_dict())
        m = m.to(DEV).eval()
        g = torch.Generator().manual_seed(9)
        batches = [torch.randn(2, 3, 80, 112, generator=g), torch.randn(1, 3, 60, 100, generator=g)]
        single = A.attention_entropy(m, batches[0].to(DEV))
        both = A.attention_entropy(m, [b.to(DEV) for b in batches])
        assert len(both) == 2 and all(torch.equal(a, b) for a, b in zip(single, both[0]))
        worst = 0.0
        for x, ent in zip(batches, both):
            with torch.no_grad():
                maps = m.forward_selfattention(x.to(DEV), n=2)
                _, _, ref_maps, _ = SR.features(sd, x.double(), GU.NANO)
            geo = SR.block_geometry(GU.NANO, x.shape[-2] // 4, x.shape[-1] // 4)
            assert len(ent) == len(maps) == len(geo) == sum(GU.NANO["depths"])
            blocks = [b for layer in m.layers for b in layer.blocks]
            for e, p, r, (H, W, ws, shift), blk in zip(ent, maps, ref_maps, geo, blocks):
                assert (blk.window_size, blk.shift_size) == (ws, shift)
                assert torch.equal(e, torch.special.entr(p.float()).sum(-1) / math.log(2.0))
                on_grid = A.swin_window_to_grid(e, H, W, ws, shift)
                want = SR.slots_to_grid(torch.special.entr(r).sum(-1) / math.log(2.0), H, W, ws, shift)
                assert on_grid.shape == want.shape == (x.shape[0], p.shape[1], H, W)
                worst = max(worst, ((on_grid.double().cpu() - want).abs() / (3e-4 * (want + math.log2(math.e)))).max().item())
        GU.record_parity(test="swin_rect_entropy", images=[list(b.shape[-2:]) for b in batches], ratio_entropy=worst)
        assert worst <= 1, worst
        per = A.AttentionEntropyMeter().update(m, [b.to(DEV) for b in batches]).compute()
        assert len(per) == sum(GU.NANO["depths"])
    finally:
        esvit_amd.set_precision("bf16")
