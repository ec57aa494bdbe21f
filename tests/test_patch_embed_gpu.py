"""-m gpu: the fused patch embedding (ops.patch_embed_fwd / patch_embed_bwd / patch_embed_reduce) on the MI355X against the fp64 statement
of tests/patch_embed_ref.py, at every supported width and at the token counts of patch_embed_ref.SHAPES.  Every input lies inside a
NaN moat, every output and the partial workspace inside a sentinel pattern that must survive.  Bounds: patch_embed_ref's docstring.
The backward launches one workgroup per CU, at most one per 128-row tile, so no workgroup of a launch is without a tile; walk_uneven has
workgroups with two tiles beside workgroups with one.  ESVIT_PATCH_PARITY_OUT=<file> appends the observed ratios as JSON lines."""
import json
import os

import pytest
import torch

from tests import patch_embed_ref as R

pytestmark = pytest.mark.gpu
EPS = 1e-6  # functional.LN_EPS
WIDTHS = (96, 128, 192)
SENTINEL = -7.25
PAD = 1024  # elements of moat / sentinel on either side (a multiple of 16 bytes in every dtype)


def _log(test, case, E, **ratios):
    path = os.environ.get("ESVIT_PATCH_PARITY_OUT")
    print(test, case, E, " ".join("%s=%.3g" % kv for kv in ratios.items()))
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(test=test, case=case, E=E, **ratios)) + "\n")


def moat(t, dev):
    """a device copy of t with NaN on both sides"""
    buf = torch.full((t.numel() + 2 * PAD,), float("nan"), dtype=t.dtype, device=dev)
    buf[PAD:PAD + t.numel()] = t.reshape(-1).to(dev)
    return buf[PAD:PAD + t.numel()].view(t.shape)


class Guarded:
    """an output buffer inside a sentinel pattern"""

    def __init__(self, shape, dev):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.buf[PAD:PAD + n].view(shape)
        self.n = n

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.n:] == SENTINEL).all())


def _dev_inputs(imgs, W, bias, gamma, beta, dev):
    return [moat(im, dev) for im in imgs], moat(W.bfloat16(), dev), moat(bias, dev), moat(gamma, dev), moat(beta, dev)


def _run_fwd(ops, d_in, E, M, dev, stats=True):
    imgs, W, bias, gamma, beta = d_in
    x, mean, rstd = Guarded((M, E), dev), Guarded((M,), dev), Guarded((M,), dev)
    ops.patch_embed_fwd(imgs, W, bias, gamma, beta, EPS, out=(x.t, mean.t, rstd.t) if stats else (x.t, None, None))
    torch.cuda.synchronize()
    assert x.intact() and mean.intact() and rstd.intact()
    if not stats:
        assert bool((mean.t == SENTINEL).all()) and bool((rstd.t == SENTINEL).all())
    return x.t, mean.t, rstd.t


def _run_bwd(ops, d_in, gx, mean, rstd, E, dev):
    imgs, W, bias, gamma, _ = d_in
    nparts = ops.patch_embed_parts(E, imgs)
    ws = Guarded((nparts, 51 * E), dev)
    part, n = ops.patch_embed_bwd(imgs, W, bias, gamma, moat(gx, dev), moat(mean, dev), moat(rstd, dev), partials=ws.t)
    assert n == nparts
    outs = [Guarded(s, dev) for s in ((E, 48), (E,), (E,), (E,))]
    ops.patch_embed_reduce(part, n, E, out=[o.t for o in outs])
    torch.cuda.synchronize()
    assert ws.intact() and all(o.intact() for o in outs)
    assert not bool((ws.t == SENTINEL).all(1).any()) and bool(torch.isfinite(ws.t).all())  # every record was written
    return [o.t for o in outs]


@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("case", sorted(R.SHAPES))
def test_exact_inputs_against_the_statement(lib_built, case, E):
    """pixels and weights that make y exact: x, mean, rstd and the four gradients within 3 x the fp32 restatement's error"""
    from esvit_amd import ops
    dev = torch.device("cuda")
    cpu = R.exact_inputs(R.SHAPES[case], E, seed=len(case) + E)
    imgs, W, bias, gamma, beta = cpu
    M = sum(R.rows_of(imgs))
    x64, mean64, rstd64, _ = R.forward(*cpu, EPS)
    x32, mean32, rstd32, _ = R.forward(*cpu, EPS, dtype=torch.float32)
    d_in = _dev_inputs(*cpu, dev)
    x, mean, rstd = _run_fwd(ops, d_in, E, M, dev)
    rx = R.ratio(x, x64, R.bound(x64, x32))
    rm, rr = R.ratio(mean, mean64, R.bound(mean64, mean32)), R.ratio(rstd, rstd64, R.bound(rstd64, rstd32))
    x_only = _run_fwd(ops, d_in, E, M, dev, stats=False)[0]
    assert torch.equal(x_only, x)  # the pass without statistics writes the same x
    # the backward on its own: the statement's statistics rounded to fp32, a Gaussian upstream gradient
    gx = torch.randn(M, E, generator=torch.Generator().manual_seed(M + E))
    m32, r32 = mean64.float(), rstd64.float()
    ref = R.backward(imgs, W, bias, gamma, gx, m32, r32)
    res = R.backward(imgs, W, bias, gamma, gx, m32, r32, dtype=torch.float32)
    aW, ab = R.dya_flip_allowance(ref[4], res[4], R.cols_of(imgs))
    got = _run_bwd(ops, d_in, gx, m32, r32, E, dev)
    bounds = [R.bound(ref[0], res[0]) + aW, R.bound(ref[1], res[1]) + ab, R.bound(ref[2], res[2]), R.bound(ref[3], res[3])]
    rg = [R.ratio(g, r, b) for g, r, b in zip(got, ref[:4], bounds)]
    _log("exact_inputs", case, E, x=rx, mean=rm, rstd=rr, dW=rg[0], dbp=rg[1], dgamma=rg[2], dbeta=rg[3])
    assert rx <= 1 and rm <= 1 and rr <= 1, (rx, rm, rr)
    assert all(r <= 1 for r in rg), rg


def _exact_dya_case(shapes, E, seed):
    """gamma = 1, paired channels, gx = +a on channel 2 i and -a on 2 i + 1, mean in eighths, rstd a power of two: s1 = s2 = 0 exactly and
    dya = rstd gx is a small dyadic -- dW and dbp are sums of multiples of 1/32 below 2^24 / 32, exact in fp32 in any order"""
    imgs, W, bias, _, beta = R.exact_inputs(shapes, E, seed, paired=True)
    gamma = torch.ones(E)
    M = sum(R.rows_of(imgs))
    g = torch.Generator().manual_seed(seed + 1)
    a = torch.randint(-8, 9, (M, E // 2), generator=g).float() / 4
    gx = torch.stack([a, -a], 2).reshape(M, E)
    mean = torch.randint(-16, 17, (M,), generator=g).float() / 8
    rstd = 2.0 ** torch.randint(-1, 2, (M,), generator=g).float()
    return (imgs, W, bias, gamma, beta), gx, mean, rstd


@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("case", ["three_20x12", "two_res_mid_tile", "bwd_tile_p1", "seventeen_crops", "walk_3_tiles", "walk_uneven"])
def test_dw_and_dbp_are_exact_when_dya_is(lib_built, case, E):
    from esvit_amd import ops
    dev = torch.device("cuda")
    shapes = R.SHAPES.get(case) or R.WALK_SHAPES[case]
    cpu, gx, mean, rstd = _exact_dya_case(shapes, E, seed=7 + E)
    imgs, W, bias, gamma, beta = cpu
    ref = R.backward(imgs, W, bias, gamma, gx, mean, rstd)
    assert torch.equal(R.bf16_round(ref[4]), ref[4]) and float(ref[0].abs().max()) * 32 < 2 ** 24 and float(ref[1].abs().max()) * 8 < 2 ** 24
    if case in R.WALK_SHAPES:
        tiles, grid = -(-gx.shape[0] // ops.PATCH_EMBED_BWD_TILE), ops.patch_embed_parts(E, imgs)
        assert (tiles >= 3 * grid) if case == "walk_3_tiles" else (grid < tiles < 2 * grid), (tiles, grid)
    got = _run_bwd(ops, _dev_inputs(*cpu, dev), gx, mean, rstd, E, dev)
    assert torch.equal(got[0].double().cpu(), ref[0]) and torch.equal(got[1].double().cpu(), ref[1])
    res = R.backward(imgs, W, bias, gamma, gx, mean, rstd, dtype=torch.float32)
    rg = [R.ratio(got[i], ref[i], R.bound(ref[i], res[i])) for i in (2, 3)]
    _log("dya_exact", case, E, dgamma=rg[0], dbeta=rg[1])
    assert all(r <= 1 for r in rg), rg


@pytest.mark.parametrize("E", WIDTHS)
def test_three_launches_give_the_same_bits(lib_built, E):
    from esvit_amd import ops
    dev = torch.device("cuda")
    cpu = R.gaussian_inputs(R.SHAPES["route_ab"] + R.SHAPES["three_20x12"], E, seed=E)
    M = sum(R.rows_of(cpu[0]))
    d_in = _dev_inputs(*cpu, dev)
    gx = torch.randn(M, E, generator=torch.Generator().manual_seed(1))
    runs = []
    for _ in range(3):
        x, mean, rstd = _run_fwd(ops, d_in, E, M, dev)
        runs.append([x.clone(), mean.clone(), rstd.clone()] + [t.clone() for t in _run_bwd(ops, d_in, gx, mean.cpu(), rstd.cpu(), E, dev)])
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


@pytest.mark.parametrize("E", WIDTHS)
def test_against_the_unfused_route(lib_built, E, monkeypatch):
    """Gaussian inputs at 2 x 32 x 32 + 3 x 16 x 16: x, mean, rstd bit for bit what im2col + GEMM + LayerNorm give, or else within the fp64
    bound (which case holds is printed and logged: on the MI355X they are bit-identical at all three widths, the forward's row sums follow
    ln_fwd_kernel's order); the four gradients of both routes through functional.PatchEmbedMultiFn within the bound"""
    from esvit_amd import functional as F
    from esvit_amd import ops
    dev = torch.device("cuda")
    assert ops.act_dtype() == torch.bfloat16
    cpu = R.gaussian_inputs(R.SHAPES["route_ab"], E, seed=11 + E)
    imgs, W, bias, gamma, beta = cpu
    M = sum(R.rows_of(imgs))
    d_imgs, d_W, d_bias, d_gamma, d_beta = _dev_inputs(*cpu, dev)
    x, mean, rstd = _run_fwd(ops, (d_imgs, d_W, d_bias, d_gamma, d_beta), E, M, dev)
    cols = torch.cat([ops.patch_im2col(im.contiguous(), 4, 48) for im in d_imgs])
    y_old = ops.linear_fwd(cols, d_W.contiguous(), d_bias, out_f32=True)
    x_old, _, mean_old, rstd_old = ops.layernorm_fwd(y_old, d_gamma, d_beta, EPS, dtype=torch.float32)
    same = [torch.equal(a, b) for a, b in ((x, x_old), (mean, mean_old), (rstd, rstd_old))]
    x64, mean64, rstd64, _ = R.forward(*cpu, EPS)
    x32, mean32, rstd32, _ = R.forward(*cpu, EPS, dtype=torch.float32)
    rx = R.ratio(x, x64, R.bound(x64, x32))
    rm, rr = R.ratio(mean, mean64, R.bound(mean64, mean32)), R.ratio(rstd, rstd64, R.bound(rstd64, rstd32))
    print("bit-identical to the unfused route (x, mean, rstd):", same)
    assert all(same) or (rx <= 1 and rm <= 1 and rr <= 1), (same, rx, rm, rr)
    # gradients through the autograd node, both routes
    gx = torch.randn(M, E, generator=torch.Generator().manual_seed(5))
    ref = R.backward(imgs, W, bias, gamma, gx, mean64, rstd64)
    res = R.backward(imgs, W, bias, gamma, gx, mean32, rstd32, dtype=torch.float32)
    aW, ab = R.dya_flip_allowance(ref[4], res[4], R.cols_of(imgs))
    bounds = [R.bound(ref[0], res[0]) + aW, R.bound(ref[1], res[1]) + ab, R.bound(ref[2], res[2]), R.bound(ref[3], res[3])]
    ratios = {}
    for fused in (True, False):
        monkeypatch.setattr(F, "PATCH_FUSED", fused)
        prm = [torch.nn.Parameter(t.to(dev)) for t in (W.view(E, 3, 4, 4), bias, gamma, beta)]
        out = F.PatchEmbedMultiFn.apply(*prm, 4, *[im.contiguous() for im in d_imgs])
        assert torch.equal(out, x if fused else x_old)
        out.backward(gx.to(dev))
        torch.cuda.synchronize()
        grads = [prm[0].grad.view(E, 48), prm[1].grad, prm[2].grad, prm[3].grad]
        ratios[fused] = [R.ratio(g, r, b) for g, r, b in zip(grads, ref[:4], bounds)]
    _log("unfused_route", "route_ab", E, x=rx, mean=rm, rstd=rr, bit_identical=float(all(same)), dW=ratios[True][0], dbp=ratios[True][1],
         dgamma=ratios[True][2], dbeta=ratios[True][3], dW_unfused=ratios[False][0], dbp_unfused=ratios[False][1],
         dgamma_unfused=ratios[False][2], dbeta_unfused=ratios[False][3])
    assert all(r <= 1 for r in ratios[True]), ratios
