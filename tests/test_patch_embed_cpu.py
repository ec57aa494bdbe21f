"""The fused patch embedding, host side (no GPU): the fp64 statement of tests/patch_embed_ref.py agrees with F.conv2d + F.layer_norm and
their autograd gradients and catches its mutants under the bound the GPU test applies; the fused mode of esvit_patch_im2col refuses bad
arguments before any device call; the binding matches the header; functional routes by what the ops module offers."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from tests import patch_embed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5


def _case(E=96, seed=3):
    shapes = R.SHAPES["two_res_mid_tile"]
    imgs, W, bias, gamma, beta = R.gaussian_inputs(shapes, E, seed)
    M = sum(R.rows_of(imgs))
    gx = torch.randn(M, E, generator=torch.Generator().manual_seed(seed + 1))
    return imgs, W, bias, gamma, beta, gx


def _torch_reference(imgs, W, bias, gamma, beta, gx):
    """conv2d + layer_norm in fp64 on the bf16-rounded pixels, gradients by autograd (dL/dy not rounded)"""
    E = W.shape[0]
    prm = [t.double().clone().requires_grad_(True) for t in (W, bias, gamma, beta)]
    outs = []
    for im in imgs:
        y = torch.nn.functional.conv2d(R.bf16_round(im.double()), prm[0].view(E, 3, 4, 4), prm[1], stride=4)
        outs.append(torch.nn.functional.layer_norm(y.flatten(2).transpose(1, 2), (E,), prm[2], prm[3], EPS).reshape(-1, E))
    x = torch.cat(outs)
    x.backward(gx.double())
    return x.detach(), [p.grad for p in prm]


def test_statement_is_conv_plus_layernorm():
    imgs, W, bias, gamma, beta, gx = _case()
    x, mean, rstd, y = R.forward(imgs, W, bias, gamma, beta, EPS)
    xt, (dWt, dbt, dgt, dbet) = _torch_reference(imgs, W, bias, gamma, beta, gx)
    assert float((x - xt).abs().max()) < 1e-12
    dW, dbp, dg, db, _ = R.backward(imgs, W, bias, gamma, gx, mean, rstd, round_dya=False)
    for got, want in ((dW, dWt), (dbp, dbt), (dg, dgt), (db, dbet)):
        assert float((got - want).abs().max()) < 1e-10 * max(1.0, float(want.abs().max()))
    # the rounding of dya moves dW by no more than bf16's half ulp of every term
    dWr, dbpr, dgr, dbr, dya = R.backward(imgs, W, bias, gamma, gx, mean, rstd)
    assert torch.equal(dgr, dg) and torch.equal(dbr, db) and not torch.equal(dWr, dW)
    lim = 2.0 ** -8 * (dya.abs().t() @ R.cols_of(imgs).abs())  # (dya: dL/dy before the rounding)
    aW, ab = R.dya_flip_allowance(dya, dya.float(), R.cols_of(imgs))
    assert aW.shape == dW.shape and bool((aW <= 2 * lim + 1e-12).all()) and float(aW.sum()) < 0.05 * float(lim.sum())  # few roundings are in reach
    assert bool(((dWr - dW).abs() <= lim + 1e-12).all())


def test_mutants_are_caught_by_the_bound_of_the_gpu_test():
    imgs, W, bias, gamma, beta, gx = _case()
    x, mean, rstd, y = R.forward(imgs, W, bias, gamma, beta, EPS)
    x32, mean32, rstd32, _ = R.forward(imgs, W, bias, gamma, beta, EPS, dtype=torch.float32)
    bx = R.bound(x, x32)
    assert R.ratio(x32, x, bx) <= 1.0 / 3 + 1e-9  # the restatement itself sits at a third of its bound
    for kw in (dict(order="phpwc"), dict(drop_bias=True)):
        xm = R.forward(imgs, W, bias, gamma, beta, EPS, dtype=torch.float32, **kw)[0]
        assert R.ratio(xm, x, bx) > 100, kw
    m32, r32 = mean.float(), rstd.float()
    ref = R.backward(imgs, W, bias, gamma, gx, m32, r32)
    res = R.backward(imgs, W, bias, gamma, gx, m32, r32, dtype=torch.float32)
    bounds = [R.bound(a, b) for a, b in zip(ref[:4], res[:4])]
    for a, b, bd in zip(ref[:4], res[:4], bounds):
        assert R.ratio(b, a, bd) <= 1.0 / 3 + 1e-9
    unrounded = R.backward(imgs, W, bias, gamma, gx, m32, r32, dtype=torch.float32, round_dya=False)
    assert R.ratio(unrounded[0], ref[0], bounds[0]) > 10 and R.ratio(unrounded[1], ref[1], bounds[1]) > 10
    skipped = R.backward(imgs, W, bias, gamma, gx, m32, r32, dtype=torch.float32, skip_rows=(16, 32))
    for i in range(4):
        assert R.ratio(skipped[i], ref[i], bounds[i]) > 100, i


def test_exact_inputs_make_y_exact():
    for E in (96, 128, 192):
        imgs, W, bias, gamma, beta = R.exact_inputs(R.SHAPES["three_20x12"], E, paired=True)
        y64 = R.forward(imgs, W, bias, gamma, beta, EPS)[3]
        y32 = R.forward(imgs, W, bias, gamma, beta, EPS, dtype=torch.float32)[3]
        assert torch.equal(y32.double(), y64) and torch.equal(y64 * 8, (y64 * 8).round()) and torch.equal(y64[:, 0::2], y64[:, 1::2])
        assert torch.equal(R.bf16_round(W), W) and all(torch.equal(R.bf16_round(im), im) for im in imgs)


# ---- the library --------------------------------------------------------------------------------------------------------------------
def test_binding_matches_the_header(lib_built):
    from esvit_amd import _lib, ops
    raw = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "#define ESVIT_Q_PATCH_EMBED_WS %d" % ops.Q_PATCH_EMBED_WS in raw
    assert "#define ESVIT_PATCH_EMBED_MAX_CROPS %d" % _lib.PATCH_EMBED_MAX_CROPS in raw
    for name, val in (("FWD", _lib.PATCH_EMBED_FWD), ("BWD", _lib.PATCH_EMBED_BWD), ("REDUCE", _lib.PATCH_EMBED_REDUCE)):
        assert "#define ESVIT_PATCH_EMBED_%s %d" % (name, val) in raw
    for struct, cls in (("esvit_patch_crop", _lib.PatchCrop), ("esvit_patch_embed", _lib.PatchEmbed)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, raw).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.findall(r"([A-Za-z_0-9]+)\s*(?:\[[^\]]*\])?$", part.strip())[0] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], (names, [f[0] for f in cls._fields_])
    assert C.sizeof(_lib.PatchCrop) == 32 and C.sizeof(_lib.PatchEmbed) == 120 + 16 * 32


def test_query_answers_without_a_device(lib_built):
    from esvit_amd import ops
    for E in (96, 128, 192):
        rec = 4 * E * 51
        assert ops.query(ops.Q_PATCH_EMBED_WS, 1, E, 1) == rec and ops.query(ops.Q_PATCH_EMBED_WS, 1, E, 129) == 2 * rec
        big = ops.query(ops.Q_PATCH_EMBED_WS, 1, E, 1 << 30)
        assert big % rec == 0 and 0 < big // rec <= 1024
        assert ops.patch_embed_supported(torch.bfloat16, E) and not ops.patch_embed_supported(torch.float32, E)
        assert not ops.patch_embed_supported(torch.bfloat16, E, patch=8) and not ops.patch_embed_supported(torch.bfloat16, E, in_ch=1)
    for dt, E, M in ((0, 96, 64), (1, 64, 64), (1, 256, 64), (1, 96, 0), (1, 96, (1 << 30) + 1)):
        assert ops.query(ops.Q_PATCH_EMBED_WS, dt, E, M) == 0


def test_fused_mode_refuses_bad_arguments_before_any_device_call(lib_built):
    """ESVIT_ERR_ARG (-1) with the cause in esvit_last_error() (on a host without a GPU a launch would come back as another error)"""
    from esvit_amd import _lib
    lib = _lib.lib
    buf = torch.zeros(4096)
    base = buf.data_ptr() + (-buf.data_ptr()) % 16

    def desc(mode=0, E=96, crops=((1, 8, 8, 0),), **kw):
        d = _lib.PatchEmbed()
        d.mode, d.E = mode, E
        for f in ("W", "bias", "gamma", "beta", "x", "mean", "rstd", "gx", "partials", "dW", "dbp", "dgamma", "dbeta"):
            setattr(d, f, base)
        for i, (nB, H, W, r0) in enumerate(crops):
            d.crops[i].img, d.crops[i].nB, d.crops[i].H, d.crops[i].W, d.crops[i].row0 = base, nB, H, W, r0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d, n=1, dtype=1, S=0, Pp=4, Kpad=48):
        rc = lib.esvit_patch_im2col(dtype, C.cast(C.pointer(d), C.c_void_p), None, -n, S, Pp, Kpad, None)
        return rc, lib.esvit_last_error()

    two = ((1, 8, 8, 0), (1, 8, 8, 5))
    for got, cause in ((call(desc(), dtype=0), b"bf16"), (call(desc(), Pp=8), b"P=8"), (call(desc(), Kpad=64), b"Kpad=64"), (call(desc(), S=8), b"S=8"),
                       (call(desc(E=64)), b"E=64"), (call(desc(mode=7)), b"mode 7"), (call(desc(), n=17), b"not 17"),
                       (call(desc(crops=((1, 8, 10, 0),))), b"W=10"), (call(desc(crops=((0, 8, 8, 0),))), b"nB=0"),
                       (call(desc(crops=two), n=2), b"starts at row 5"), (call(desc(W=base + 2)), b"weight"), (call(desc(x=base + 4)), b"x"),
                       (call(desc(mean=None)), b"mean and rstd"), (call(desc(mode=1, gx=None)), b"null gx"),
                       (call(desc(mode=2, first_partial=0)), b"0 partial"), (call(desc(mode=2, dW=None)), b"null pointer"),
                       (call(desc(crops=(((1 << 14) + 1, 1024, 1024, 0),))), b"token rows")):
        assert got[0] == -1 and b"esvit_patch_im2col" in got[1] and cause in got[1], (got, cause)
    crop_misaligned = desc()
    crop_misaligned.crops[0].img = base + 4
    got = call(crop_misaligned)
    assert got[0] == -1 and b"misaligned image" in got[1]
    assert lib.esvit_patch_im2col(1, None, None, -1, 0, 4, 48, None) == -1
    assert not bool(buf.any())


# ---- routing ------------------------------------------------------------------------------------------------------------------------
def test_cpu_stand_in_and_the_switch_keep_the_present_route(lib_built, monkeypatch):
    from esvit_amd import functional as F
    from esvit_amd import ops
    from oracle import ops_ref
    assert F.PATCH_FUSED and not hasattr(ops_ref, "patch_embed_fwd")
    Wp = torch.zeros(96, 3, 4, 4)
    g = torch.ones(96)
    imgs = [torch.zeros(1, 3, 8, 8)]
    assert not F._patch_fused(ops_ref, Wp, g, 4, imgs)
    stub = types.SimpleNamespace(patch_embed_fwd=None, act_dtype=lambda: torch.bfloat16, patch_embed_supported=ops.patch_embed_supported)
    assert F._patch_fused(stub, Wp, g, 4, imgs)
    assert not F._patch_fused(stub, Wp, None, 4, imgs)  # PATCH_NORM off
    assert not F._patch_fused(stub, torch.zeros(64, 3, 4, 4), g, 4, imgs) and not F._patch_fused(stub, torch.zeros(96, 3, 8, 8), g, 8, imgs)
    assert not F._patch_fused(stub, Wp, g, 4, [torch.zeros(1, 3, 8, 10)]) and not F._patch_fused(stub, Wp, g, 4, [torch.zeros(1, 3, 8, 8, dtype=torch.float64)])
    stub32 = types.SimpleNamespace(patch_embed_fwd=None, act_dtype=lambda: torch.float32, patch_embed_supported=ops.patch_embed_supported)
    assert not F._patch_fused(stub32, Wp, g, 4, imgs)
    monkeypatch.setattr(F, "PATCH_FUSED", False)
    assert not F._patch_fused(stub, Wp, g, 4, imgs)  # ESVIT_PATCH_FUSED=0


def test_fused_route_hands_the_sinks_over_and_saves_no_activation(lib_built, monkeypatch):
    from esvit_amd import functional as F
    from esvit_amd import params as P
    E = 96
    seen = {}

    def patch_embed_fwd(imgs, W, bias, gamma, beta, eps, *, stats=True, out=None):
        M = sum(R.rows_of(imgs))
        seen.update(fwd=(len(imgs), tuple(W.shape), W.dtype, stats))
        return torch.full((M, E), 2.0), (torch.zeros(M) if stats else None), (torch.ones(M) if stats else None)

    def patch_embed_bwd(imgs, W, bias, gamma, gx, mean, rstd, *, partials=None):
        seen.update(bwd=(len(imgs), tuple(gx.shape)))
        return torch.zeros(3, E * 51), 3

    def patch_embed_reduce(part, nparts, E_, *, out=None):
        seen.update(red=(nparts, out))
        outs = [o if o is not None else torch.empty(s) for o, s in zip(out, ((E, 48), (E,), (E,), (E,)))]
        for i, o in enumerate(outs):
            o.fill_(float(i + 1))
        return tuple(outs)

    stub = types.SimpleNamespace(patch_embed_fwd=patch_embed_fwd, patch_embed_bwd=patch_embed_bwd, patch_embed_reduce=patch_embed_reduce,
                                 patch_embed_supported=lambda dt, E_, p, c: True, act_dtype=lambda: torch.bfloat16, PATCH_EMBED_K=48,
                                 cast_to_act=lambda t: t.bfloat16())
    monkeypatch.setattr(F, "ops", stub)
    monkeypatch.setattr(P, "ops", stub)
    prm = [torch.nn.Parameter(t) for t in (torch.randn(E, 3, 4, 4), torch.randn(E), torch.ones(E), torch.zeros(E))]
    imgs = [torch.randn(2, 3, 8, 8), torch.randn(1, 3, 4, 12)]
    sinks = {id(p): torch.zeros_like(p) for p in prm}
    P.set_grad_sink(sinks)
    try:
        x = F.PatchEmbedMultiFn.apply(*prm, 4, *imgs)
        saved = x.grad_fn.saved_tensors
        assert x.shape == (11, E) and seen["fwd"] == (2, (E, 48), torch.bfloat16, True)
        assert sorted(t.numel() for t in saved if t.dtype == torch.float32 and t.dim() == 1 and t.numel() == 11) == [11, 11]  # mean, rstd
        assert not any(t.shape == (11, E) or t.shape == (11, 48) for t in saved)  # neither y nor cols
        x.sum().backward()
    finally:
        P.set_grad_sink(None)
    assert seen["bwd"] == (2, (11, E)) and seen["red"][0] == 3
    assert seen["red"][1][0].data_ptr() == sinks[id(prm[0])].data_ptr() and all(seen["red"][1][i] is sinks[id(prm[i])] for i in (1, 2, 3))
    for i, p in enumerate(prm):
        assert p.grad.shape == p.shape and bool((p.grad == i + 1).all()) and p.grad.data_ptr() == sinks[id(p)].data_ptr()
    F.PatchEmbedMultiFn.apply(*[p.detach() for p in prm], 4, *imgs)
    assert seen["fwd"][3] is False  # a pass over frozen parameters (the EMA teacher) asks for x alone
    # the single-tensor node
    x1 = F.PatchEmbedFn.apply(imgs[0], *prm, 4)
    assert x1.shape == (2, 4, E)
    x1.sum().backward()
    assert seen["bwd"] == (1, (8, E)) and seen["red"][1] == [None] * 4
