"""-m gpu: ViT backbones on rectangular images on the MI355X.  esvit_patch_im2col's rectangular form against F.unfold (a pure copy: bit
for bit), the (h, w) position-grid resampling against its fp64 statement under the bound B of tests/vit_rect_ref.py, the nano models
against the REFERENCE's VisionTransformer (tests/golden/vit_rect.pt), the attention routes at deit_tiny's width against the same
module on the CPU restatement of the kernels (oracle/ops_ref.py), one training step on a mixed crop list, and the analysis entry
points.  No bound here is new: each is the one the named square-crop test applies on the same route (a rectangle adds no arithmetic to
those kernels).  The largest observed fraction of every bound goes to profiles/vit_rect_parity_observed.jsonl; above 1 fails."""
import json
import math
import os
from functools import partial

import pytest
import torch

from oracle import ops_ref
from tests import attn_stats_ref as AR
from tests import golden_utils as GU
from tests import vit_rect_ref as R
from tests.test_step_gpu import _setup, _teardown
from tests.test_vit_cpu import nano_vit_pair
from tests.test_vit_gpu import NANO_VIT_BF16
from tests.test_vit_rect_cpu import nano_vit, package_resample

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vit_rect.pt")
OBSERVED = os.path.join(ROOT, "profiles", "vit_rect_parity_observed.jsonl")


def _record(test, case, **ratios):
    """one line per (test, case): the observed fraction of each bound; rewritten in place on a later run"""
    rec = dict(test=test, case=case, **{k: float("%.4g" % v) for k, v in ratios.items()})
    print(json.dumps(rec))
    old = []
    if os.path.exists(OBSERVED):
        with open(OBSERVED) as f:
            old = [json.loads(ln) for ln in f if ln.strip()]
    old = [r for r in old if (r["test"], r["case"]) != (test, case)]
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "w") as f:
            for r in old + [rec]:
                f.write(json.dumps(r) + "\n")
    except OSError:
        pass
    for k, v in ratios.items():
        assert v <= 1.0, (test, case, k, v)


def _allclose_ratio(got, ref, rtol, atol):
    """the largest |got - ref| / (atol + rtol |ref|): torch.allclose holds exactly when this is <= 1"""
    got, ref = got.float().cpu().double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    r = ((got - ref).abs() / (atol + rtol * ref.abs())).max().item()
    assert math.isfinite(r)
    return r


def _scale_ratio(got, ref, tol):
    """test_vit_gpu._close as a fraction: max |got - ref| / (tol max |ref|)"""
    got, ref = got.float().cpu().double(), ref.float().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    r = (got - ref).abs().max().item() / (tol * (ref.abs().max().item() + 1e-12))
    assert math.isfinite(r)
    return r


class _cpu_restatement:
    """inside: esvit_amd runs on oracle/ops_ref in fp32 (what the cpu_ops fixture of the CPU tests does)"""

    def __enter__(self):
        import esvit_amd.functional as Fn
        import esvit_amd.loss as L
        import esvit_amd.params as P
        self.mods = (Fn, L, P)
        self.saved = [m.ops for m in self.mods]
        for m in self.mods:
            m.ops = ops_ref
        ops_ref.set_act_dtype(torch.float32)
        P.clear()
        Fn._GEOM.clear()

    def __exit__(self, *exc):
        Fn, _, P = self.mods
        for m, o in zip(self.mods, self.saved):
            m.ops = o
        P.clear()
        Fn._GEOM.clear()


# ---- esvit_patch_im2col ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("geo", [(2, 32, 80, 16), (2, 24, 40, 8)], ids=lambda g: "%dx%dx%d_p%d" % g)
def test_patch_im2col_of_a_rectangle_equals_unfold(lib_built, geo, dt):
    """fp32: the bits of F.unfold; bf16: torch's round-to-nearest-even of them; zero tail columns up to Kpad; a NaN moat around the
    output intact; a square image in the rectangular encoding of S gives the bits of the plain call"""
    from esvit_amd import ops
    nB, H, W, Pp = geo
    K = 3 * Pp * Pp
    Kpad = K + 8
    rows = nB * (H // Pp) * (W // Pp)
    img = torch.randn(nB, 3, H, W, generator=torch.Generator().manual_seed(H + W)).cuda()
    want = torch.nn.functional.unfold(img, Pp, stride=Pp).transpose(1, 2).reshape(rows, K)
    guard = 4
    buf = torch.full((rows + 2 * guard, Kpad), float("nan"), dtype=dt, device="cuda")
    got = ops.patch_im2col(img, Pp, Kpad, dtype=dt, out=buf[guard:guard + rows])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf[guard].data_ptr()
    assert torch.equal(got[:, :K], want.to(dt)) and (got[:, K:] == 0).all()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + rows:]).all()
    assert torch.equal(ops.patch_im2col(img, Pp, K, dtype=dt), want.to(dt))
    sq = torch.randn(nB, 3, H, H, generator=torch.Generator().manual_seed(H)).cuda()
    plain = ops.patch_im2col(sq, Pp, Kpad, dtype=dt)
    packed = torch.full_like(plain, float("nan"))
    ops.check(ops.lib.esvit_patch_im2col(ops._code(dt), ops._p(sq), ops._p(packed), nB, H | (H << 16), Pp, Kpad, ops._stream()), "patch_im2col")
    assert torch.equal(packed, plain)
    assert torch.equal(plain[:, :K], torch.nn.functional.unfold(sq, Pp, stride=Pp).transpose(1, 2).reshape(-1, K).to(dt))


# ---- the position grid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%d_to_%dx%d" % c)
def test_resampling_on_the_device_matches_the_statement(lib_built, case):
    """forward under B, the gradient of the grid under Bg (tests/vit_rect_ref.py), and the same gradient bits on three passes"""
    S, gh, gw = case
    p = R.grid_input(S)
    val, B = R.resample64(p, gh, gw)
    g = torch.randn(gh, gw, p.shape[2], generator=torch.Generator().manual_seed(S + gh + gw))
    gval, Bg = R.resample_bwd64(g, S, gh, gw)
    grads = []
    for _ in range(3):
        pd = p.cuda().requires_grad_(True)
        out = package_resample(pd, gh, gw)
        out.backward(g.cuda())
        grads.append(pd.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    _record("resample", "%d_to_%dx%d" % case, forward=R.worst_ratio(out.detach().cpu(), val, B), backward=R.worst_ratio(grads[0].cpu(), gval, Bg))


# ---- the nano models against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(R.GOLD_CASES))
def test_nano_vit_on_rectangles_matches_the_reference(lib_built, name, prec):
    """attention maps and final-norm tokens against tests/golden/vit_rect.pt: the fp32 parity mode at test_vit_gpu's rt = 5e-4 (the
    form of check_nano_vit_hooks), bf16 at the 6e-2 of the largest reference entry that file grants a bf16 ViT's outputs"""
    g = torch.load(GOLD, weights_only=False)[name]
    c = R.GOLD_CASES[name]
    dev = _setup(prec)
    try:
        m = nano_vit(c["img"], dev=dev).eval()
        x = R.gold_images(name).to(dev)
        with torch.no_grad():
            a1 = m.forward_selfattention(x)
            a2 = m.forward_selfattention(x, n=2)
            fm = m.forward_feature_maps(x)
        assert len(a2) == 2
        if prec == "fp32":
            rt = 5e-4
            _record("nano_golden_fp32", name, attn1=_allclose_ratio(a1, g["attn1"], rt, 1e-5), attn2_0=_allclose_ratio(a2[0], g["attn2_0"], rt, 1e-5),
                    attn2_1=_allclose_ratio(a2[1], g["attn1"], rt, 1e-5), feats=_allclose_ratio(fm, g["feats"], rt, rt))
        else:
            _record("nano_golden_bf16", name, attn1=_scale_ratio(a1, g["attn1"], 6e-2), attn2_0=_scale_ratio(a2[0], g["attn2_0"], 6e-2),
                    attn2_1=_scale_ratio(a2[1], g["attn1"], 6e-2), feats=_scale_ratio(fm, g["feats"], 6e-2))
    finally:
        _teardown()


# ---- the attention routes at deit_tiny's width ---------------------------------------------------------------------------------------------
def _tiny_width_vit(dev="cpu"):
    from esvit_amd.models import vision_transformer as V
    m = V.VisionTransformer(img_size=[224], patch_size=16, embed_dim=192, depth=2, num_heads=3, mlp_ratio=4, qkv_bias=True,
                            norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), drop_path_rate=0.0)
    GU.fill_state_dict(m.state_dict(), 3)
    return m.to(dev).eval()


@pytest.mark.parametrize("geo", [(224, 160, 141, None), (256, 352, 353, "gemm"), (256, 352, 353, "flash")], ids=["141_one_window", "353_gemm", "353_flash"])
def test_attention_routes_take_rectangles(lib_built, monkeypatch, geo):
    """192 wide, 3 heads of 64, 2 blocks, B = 2, bf16.  224 x 160: 141 tokens through the 224-slot one-window kernels; 256 x 352: 353
    tokens through the batched-GEMM and through the flash route.  Final-norm tokens against the same module on the CPU restatement in
    fp32, at the 6e-2 of the largest reference entry test_vit_gpu grants the outputs of a full-width bf16 ViT, the attention maps of
    forward_selfattention included; their row sums within 2e-2 of 1 (test_patch8_vit_routes_agree)"""
    import esvit_amd.functional as Fn
    from esvit_amd import ops
    H, W, N, route = geo
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    with _cpu_restatement(), torch.no_grad():
        ref = _tiny_width_vit()
        fm_ref, att_ref = ref.forward_feature_maps(x), ref.forward_selfattention(x)
    assert fm_ref.shape == (2, N, 192) and att_ref.shape == (2, 3, N, N)
    dev = _setup("bf16")
    try:
        seen = []
        f0 = ops.global_attn_fwd
        monkeypatch.setattr(ops, "global_attn_fwd", lambda qkv, B, n, *a, **k: (seen.append(n), f0(qkv, B, n, *a, **k))[1])
        if route is not None:
            monkeypatch.setattr(Fn, "VIT_LONG_ATTENTION", route)
        m = _tiny_width_vit(dev)
        with torch.no_grad():
            fm = m.forward_feature_maps(x.to(dev))
            assert seen == ([N, N] if route == "flash" else []), seen  # one call per block on the flash route, none on the others
            att = m.forward_selfattention(x.to(dev))
        assert Fn._vit_fused_route(N, 64, torch.bfloat16) == (route is None)
        assert (att >= 0).all()
        _record("attention_routes", "%dx%d_%s" % (H, W, route or "one_window"), feats=_scale_ratio(fm, fm_ref, 6e-2), attn=_scale_ratio(att, att_ref, 6e-2),
                attn_row_sum=(att.float().sum(-1) - 1).abs().max().item() / 2e-2)
    finally:
        _teardown()


# ---- a training step on a mixed crop list -----------------------------------------------------------------------------------------------------
def _mixed_step(student, teacher, loss_mod, crops, dev):
    loss_fn = loss_mod.DDINOLoss(GU.NANO_HEAD["out_dim"], 5, 0.04, 0.07, 5, 10).to(dev)
    t_out = teacher(crops[:2])
    s_out = student(crops)
    loss = loss_fn(s_out, t_out, 2, None)
    student.zero_grad(set_to_none=True)
    loss.backward()
    return s_out, loss.item(), {n: p.grad.detach().clone() for n, p in student.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_training_step_on_squares_and_rectangles(lib_built, prec):
    """the nano student / teacher + DINOHeads + DDINOLoss on [64^2, 64^2, 48x80 x 3] (ragged route): loss and every gradient norm against
    the same step on the CPU restatement, at the nano ViT step's bounds (fp32: loss 1e-4, norms 3e-3, features 5e-4 of the largest
    entry; bf16: NANO_VIT_BF16); gradients reach pos_embed, cls_token and patch_embed.proj; three steps give the same pos_embed.grad bits"""
    import esvit_amd.loss as L
    g = torch.Generator().manual_seed(31)
    crops = [torch.randn(2, 3, h, w, generator=g) for h, w in ((64, 64), (64, 64), (48, 80), (48, 80), (48, 80))]
    with _cpu_restatement():
        student, teacher = nano_vit_pair()
        s_ref, l_ref, g_ref = _mixed_step(student, teacher, L, crops, "cpu")
    assert list(s_ref[3]) == [16, 15] and all(g_ref[n].abs().max().item() > 0 for n in ("pos_embed", "cls_token", "patch_embed.proj.weight"))
    dev = _setup(prec)
    try:
        student, teacher = nano_vit_pair(dev)
        dcrops = [c.to(dev) for c in crops]
        steps = [_mixed_step(student, teacher, L, dcrops, dev) for _ in range(3)]
        s_out, loss, grads = steps[0]
        assert list(s_out[3]) == [16, 15] and sorted(grads) == sorted(g_ref)
        assert torch.equal(steps[1][2]["pos_embed"], grads["pos_embed"]) and torch.equal(steps[2][2]["pos_embed"], grads["pos_embed"])
        fp = prec == "fp32"
        loss_tol, grad_tol = (1e-4, 3e-3) if fp else NANO_VIT_BF16
        worst = max((abs(grads[n].norm().item() - r.norm().item()) - (0.0 if fp else 1e-6)) / (grad_tol * r.norm().item() + 1e-12) for n, r in g_ref.items())
        _record("mixed_step_" + prec, "64x64x2_48x80x3", loss=abs(loss - l_ref) / loss_tol, grad_norms=max(worst, 0.0),
                feats=_scale_ratio(s_out[2], s_ref[2].detach(), 5e-4 if fp else 6e-2))
    finally:
        _teardown()


# ---- analysis ------------------------------------------------------------------------------------------------------------------------------
def test_analysis_on_a_rectangle_matches_fp64(lib_built):
    """a 2-block patch-8 ViT of deit_tiny's width in bf16 on 48 x 80 (61 tokens), as test_vit_analysis_matches_fp64_and_the_attention_maps
    does for squares: attention_entropy / attention_rows against the fp64 statement on the same blocks' qkv (the bounds of
    tests/test_attn_stats_gpu.py) and against forward_selfattention(n=2)'s maps (that test's bound for the two routes); a mixed list
    gives the same tensors in its order"""
    import esvit_amd
    import esvit_amd.functional as Fn
    from esvit_amd import analysis as A
    from tests.test_attn_stats_gpu import ULP1, _fractions, _queries, _vit
    dev = torch.device("cuda:0")
    esvit_amd.set_precision("bf16")
    try:
        m = _vit(dev, 192, 3, 8, 64)
        nH, hd, N = 3, 64, 61
        x = torch.randn(2, 3, 48, 80, generator=torch.Generator().manual_seed(48)).to(dev)
        sq = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(64)).to(dev)
        queries = _queries(N)
        ent = A.attention_entropy(m, x, unit="nats")
        rows = A.attention_rows(m, x, queries, blocks=[0, 1])
        assert ent.shape == (2, 2, nH, N) and rows.shape == (2, 2, nH, len(queries), N)
        both = A.attention_entropy(m, [sq, x], unit="nats")
        assert both[0].shape == (2, 1, nH, 65) and torch.equal(both[1], ent)
        assert torch.equal(A.attention_rows(m, [x, sq], [0, 60], blocks=[0, 1])[0], A.attention_rows(m, x, [0, 60], blocks=[0, 1]))
        with torch.no_grad(), Fn._long_attention("flash"):
            maps = m.forward_selfattention(x, n=2)
            t = m._tokens(x)
            o = Fn.ops_module()
            for i, blk in enumerate(m.blocks):
                g1, b1, Wqkv, bqkv = blk._params()[:4]
                qkv = o.linear_fwd(o.layernorm_fwd(t.contiguous().view(2 * N, 192), g1, b1, Fn.LN_EPS)[0], Fn._weight(Wqkv), bqkv)
                ent64, rows64, lse64 = AR.stats64(qkv, 2, N, nH, hd, hd ** -0.5, queries)
                frac = _fractions(ent[i], rows[i], lse64, ent64, rows64, lse64, N, queries)
                smax = AR.scores64(qkv, 2, N, nH, hd, hd ** -0.5).abs().max(-1).values
                delta, dg = 1e-3 * (1 + lse64.abs()), 2.0 ** -9 * smax
                p = maps[i].double()
                ent_tol = 2 * (delta + dg) * max(1.0, math.log(N)) + 2.0 ** -9 * (math.log(N) + 1)
                dq, dgq = delta[:, :, queries].unsqueeze(-1), dg[:, :, queries].unsqueeze(-1)
                row_tol = (2 * dq + torch.expm1(2 * dgq) + 2.0 ** -9) * rows64 + ULP1
                _record("analysis_48x80", "block%d" % i, entropy=frac["entropy"], rows=frac["rows"], row_sum=frac["row_sum"],
                        maps_entropy=((ent[i].double() - torch.special.entr(p).sum(-1)).abs() / ent_tol).max().item(),
                        maps_rows=((rows[i].double() - p[:, :, queries]).abs() / row_tol).max().item())
                t = blk(t)
    finally:
        esvit_amd.set_precision("fp32")
