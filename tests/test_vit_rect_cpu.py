"""ViT backbones on rectangular images, CPU side: the fp64 statement of the (h, w) position-grid resampling (tests/vit_rect_ref.py)
against torch's own F.interpolate and against mutants of itself, the package's separable route against the statement, and the package
model on the torch restatement of the kernels (oracle/ops_ref.py) against tests/golden/vit_rect.pt -- the REFERENCE's own
VisionTransformer on the same weights and images (tools/gen_vit_rect_golden.py).  The bound B is derived in tests/vit_rect_ref.py."""
import ctypes as C
import math
import os
from functools import partial

import numpy as np
import pytest
import torch

from tests import golden_utils as GU
from tests import vit_rect_ref as R
from tests.test_composition_cpu import cpu_ops  # noqa: F401  (fixture)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_rect.pt")
P = GU.NANO_VIT["patch"]


def nano_vit(img, dense=False, dev="cpu"):
    from esvit_amd.models import vision_transformer as V
    v = GU.NANO_VIT
    m = V.VisionTransformer(img_size=[img], patch_size=v["patch"], embed_dim=v["embed_dim"], depth=v["depth"], num_heads=v["heads"], mlp_ratio=4,
                            qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), drop_path_rate=0.0, use_dense_prediction=dense)
    GU.fill_state_dict(m.state_dict(), 0)
    if dense:
        m.head, m.head_dense = torch.nn.Identity(), torch.nn.Identity()
    return m.to(dev)


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


def package_resample(p, gh, gw):
    """functional.vit_pos_resample on the grid p [S, S, C] (a zero class-token entry in front) -> [gh, gw, C]"""
    import esvit_amd.functional as Fn
    S, _, Cc = p.shape
    pe = torch.cat((torch.zeros(1, 1, Cc, dtype=p.dtype, device=p.device), p.reshape(1, S * S, Cc)), dim=1)
    return Fn.vit_pos_resample(pe, gh, gw)[0, 1:].view(gh, gw, Cc)


# ---- the statement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%d_to_%dx%d" % c)
def test_statement_torch_and_the_package_route_agree_under_the_bound(case):
    """torch's F.interpolate with the scale-factor tuple (fp32) and the package's two fp32 matrix products, each within B of the fp64
    statement; the output extents, and the zero lines at side 61"""
    import esvit_amd.functional as Fn
    S, gh, gw = case
    p = R.grid_input(S)
    val, B = R.resample64(p, gh, gw)
    assert val.shape == (gh, gw, p.shape[2])
    raw = torch.nn.functional.interpolate(p.permute(2, 0, 1).unsqueeze(0), scale_factor=(gh / math.sqrt(S * S), gw / math.sqrt(S * S)), mode="bicubic")
    want = tuple(g - 1 if g == 61 else g for g in (gh, gw))  # floor(S * 61 / S) = 60 in doubles; every other side of the table is exact
    assert tuple(raw.shape[2:]) == want == (R.n_lines(S, S * S, gh), R.n_lines(S, S * S, gw))
    r_torch = R.worst_ratio(R.torch_interpolate(p, gh, gw), val, B)
    got = package_resample(p, gh, gw)
    r_pkg = R.worst_ratio(got, val, B)
    print("S %d -> %dx%d: torch %.3f B, package %.3f B" % (S, gh, gw, r_torch, r_pkg))
    assert r_torch <= 1.0 and r_pkg <= 1.0, (r_torch, r_pkg)
    if gh == 61:
        assert (val[60] == 0).all() and (got[60] == 0).all() and (val[59] != 0).any() and (B[60] == 0).all()
    if gw == 61:
        assert (val[:, 60] == 0).all() and (got[:, 60] == 0).all() and (val[:, 59] != 0).any()
    for g in (gh, gw):  # the package builds the same matrix as the statement, in fp64
        assert np.abs(Fn.vit_pos_axis_matrix(S, S * S, g) - R.axis(S, g)[0]).max() <= 1e-14


def test_every_mutant_of_the_statement_exceeds_the_bound():
    """A = -0.5, the align_corners mapping, the coordinate scale from the size ratio, zero taps for the border clamp, swapped axes,
    a replicated last line for the zero lines: each beyond B on at least one case.  The size ratio and the replicated line are told
    apart by the 61 cases alone (everywhere else floor(S * sf) is the side asked for)."""
    import esvit_amd.functional as Fn
    worst = {m: {} for m in R.MUTANTS}
    for S, gh, gw in R.CASES:
        p = R.grid_input(S)
        val, B = R.resample64(p, gh, gw)
        assert R.worst_ratio(package_resample(p, gh, gw), val, B) <= 1.0
        for m in R.MUTANTS:
            worst[m][(S, gh, gw)] = R.worst_ratio(R.resample64(p, gh, gw, m)[0], val, B)
    for m, per in worst.items():
        print(m, {k: "%.3g" % v for k, v in per.items()})
        assert max(per.values()) > 1.0, (m, per)
    for m in ("size_ratio", "replicate_last"):
        assert all((v > 1.0) == (61 in k[1:]) for k, v in worst[m].items()), (m, worst[m])
    assert Fn._CUBIC_A == -0.75


def test_resampling_matrices_are_cached_per_geometry():
    import esvit_amd.functional as Fn
    a = Fn.vit_pos_matrices(196, 14, 10, torch.device("cpu"))
    b = Fn.vit_pos_matrices(196, 14, 10, torch.device("cpu"))
    assert a[0] is b[0] and a[1] is b[1] and a[0].shape == (14, 14) and a[1].shape == (10, 14) and a[0].dtype == torch.float32
    assert torch.equal(a[0], torch.eye(14))  # sf = 1: every line reads its own source line


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_square_images_keep_their_token_expression_bit_for_bit(cpu_ops):  # noqa: F811
    import esvit_amd.functional as Fn
    m = nano_vit(64)
    for size in (64, 32):
        x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(size))
        with torch.no_grad():
            patches = Fn.VitPatchEmbedFn.apply(x, m.patch_embed.proj.weight, m.patch_embed.proj.bias, P)
            t = torch.cat((m.cls_token.expand(2, -1, -1), patches), dim=1)
            want = Fn.ApeAddFn.apply(t, m.interpolate_pos_encoding(t, m.pos_embed).contiguous())
            assert torch.equal(m._tokens(x), want)


@pytest.mark.parametrize("name", list(R.GOLD_CASES))
def test_package_model_matches_the_reference_on_rectangles(cpu_ops, gold, name):  # noqa: F811
    """attention maps (n = 1 and n != 1) and the final-norm tokens against the reference's VisionTransformer, at the bounds of
    test_vit_cpu.check_nano_vit_hooks; forward_features / forward_return_n_last_blocks read the same tokens"""
    g = gold[name]
    c = R.GOLD_CASES[name]
    m = nano_vit(c["img"]).eval()
    x = R.gold_images(name)
    with torch.no_grad():
        a1 = m.forward_selfattention(x)
        a2 = m.forward_selfattention(x, n=2)
        fm = m.forward_feature_maps(x)
        cls = m.forward_features(x)
        last = m.forward_return_n_last_blocks(x, n=1, return_patch_avgpool=True)
        two = m.forward_return_n_last_blocks(x, n=2)
    assert a1.shape == g["attn1"].shape and len(a2) == 2 and fm.shape == g["feats"].shape
    assert torch.allclose(a1, g["attn1"], rtol=3e-4, atol=1e-5)
    assert torch.allclose(a2[0], g["attn2_0"], rtol=3e-4, atol=1e-5) and torch.allclose(a2[1], g["attn1"], rtol=3e-4, atol=1e-5)
    assert torch.allclose(fm, g["feats"], rtol=3e-4, atol=3e-4)
    assert torch.equal(cls, fm[:, 0]) and torch.equal(last[:, :64], fm[:, 0]) and torch.allclose(last[:, 64:], fm[:, 1:].mean(1), atol=1e-6)
    assert two.shape == (c["B"], 128) and torch.equal(two[:, 64:], fm[:, 0])


def _fp64_tokens(sd, x, gh, gw):
    """a torch composition of the token path in fp64: F.unfold + the projection, the class token, the tuple F.interpolate"""
    E = sd["pos_embed"].shape[-1]
    S = int(math.sqrt(sd["pos_embed"].shape[1] - 1))
    cols = torch.nn.functional.unfold(x.double(), P, stride=P).transpose(1, 2)
    t = cols @ sd["patch_embed.proj.weight"].reshape(E, -1).t() + sd["patch_embed.proj.bias"]
    grid = sd["pos_embed"][:, 1:].reshape(1, S, S, E).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, scale_factor=(gh / math.sqrt(S * S), gw / math.sqrt(S * S)), mode="bicubic")
    assert tuple(grid.shape[2:]) == (gh, gw)
    pos = torch.cat((sd["pos_embed"][:, :1], grid.permute(0, 2, 3, 1).reshape(1, gh * gw, E)), dim=1)
    return torch.cat((sd["cls_token"].expand(x.shape[0], -1, -1), t), dim=1) + pos


def fp64_gradients(m, x, probe):
    """gradients of sum(probe * normed tokens) for every parameter, by fp64 autograd of the torch composition"""
    from oracle import esvit_oracle as O
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()}
    t = _fp64_tokens(sd, x.cpu(), x.shape[-2] // P, x.shape[-1] // P)
    for i in range(len(m.blocks)):
        t, _ = O.vit_block(sd, "blocks.%d." % i, t, GU.NANO_VIT["heads"])
    out = torch.nn.functional.layer_norm(t, (t.shape[-1],), sd["norm.weight"], sd["norm.bias"], 1e-6)
    (out * probe.double().cpu()).sum().backward()
    return out.detach(), {k: v.grad for k, v in sd.items()}


def test_gradients_reach_the_token_parameters_and_repeat_bit_for_bit(cpu_ops):  # noqa: F811
    """48 x 80: pos_embed, cls_token and patch_embed.proj.weight against fp64 autograd, under the gradient tolerance of
    test_vit_composition_matches_reference_golden (2e-3 of the norm, and of the largest entry per element); three backward passes give
    the same pos_embed.grad bits"""
    m = nano_vit(64)
    x = R.gold_images("s4_48x80")
    probe = torch.randn(2, 16, 64, generator=torch.Generator().manual_seed(8))
    _, ref = fp64_gradients(m, x, probe)
    grads = []
    for _ in range(3):
        m.zero_grad(set_to_none=True)
        (m.forward_feature_maps(x) * probe).sum().backward()
        grads.append(m.pos_embed.grad.clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    for n in ("pos_embed", "cls_token", "patch_embed.proj.weight"):
        got, want = dict(m.named_parameters())[n].grad.double(), ref[n]
        assert want.abs().max().item() > 0
        assert abs(got.norm().item() - want.norm().item()) <= 2e-3 * want.norm().item(), n
        assert (got - want).abs().max().item() <= 2e-3 * want.abs().max().item(), n


def test_crop_lists_are_grouped_by_height_and_width(cpu_ops):  # noqa: F811
    """[64^2, 48x80, 48x80, 32^2] is three runs on the ragged route and on the per-group route, each equal to the forward of its run
    alone; neighbours of equal width and different height ([48x80, 32x80]) are two runs, not one concatenation"""
    g = torch.Generator().manual_seed(12)
    crops = [torch.randn(2, 3, h, w, generator=g) for h, w in ((64, 64), (48, 80), (48, 80), (32, 32))]
    runs = [crops[0], torch.cat(crops[1:3]), crops[3]]
    m = nano_vit(64, dense=True).eval()
    with torch.no_grad():
        alone = [m.forward_feature_maps(r) for r in runs]
        for ragged in (True, False):
            m.ragged_multi_crop = ragged
            cls, _, fea, npatch = m(crops)
            assert npatch == [16, 15, 4] and cls.shape == (8, 64)
            assert torch.allclose(cls, torch.cat([a[:, 0] for a in alone]), rtol=1e-5, atol=1e-6)
            assert torch.allclose(fea, torch.cat([a[:, 1:].reshape(-1, 64) for a in alone]), rtol=1e-5, atol=1e-6)
            pair = [crops[1], torch.randn(2, 3, 32, 80, generator=torch.Generator().manual_seed(13))]
            cls2, _, _, npatch2 = m(pair)
            assert npatch2 == [15, 10]
            assert torch.allclose(cls2, torch.cat([m.forward_feature_maps(r)[:, 0] for r in pair]), rtol=1e-5, atol=1e-6)


def test_a_rectangle_is_cropped_to_whole_patches(cpu_ops):  # noqa: F811
    m = nano_vit(64).eval()
    x = torch.randn(1, 3, 55, 90, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        assert torch.equal(m.forward_feature_maps(x), m.forward_feature_maps(x[..., :48, :80]))
        assert m.forward_selfattention(x).shape == (1, 2, 16, 16)


def test_analysis_takes_rectangles_and_lists_of_shapes(cpu_ops):  # noqa: F811
    """attention_entropy / attention_rows on 48 x 80 against forward_selfattention's maps (the same probabilities by the same route on
    the CPU: 1e-6, as for squares), a mixed list in its own order, and the meter over the list"""
    from esvit_amd import analysis as A
    m = nano_vit(64).eval()
    rect, sq, tall = R.gold_images("s4_48x80"), torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(1)), R.gold_images("s4_32x96")
    with torch.no_grad():
        maps = torch.stack(m.forward_selfattention(rect, n=2)).double()
    ent = A.attention_entropy(m, rect)
    assert ent.shape == (2, 2, 2, 16) and (ent.double() - torch.special.entr(maps).sum(-1) / math.log(2.0)).abs().max().item() <= 1e-6
    rows = A.attention_rows(m, rect, [0, 15, 7], blocks=[0, 1])
    assert rows.shape == (2, 2, 2, 3, 16) and (rows.double() - maps[:, :, :, [0, 15, 7]]).abs().max().item() <= 1e-6
    batches = [sq, rect, tall]
    ents = A.attention_entropy(m, batches, queries=[0, 3])
    assert isinstance(ents, list) and [tuple(e.shape) for e in ents] == [(2, 1, 2, 2), (2, 2, 2, 2), (2, 1, 2, 2)]
    for e, b in zip(ents, batches):
        assert torch.equal(e, A.attention_entropy(m, b, queries=[0, 3]))
    rws = A.attention_rows(m, batches, [0, 3])
    assert [tuple(r.shape) for r in rws] == [(1, 1, 2, 2, 17), (1, 2, 2, 2, 16), (1, 1, 2, 2, 13)]
    assert torch.equal(rws[1], A.attention_rows(m, rect, [0, 3]))
    one = A.AttentionEntropyMeter().update(m, batches, queries=range(9)).compute()
    step = A.AttentionEntropyMeter()
    for b in batches:
        step.update(m, b, queries=range(9))
    assert one.shape == (2, 2) and torch.equal(one, step.compute()) and step.images == 4


# ---- the library's argument checks ------------------------------------------------------------------------------------------------------
def test_patch_im2col_refuses_bad_rectangles_before_any_launch(lib_built):
    """ESVIT_ERR_ARG (-1) with the sides in esvit_last_error(), the output untouched (on a host without a GPU a launch would come back
    as another error): H % P, W % P, zero sides, a negative S, P % 4, and Kpad too short or not a multiple of 8"""
    from esvit_amd import _lib, ops
    lib = _lib.lib
    img = torch.zeros(1, 3, 64, 96)
    out = torch.full((4096,), -7.25)
    keep = out.clone()

    def call(S, Pp=16, Kpad=768, dtype=ops.F32):
        rc = lib.esvit_patch_im2col(dtype, C.c_void_p(img.data_ptr()), C.c_void_p(out.data_ptr()), 1, S, Pp, Kpad, None)
        return rc, lib.esvit_last_error()

    def rect(H, W):
        return H | (W << 16)
    for got, cause in ((call(rect(40, 96)), b"H=40 W=96"), (call(rect(64, 90)), b"H=64 W=90"), (call(rect(0, 96)), b"H=0 W=96"),
                       (call(rect(64, 1) - 64), b"H=0 W=1"), (call(0), b"H=0 W=0"), (call(-16), b"P=16"), (call(rect(64, 40000)), b"P=16"),
                       (call(rect(60, 90), Pp=6, Kpad=112), b"P=6"), (call(rect(64, 96), Kpad=760), b"Kpad=760"),
                       (call(rect(64, 96), Kpad=772), b"Kpad=772"), (call(72), b"H=72 W=72")):
        assert got[0] == -1 and b"esvit_patch_im2col" in got[1] and cause in got[1], (got, cause)
    assert torch.equal(out, keep)
    assert ops.PATCH_IM2COL_RECT
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "esvit_hip.h")).read()
    assert "H = S & 0xffff" in hdr and "W = S >> 16" in hdr
