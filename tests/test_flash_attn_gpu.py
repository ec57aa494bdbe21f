"""-m gpu: the flash-attention kernels for ViT crops of any length (csrc/flash_attn.hip, the global mode of esvit_window_attn_fwd /
_bwd) against the restatement of the batched-GEMM route (oracle/ops_ref.vit_attn_fwd / _bwd) and an fp64 evaluation of the same bf16
inputs, the online softmax with the row maximum placed early and late, exactness properties (images and heads do not mix, nothing is
written past the last row, identical bits launch to launch), the memory bound that is the point of the kernels, and a small patch-8
VisionTransformer with VIT_LONG_ATTENTION = "flash" against "gemm"."""
import json
import math
import os
from functools import partial

import pytest
import torch

from tests import golden_utils as GU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "flash_attn_parity.jsonl")
BF = torch.bfloat16
BLOCK = 64  # tokens per query block and per key block of the kernels (flash_attn.hip: BLKT)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mods(lib_built):
    from esvit_amd import ops
    from oracle import ops_ref
    return ops, ops_ref


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF).to(dev)


def _rel(got, ref):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert math.isfinite(err), "non-finite output"
    return err / (ref.abs().max().item() + 1e-12)


def _attn64(qkv, dout, B, N, nH, hd, scale):
    """fp64 attention of the bf16 inputs as they are, forward and backward, in plain torch -> (out [B N, C], lse [B, nH, N], dqkv [B N, 3C])"""
    C = nH * hd
    q, k, v = qkv.double().view(B, N, 3, nH, hd).permute(2, 0, 3, 1, 4)
    s = scale * (q @ k.transpose(-2, -1))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = p @ v
    do = dout.double().view(B, N, nH, hd).permute(0, 2, 1, 3)
    dv = p.transpose(-2, -1) @ do
    dp = do @ v.transpose(-2, -1)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dq, dk = scale * (ds @ k), scale * (ds.transpose(-2, -1) @ q)
    return (o.permute(0, 2, 1, 3).reshape(B * N, C), lse,
            torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * C))


def _record(rec):
    print(json.dumps(rec))
    old = []
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            old = [json.loads(l) for l in f if l.strip()]
    old = [r for r in old if (r["test"], r["shape"]) != (rec["test"], rec["shape"])]
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "w") as f:
        for r in old + [rec]:
            f.write(json.dumps(r) + "\n")


# (B, N, nH, hd): the smallest shapes that cross each boundary of the 64-token blocking (query and key blocks are both 64)
SHAPES = [(2, 1, 2, 32),      # a single token
          (2, 17, 3, 64),     # less than one block
          (2, 64, 3, 64),     # exactly one block
          (2, 65, 3, 32),     # one token past a block
          (2, 129, 2, 64),    # one token past two blocks
          (2, 225, 3, 64),    # the first N the route will see
          (3, 257, 1, 32),    # one token past four blocks
          (2, 401, 2, 32),    # 320^2 at patch 16
          (1, 785, 3, 64)]    # the patch-8 crop


@pytest.mark.parametrize("shape", SHAPES)
def test_flash_attention_matches_restatement_and_fp64(mods, shape):
    """forward and backward vs ops_ref.vit_attn_fwd / _bwd in bf16 at the tolerances of test_large_crops_through_the_flash_kernels (out
    2e-2, dqkv 4e-2 of the reference's largest magnitude); against fp64 attention of the same bf16 inputs the error is at most three
    times that of the library's batched-GEMM route (both go to profiles/flash_attn_parity.jsonl)"""
    ops, ref = mods
    dev = _dev()
    B, N, nH, hd = shape
    C, scale = nH * hd, hd ** -0.5
    assert BLOCK == 64 and ops.global_attn_supported(BF, hd)
    qkv = _rand((B * N, 3 * C), dev, 3 + sum(shape))
    dout = _rand((B * N, C), dev, 4 + sum(shape))
    out, saved = ops.global_attn_fwd(qkv, B, N, nH, scale)
    dq = ops.global_attn_bwd(dout, saved, B, N, nH, scale)
    assert saved[2].shape == (B, nH, N) and saved[2].dtype == torch.float32
    ref.set_act_dtype(BF)
    try:
        outr, savedr = ref.vit_attn_fwd(qkv, B, N, nH, scale)
        dqr = ref.vit_attn_bwd(dout, savedr, B, N, nH, scale)
    finally:
        ref.set_act_dtype(torch.float32)
    out64, lse64, dq64 = _attn64(qkv, dout, B, N, nH, hd, scale)
    outg, savedg = ops.vit_attn_fwd(qkv, B, N, nH, scale)
    dqg = ops.vit_attn_bwd(dout, savedg, B, N, nH, scale)
    rec = dict(test="parity", shape=list(shape),
               flash_out_vs_fp64=_rel(out, out64), gemm_out_vs_fp64=_rel(outg, out64),
               flash_dqkv_vs_fp64=_rel(dq, dq64), gemm_dqkv_vs_fp64=_rel(dqg, dq64),
               flash_out_vs_restatement=_rel(out, outr), flash_dqkv_vs_restatement=_rel(dq, dqr),
               flash_lse_abs_vs_fp64=(saved[2].double() - lse64).abs().max().item())
    _record(rec)
    assert rec["flash_out_vs_restatement"] <= 2e-2, rec
    assert rec["flash_dqkv_vs_restatement"] <= 4e-2, rec
    assert rec["flash_out_vs_fp64"] <= 3 * rec["gemm_out_vs_fp64"], rec
    assert rec["flash_dqkv_vs_fp64"] <= 3 * rec["gemm_dqkv_vs_fp64"], rec


@pytest.mark.parametrize("N,hd", [(257, 64), (785, 32)])
def test_online_softmax_under_stress(mods, N, hd):
    """qkv = 4 randn (logits spread over ~ 16) and, for four queries, one key whose row is 3x the query's row, so that the row maximum
    sits in the first key block, the last full block, the tail block (one token at N = 257) and on the diagonal: the running maximum has
    to move early and late.  Against fp64 only (the restatement rounds S to bf16 and is itself off here).
      out   max |out - out64| <= 2^-7 max |v|: out is a convex combination of v rows; P is rounded to bf16 (2^-9) and so is the output
            (2^-9); four times that first-order sum
      lse   |lse - lse64| <= 1e-3 (1 + |lse64|): scores are accumulated in fp32 over hd <= 64 bf16 products
      dqkv  at most three times the batched-GEMM route's error against the same fp64"""
    ops, _ = mods
    dev = _dev()
    B, nH = 1, 2
    C, scale = nH * hd, hd ** -0.5
    nfull = N // BLOCK
    assert N % BLOCK != 0 and nfull >= 4
    qkv = _rand((B * N, 3 * C), dev, 50 + N, scale=4.0)
    pairs = [(100, 5),                              # (query, key): the maximum in the first key block
             (7, (nfull - 1) * BLOCK + 8),          # in the last full block
             (130, N - 1),                          # in the tail block
             (201, 201)]                            # on the diagonal
    assert len({k for _, k in pairs}) == 4
    for q, k in pairs:
        qkv[k, C:2 * C] = 3 * qkv[q, :C]
    dout = _rand((B * N, C), dev, 51 + N)
    out, saved = ops.global_attn_fwd(qkv, B, N, nH, scale)
    dq = ops.global_attn_bwd(dout, saved, B, N, nH, scale)
    out64, lse64, dq64 = _attn64(qkv, dout, B, N, nH, hd, scale)
    outg, savedg = ops.vit_attn_fwd(qkv, B, N, nH, scale)
    dqg = ops.vit_attn_bwd(dout, savedg, B, N, nH, scale)
    # the planted keys do hold their query's maximum
    s = scale * (qkv[:, :C].double().view(N, nH, hd).transpose(0, 1) @ qkv[:, C:2 * C].double().view(N, nH, hd).permute(1, 2, 0))
    for q, k in pairs:
        assert (s[:, q].argmax(-1) == k).all(), (q, k)
    vmax = qkv[:, 2 * C:].double().abs().max().item()
    lse = saved[2].double()
    rec = dict(test="stress", shape=[B, N, nH, hd],
               flash_out_abs_vs_fp64=(out.double() - out64).abs().max().item(), out_bound=2.0 ** -7 * vmax,
               gemm_out_abs_vs_fp64=(outg.double() - out64).abs().max().item(),
               flash_lse_rel_vs_fp64=((lse - lse64).abs() / (1 + lse64.abs())).max().item(),
               flash_dqkv_vs_fp64=_rel(dq, dq64), gemm_dqkv_vs_fp64=_rel(dqg, dq64))
    _record(rec)
    assert torch.isfinite(out.float()).all() and torch.isfinite(saved[2]).all() and torch.isfinite(dq.float()).all()
    assert rec["flash_out_abs_vs_fp64"] <= rec["out_bound"], rec
    assert rec["flash_lse_rel_vs_fp64"] <= 1e-3, rec
    assert rec["flash_dqkv_vs_fp64"] <= 3 * rec["gemm_dqkv_vs_fp64"], rec


def test_images_and_heads_do_not_mix_and_nothing_is_written_past_the_end(mods):
    ops, _ = mods
    dev = _dev()
    B, N, nH, hd = 2, 257, 3, 64
    C, scale, GUARD, CANARY = nH * hd, hd ** -0.5, 64, -7.0
    qkv = _rand((B * N, 3 * C), dev, 21)
    dout = _rand((B * N, C), dev, 22)

    def run(x):
        o = torch.full((B * N + GUARD, C), CANARY, dtype=BF, device=dev)
        d = torch.full((B * N + GUARD, 3 * C), CANARY, dtype=BF, device=dev)
        _, saved = ops.global_attn_fwd(x, B, N, nH, scale, out=o)
        ops.global_attn_bwd(dout, saved, B, N, nH, scale, dqkv=d)
        # 64 guard rows beyond B N: the canary is intact after forward and backward, and every row before them was written
        assert (o[B * N:] == CANARY).all() and (d[B * N:] == CANARY).all()
        return o[:B * N], saved[2], d[:B * N]
    o0, l0, d0 = run(qkv)
    assert torch.isfinite(o0.float()).all() and torch.isfinite(d0.float()).all()
    # another image 1: image 0's out, lse and dqkv rows keep their bits
    x1 = qkv.clone()
    x1[N:] = _rand((N, 3 * C), dev, 23)
    o1, l1, d1 = run(x1)
    assert torch.equal(o1[:N], o0[:N]) and torch.equal(l1[0], l0[0]) and torch.equal(d1[:N], d0[:N])
    assert not torch.equal(o1[N:], o0[N:])
    # other k / v columns of head 1: heads 0 and 2 keep their out columns, every row of head 1 changes
    x2 = qkv.clone()
    x2[:, C + hd:C + 2 * hd] = _rand((B * N, hd), dev, 24)
    x2[:, 2 * C + hd:2 * C + 2 * hd] = _rand((B * N, hd), dev, 25)
    o2, l2, _ = run(x2)
    assert torch.equal(o2[:, :hd], o0[:, :hd]) and torch.equal(o2[:, 2 * hd:], o0[:, 2 * hd:])
    assert torch.equal(l2[:, 0], l0[:, 0]) and torch.equal(l2[:, 2], l0[:, 2])
    assert (o2[:, hd:2 * hd] != o0[:, hd:2 * hd]).any(dim=1).all()


def test_ten_launches_give_identical_bits(mods):
    ops, _ = mods
    dev = _dev()
    B, N, nH, hd = 8, 785, 6, 64
    C, scale = nH * hd, hd ** -0.5
    qkv = _rand((B * N, 3 * C), dev, 31)
    dout = _rand((B * N, C), dev, 32)
    first = None
    for _ in range(10):
        out, saved = ops.global_attn_fwd(qkv, B, N, nH, scale)
        dq = ops.global_attn_bwd(dout, saved, B, N, nH, scale)
        if first is None:
            first = (out.clone(), saved[2].clone(), dq.clone())
            assert torch.isfinite(out.float()).all() and torch.isfinite(dq.float()).all()
        else:
            assert torch.equal(out, first[0]) and torch.equal(saved[2], first[1]) and torch.equal(dq, first[2])


def test_memory_is_linear_in_tokens(mods):
    """(1, 1601, 2, 64), 320^2 at patch 8, forward + backward: the peak above the live inputs stays below a quarter of ONE score tensor
    of the batched-GEMM route (B nH Np^2 2 B / 4 = 2.6 MB; the route needs out + dqkv + lse ~ 1.7 MB, its delta lives in the shared
    scratch; the GEMM route holds at least two score tensors of 10.4 MB), and the results agree with that route"""
    ops, _ = mods
    dev = _dev()
    B, N, nH, hd = 1, 1601, 2, 64
    C, scale = nH * hd, hd ** -0.5
    qkv = _rand((B * N, 3 * C), dev, 41)
    dout = _rand((B * N, C), dev, 42)
    _, sv = ops.global_attn_fwd(qkv[:230], 1, 230, nH, scale)  # (the shared scratch exists before the measurement)
    ops.global_attn_bwd(dout[:230], sv, 1, 230, nH, scale)
    del sv

    def peak_of(fwd, bwd):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out, saved = fwd(qkv, B, N, nH, scale)
        dq = bwd(dout, saved, B, N, nH, scale)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out, dq
    peak, out, dq = peak_of(ops.global_attn_fwd, ops.global_attn_bwd)
    peakg, outg, dqg = peak_of(ops.vit_attn_fwd, ops.vit_attn_bwd)
    Np = ops.vit_pad_tokens(N)
    one_score_tensor = B * nH * Np * Np * 2
    print(json.dumps(dict(test="memory", shape=[B, N, nH, hd], flash_peak_above_inputs_MB=peak / 1e6, gemm_peak_above_inputs_MB=peakg / 1e6,
                          one_score_tensor_MB=one_score_tensor / 1e6)))
    assert peak < one_score_tensor / 4, (peak, one_score_tensor / 4)
    assert _rel(out, outg) <= 2e-2 and _rel(dq, dqg) <= 4e-2, (_rel(out, outg), _rel(dq, dqg))


def _patch8_vit(dev, seed):
    from esvit_amd import models
    from esvit_amd.models import vision_transformer as V
    m = V.VisionTransformer(img_size=[224], patch_size=8, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                            norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), drop_path_rate=0.0, use_dense_prediction=True)
    hk = dict(hidden_dim=GU.NANO_HEAD["hidden_dim"], bottleneck_dim=GU.NANO_HEAD["bottleneck_dim"])
    m.head = models.DINOHead(128, GU.NANO_HEAD["out_dim"], norm_last_layer=True, **hk)
    m.head_dense = models.DINOHead(128, GU.NANO_HEAD["out_dim"], norm_last_layer=False, **hk)
    GU.fill_state_dict(m.state_dict(), seed)
    return m.to(dev)


def test_patch8_vit_routes_agree(lib_built, monkeypatch):
    """VisionTransformer(patch 8, 128 wide, 2 heads of 64, 2 blocks) + DINOHeads + DDINOLoss on 2 x 224^2 + 2 x 96^2 crops (785 and 145
    tokens), one forward + backward per route from the same weights, on the ragged and on the per-group schedule: under "flash" the
    785-token group goes through ops.global_attn_fwd and the 145-token group does not; loss and every gradient norm agree with the
    "gemm" route within NANO_VIT_BF16, the project's bound for a bf16 ViT step against its reference"""
    import esvit_amd.functional as Fn
    import esvit_amd.loss as L
    from esvit_amd import ops
    from tests.test_step_gpu import _setup, _teardown
    from tests.test_vit_gpu import NANO_VIT_BF16
    dev = _setup("bf16")
    seen = []
    f0 = ops.global_attn_fwd
    monkeypatch.setattr(ops, "global_attn_fwd", lambda qkv, B, N, *a, **k: (seen.append(N), f0(qkv, B, N, *a, **k))[1])
    res = {}
    try:
        crops = [c.to(dev) for c in GU.make_crops(2, n_local=2, seed=5)]
        assert [tuple(c.shape) for c in crops] == [(2, 3, 224, 224)] * 2 + [(2, 3, 96, 96)] * 2
        for ragged in (True, False):
            for route in ("flash", "gemm"):
                monkeypatch.setattr(Fn, "VIT_LONG_ATTENTION", route)
                del seen[:]
                student, teacher = _patch8_vit(dev, 0), _patch8_vit(dev, 7)
                student.head.last_layer.weight_g.data.fill_(1)
                for p in teacher.parameters():
                    p.requires_grad = False
                student.ragged_multi_crop = teacher.ragged_multi_crop = ragged
                loss_fn = L.DDINOLoss(GU.NANO_HEAD["out_dim"], 4, 0.04, 0.07, 5, 10).to(dev)
                t_out = teacher(crops[:2])
                s_out = student(crops)
                assert sorted(set(s_out[3])) == [144, 784], s_out[3]
                loss = loss_fn(s_out, t_out, 2, None)
                loss.backward()
                res[ragged, route] = (loss.item(), {n: p.grad.norm().item() for n, p in student.named_parameters() if p.grad is not None})
                if route == "flash":  # teacher and student, two blocks each, the 785-token group only
                    assert seen and set(seen) == {785} and len(seen) == 4, (ragged, seen)
                else:
                    assert not seen, (ragged, seen)
                if ragged and route == "flash":
                    student.eval()
                    with torch.no_grad():
                        att = student.forward_selfattention(crops[0])  # (needs the probabilities: the batched-GEMM route)
                    assert att.shape == (2, 2, 785, 785)
                    assert (att.float().sum(-1) - 1).abs().max().item() < 2e-2 and (att >= 0).all()
    finally:
        _teardown()
    for ragged in (True, False):
        (lf, gf), (lg, gg) = res[ragged, "flash"], res[ragged, "gemm"]
        worst = max(abs(gf[n] - gg[n]) / (gg[n] + 1e-12) for n in gg)
        print(json.dumps(dict(test="patch8_vit", ragged=ragged, loss_flash=lf, loss_gemm=lg, worst_grad_norm_rel=worst)))
        assert math.isfinite(lf) and abs(lf - lg) < NANO_VIT_BF16[0], (ragged, lf, lg)
        assert sorted(gf) == sorted(gg)
        for n, r in gg.items():
            assert abs(gf[n] - r) <= NANO_VIT_BF16[1] * r + 1e-6, (ragged, n, gf[n], r)
