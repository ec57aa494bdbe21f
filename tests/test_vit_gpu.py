"""Monolithic ViT backbones on the MI355X: the layout / softmax kernels of csrc/vit_attn.hip and the batched GEMMs around them
against the torch restatement (oracle/ops_ref.py), then the whole step -- forward, DDINOLoss, every gradient -- and the evaluation
hooks against the golden produced by the REFERENCE's VisionTransformer (tests/golden/nano_vit_step.pt).
Tolerances: fp32 mode 5e-4 relative on outputs / 3e-3 on gradient norms (tf32-free fp32 MFMA, different summation order);
bf16 mode: bounds at three times the observed deltas (NANO_VIT_BF16)."""
import math
import os

import pytest
import torch

from oracle import ops_ref
from tests import golden_utils as GU
from tests.test_step_gpu import _setup, _teardown
from tests.test_vit_cpu import check_nano_vit, check_nano_vit_hooks, nano_vit_pair, run_nano_vit_step

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _close(name, got, ref, tol):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    assert math.isfinite(err), "%s: non-finite output" % name
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e (rel %.3e > tol %.1e)" % (name, err, scale, err / scale, tol)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 37, 3, 64), (3, 197, 6, 64), (3, 17, 2, 32), (1, 5, 12, 64), (2, 256, 1, 32)])
def test_heads_split_merge_and_softmax(dt, shape, lib_built):
    from esvit_amd import ops
    B, N, nH, hd = shape
    C = nH * hd
    Np = ops.vit_pad_tokens(N)
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B * N, 3 * C, generator=g).to(dt).cuda()
    y = ops.heads_split(x, B, N, nH, 3)
    want = torch.zeros(3, B, nH, Np, hd, dtype=dt, device="cuda")
    want[:, :, :, :N] = x.view(B, N, 3, nH, hd).permute(2, 0, 3, 1, 4)
    assert torch.equal(y, want)
    assert torch.equal(ops.heads_merge(y, N), x)                                       # the exact inverse on the live rows
    one = ops.heads_split(x[:, :C].contiguous(), B, N, nH, 1)
    assert torch.equal(one[0, :, :, :N], x[:, :C].reshape(B, N, nH, hd).permute(0, 2, 1, 3))
    # softmax rows, in place; pad rows / columns come out zero whatever they held
    Z, scale = B * nH, hd ** -0.5
    s = (4 * torch.randn(Z, Np, Np, generator=g)).to(dt).cuda()
    ref = torch.zeros(Z, Np, Np)
    ref[:, :N, :N] = torch.softmax(scale * s[:, :N, :N].float().cpu(), dim=-1)
    p = s.clone()
    ops.check(ops.lib.esvit_softmax_rows_fwd(ops._code(dt), ops._p(p), Z, N, Np, scale, ops._stream()), "softmax_rows_fwd")
    _close("softmax", p, ref, 1e-6 if dt == torch.float32 else 8e-3)
    assert (p[:, N:] == 0).all() and (p[:, :, N:] == 0).all()
    dp = torch.randn(Z, Np, Np, generator=g).to(dt).cuda()
    pr = p.float().cpu()
    dref = scale * pr * (dp.float().cpu() - (pr[:, :, :N] * dp.float().cpu()[:, :, :N]).sum(-1, keepdim=True))
    dref[:, N:], dref[:, :, N:] = 0, 0
    ops.check(ops.lib.esvit_softmax_rows_bwd(ops._code(dt), ops._p(p), ops._p(dp), Z, N, Np, scale, ops._stream()), "softmax_rows_bwd")
    _close("softmax backward", dp, dref, 1e-5 if dt == torch.float32 else 1.5e-2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 37, 3, 64), (4, 197, 6, 64), (3, 17, 2, 32), (2, 197, 12, 64), (1, 785, 3, 64), (2, 401, 2, 32)])
def test_vit_attention_matches_restatement(dt, shape, lib_built):
    """Attention.forward between the two projections, and its gradient: batched esvit_gemm + softmax vs oracle/ops_ref"""
    from esvit_amd import ops
    B, N, nH, hd = shape
    C = nH * hd
    g = torch.Generator().manual_seed(7 + sum(shape))
    qkv = torch.randn(B * N, 3 * C, generator=g).to(dt)
    dout = torch.randn(B * N, C, generator=g).to(dt)
    ops_ref.set_act_dtype(dt)
    try:
        o_ref, saved = ops_ref.vit_attn_fwd(qkv, B, N, nH, hd ** -0.5)
        d_ref = ops_ref.vit_attn_bwd(dout, saved, B, N, nH, hd ** -0.5)
    finally:
        ops_ref.set_act_dtype(torch.float32)
    o, att = ops.vit_attn_fwd(qkv.cuda(), B, N, nH, hd ** -0.5)
    d = ops.vit_attn_bwd(dout.cuda(), att, B, N, nH, hd ** -0.5)
    tol = 2e-5 if dt == torch.float32 else 2e-2
    _close("attention output", o, o_ref, tol)
    _close("attention probabilities", att[1].view(B, nH, att[1].shape[-2], -1)[:, :, :N, :N], saved[1], tol)
    _close("d qkv", d, d_ref, tol * 2)


NANO_VIT_BF16 = (2.3e-3, 0.026)  # (|loss - reference|, relative gradient-norm error): <= 3x the observed 7.4e-4 / 0.85 % (profiles/r03_parity_observed.jsonl)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_nano_vit_step_matches_reference_golden(prec, lib_built):
    import esvit_amd.loss as L
    g = torch.load(os.path.join(GOLD, "nano_vit_step.pt"), weights_only=False)
    dev = _setup(prec)
    try:
        student, teacher = nano_vit_pair(dev)
        s_out, t_out, loss = run_nano_vit_step(student, teacher, L, dev=dev)
        if prec == "fp32":
            check_nano_vit(g, student, s_out, t_out, loss, rt=5e-4, loss_tol=1e-4, grad_tol=3e-3)
        else:
            got = {n: p.grad for n, p in student.named_parameters() if p.grad is not None}
            GU.record_parity(test="nano_vit_step", prec="bf16", abs_err=abs(loss.item() - g["ddino_loss"]),
                             worst_grad_norm_rel=max(max(abs(got[n].norm().item() - ref) - 1e-6, 0.0) / (ref + 1e-12) for n, ref in g["grad_norms"].items()))
            assert abs(loss.item() - g["ddino_loss"]) < NANO_VIT_BF16[0], (loss.item(), g["ddino_loss"])
            assert sorted(got) == sorted(g["grad_norms"])
            for n, ref in g["grad_norms"].items():
                assert abs(got[n].norm().item() - ref) <= NANO_VIT_BF16[1] * ref + 1e-6, (n, got[n].norm().item(), ref)
    finally:
        _teardown()


def test_nano_vit_hooks_match_reference_golden(lib_built):
    g = torch.load(os.path.join(GOLD, "nano_vit_step.pt"), weights_only=False)
    dev = _setup("fp32")
    try:
        student, _ = nano_vit_pair(dev)
        check_nano_vit_hooks(g, student, dev=dev, rt=5e-4)
    finally:
        _teardown()


def test_deit_small_step_runs_through_the_trainer(lib_built):
    """deit_small at full width (197 / 37 tokens, 6 heads of 64) through EsvitTrainer: finite loss near log(K), parameters move,
    the teacher follows by EMA"""
    import esvit_amd
    from esvit_amd.engine import EsvitTrainer
    from esvit_amd.models import vision_transformer as V
    from tests import golden_utils as GU
    dev = _setup("bf16")
    try:
        torch.manual_seed(0)
        K = 4096

        def make(dp):
            m = V.deit_small(patch_size=16, drop_path_rate=dp, use_dense_prediction=True)
            m.head, m.head_dense = esvit_amd.DINOHead(384, K), esvit_amd.DINOHead(384, K)
            return m.to(dev)
        student, teacher = make(0.1), make(0.0)
        teacher.load_state_dict(student.state_dict())
        for p in teacher.parameters():
            p.requires_grad = False
        trainer = EsvitTrainer(student, teacher, esvit_amd.DDINOLoss(K, 10, 0.04, 0.04, 0, 10).to(dev), clip_grad=3.0, freeze_last_layer=1)
        crops = [c.to(dev) for c in GU.make_crops(4)]
        w0 = student.blocks[5].attn.qkv.weight.detach().clone()
        t0 = teacher.blocks[5].attn.qkv.weight.detach().clone()
        losses = [trainer.step(crops, 5e-4, 0.04, 0.99, epoch=1).item() for _ in range(3)]
        assert all(math.isfinite(v) for v in losses) and abs(losses[0] - math.log(K)) < 1.0, losses  # 0.5 * (view + region), each ~ log K
        assert (student.blocks[5].attn.qkv.weight - w0).abs().max().item() > 0
        assert (teacher.blocks[5].attn.qkv.weight - t0).abs().max().item() > 0
    finally:
        _teardown()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(6, 37, 6, 64), (5, 37, 3, 64), (4, 17, 2, 32), (3, 5, 2, 32), (2, 64, 12, 64), (3, 50, 1, 64)])
def test_small_crops_through_the_windowed_kernels(dt, shape, lib_built):
    """crops of <= 64 tokens (the 37 tokens of a 96^2 crop) run as ONE window per image through the fused kernels of window_attn.hip
    (N < ws^2, zero bias table): same result as the plain attention restatement, forward and backward"""
    import esvit_amd.functional as Fn
    from esvit_amd import ops
    B, N, nH, hd = shape
    C = nH * hd
    g = torch.Generator().manual_seed(11 + sum(shape))
    qkv = torch.randn(B * N, 3 * C, generator=g).to(dt)
    dout = torch.randn(B * N, C, generator=g).to(dt)
    bqkv = torch.zeros(3 * C)
    ops_ref.set_act_dtype(dt)
    try:
        o_ref, saved = ops_ref.vit_attn_fwd(qkv, B, N, nH, hd ** -0.5)
        d_ref = ops_ref.vit_attn_bwd(dout, saved, B, N, nH, hd ** -0.5)
    finally:
        ops_ref.set_act_dtype(torch.float32)
    o, att = Fn.vit_attention(ops, qkv.cuda(), bqkv.cuda(), B, N, nH, hd ** -0.5, True)
    assert att.route == "window" and att.lse is None            # the windowed route was taken: the 64-slot kernels keep no log-sum-exp
    d = Fn.vit_attention_bwd(ops, dout.cuda(), att, bqkv.cuda(), B, N, nH, hd ** -0.5)
    tol = 2e-5 if dt == torch.float32 else 2e-2
    _close("attention output (windowed route)", o, o_ref, tol)
    _close("d qkv (windowed route)", d, d_ref, tol * 2)
    long_seq = Fn.vit_attention(ops, torch.randn(2 * 230, 3 * C).to(dt).cuda(), bqkv.cuda(), 2, 230, nH, hd ** -0.5, True)[1]
    assert long_seq.route == "gemm"                             # 230 tokens: beyond the windowed kernels, the batched-GEMM route


@pytest.mark.parametrize("shape", [(3, 197, 6, 64), (2, 197, 3, 64), (5, 197, 12, 64), (2, 145, 2, 64), (2, 224, 1, 64), (2, 100, 4, 32), (3, 65, 6, 64)])
def test_large_crops_through_the_flash_kernels(shape, lib_built):
    """the 197 tokens of a 224^2 crop as ONE window of the 224-slot kernels of window_attn_big.hip (head_dim 64 instances, bf16, zero
    bias table over a 15 x 15 grid): same result as the plain attention restatement, forward and backward"""
    import esvit_amd.functional as Fn
    from esvit_amd import ops
    B, N, nH, hd = shape
    C = nH * hd
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(3 + sum(shape))
    qkv = torch.randn(B * N, 3 * C, generator=g).to(dt)
    dout = torch.randn(B * N, C, generator=g).to(dt)
    bqkv = torch.zeros(3 * C)
    ops_ref.set_act_dtype(dt)
    try:
        o_ref, saved = ops_ref.vit_attn_fwd(qkv, B, N, nH, hd ** -0.5)
        d_ref = ops_ref.vit_attn_bwd(dout, saved, B, N, nH, hd ** -0.5)
    finally:
        ops_ref.set_act_dtype(torch.float32)
    o, att = Fn.vit_attention(ops, qkv.cuda(), bqkv.cuda(), B, N, nH, hd ** -0.5, True)
    assert att.route == "window" and isinstance(att.lse, torch.Tensor)  # the 224-slot kernels: the windowed route WITH a log-sum-exp
    d = Fn.vit_attention_bwd(ops, dout.cuda(), att, bqkv.cuda(), B, N, nH, hd ** -0.5)
    _close("attention output (224-slot kernels)", o, o_ref, 2e-2)
    _close("d qkv (224-slot kernels)", d, d_ref, 4e-2)
    if hd == 64:  # fp32 parity mode at head_dim 64 does not fit them: the batched-GEMM route
        assert Fn.vit_attention(ops, qkv.float().cuda(), bqkv.cuda(), B, N, nH, hd ** -0.5, True)[1].route == "gemm"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_deit_small_step_matches_reference_golden(prec, lib_built):
    """deit_small at FULL width (197 / 37 tokens, both attention routes, 12 blocks), batch 2, out_dim 4096: outputs, loss, the loss
    centres, every gradient norm and a dozen sampled gradient tensors against the step of the REFERENCE's own VisionTransformer on the
    same weights and crops (tests/golden/full_vit.pt, oracle/gen_golden.py:gen_full_vit)."""
    import esvit_amd
    from esvit_amd.models import vision_transformer as V
    from tests import golden_utils as GU
    from tests.test_composition_cpu import probe_close
    g = torch.load(os.path.join(GOLD, "full_vit.pt"), map_location="cpu", weights_only=False)
    K = g["K"]
    dev = _setup(prec)
    try:
        def make(seed):
            m = V.deit_small(patch_size=16, drop_path_rate=0.0, use_dense_prediction=True)
            m.head, m.head_dense = esvit_amd.DINOHead(384, K, norm_last_layer=True), esvit_amd.DINOHead(384, K, norm_last_layer=False)
            GU.fill_state_dict(m.state_dict(), seed)
            return m
        student, teacher = make(41), make(42)
        student.head.last_layer.weight_g.data.fill_(1)
        for p in teacher.parameters():
            p.requires_grad = False
        student, teacher = student.to(dev), teacher.to(dev)
        crops = [c.to(dev) for c in GU.make_crops(2, seed=77)]
        loss_fn = esvit_amd.DDINOLoss(K, 10, 0.04, 0.07, 5, 10).to(dev)
        t_out = teacher(crops[:2])
        s_out = student(crops)
        loss = loss_fn(s_out, t_out, 2, None)
        loss.backward()
        fp = prec == "fp32"
        assert (list(s_out[3]), list(t_out[3])) == g["npatch"]
        for nm, t in (("s_cls", s_out[0]), ("s_reg", s_out[1]), ("s_fea", s_out[2]), ("t_cls", t_out[0])):
            probe_close(nm, t.float().cpu(), g[nm], rtol=5e-4 if fp else 6e-2)
        assert abs(loss.item() - g["loss"]) < (1e-4 if fp else 1e-2), (loss.item(), g["loss"])
        assert (loss_fn.center.cpu() - g["center_after"]).abs().max().item() < (1e-6 if fp else 2e-3)
        assert (loss_fn.center_grid.cpu() - g["center_grid_after"]).abs().max().item() < (1e-6 if fp else 2e-3)
        prm = dict(student.named_parameters())
        assert sorted(n for n, p in prm.items() if p.grad is not None) == sorted(g["grad_norms"])
        worst = max(abs(prm[n].grad.norm().item() - ref) / (ref + 1e-12) for n, ref in g["grad_norms"].items())
        assert worst < (5e-3 if fp else 0.2), worst
        for n, ref in g["grad_samples"].items():
            got = GU.strided(prm[n].grad.float().cpu(), 4096)
            err = (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
            assert err < (5e-3 if fp else 0.25), (n, err)
    finally:
        _teardown()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_deit_tiny_step_matches_oracle(prec, lib_built):
    """deit_tiny at full width (192 wide, 3 heads of 64, 12 blocks; 197 / 37 tokens) against the functional oracle
    (oracle/esvit_oracle.vit_multicrop, itself pinned against the reference's VisionTransformer): outputs, loss, every gradient norm.
    A case no fixture holds -- the oracle runs on the GPU box's host."""
    import esvit_amd
    from esvit_amd.models import vision_transformer as V
    from oracle import esvit_oracle as O
    from tests import golden_utils as GU
    K = 2048
    dev = _setup(prec)
    try:
        def make(seed):
            m = V.deit_tiny(patch_size=16, drop_path_rate=0.0, use_dense_prediction=True)
            m.head, m.head_dense = esvit_amd.DINOHead(192, K, norm_last_layer=True), esvit_amd.DINOHead(192, K, norm_last_layer=False)
            GU.fill_state_dict(m.state_dict(), seed)
            return m
        student, teacher = make(51), make(52)
        student.head.last_layer.weight_g.data.fill_(1)
        for p in teacher.parameters():
            p.requires_grad = False
        crops = GU.make_crops(2, seed=91)
        # oracle (CPU, fp32)
        sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in student.state_dict().items()}
        td = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
        cfg = dict(depth=12, heads=3, patch=16)
        s_ref = O.vit_multicrop(sd, crops, cfg)
        with torch.no_grad():
            t_ref = O.vit_multicrop(td, crops[:2], cfg)
        c0 = torch.zeros(1, K)
        l_ref, _, _ = O.ddino_loss(s_ref, t_ref, c0, c0, O.teacher_temp(2, 0.04, 0.07, 5, 10), 10)
        l_ref.backward()
        # HIP path
        student, teacher = student.to(dev), teacher.to(dev)
        loss_fn = esvit_amd.DDINOLoss(K, 10, 0.04, 0.07, 5, 10).to(dev)
        dcrops = [c.to(dev) for c in crops]
        t_out = teacher(dcrops[:2])
        s_out = student(dcrops)
        loss = loss_fn(s_out, t_out, 2, None)
        loss.backward()
        fp = prec == "fp32"
        assert list(s_out[3]) == list(s_ref[3])
        for nm, a, b in (("cls logits", s_out[0], s_ref[0]), ("region logits", s_out[1], s_ref[1]), ("features", s_out[2], s_ref[2])):
            _close(nm, a, b.detach(), 1e-3 if fp else 8e-2)
        assert abs(loss.item() - l_ref.item()) < (2e-4 if fp else 2e-2), (loss.item(), l_ref.item())
        worst, name = 0.0, None
        for n, p in student.named_parameters():
            if not p.requires_grad:  # norm_last_layer freezes head.last_layer.weight_g (the oracle's dict has no such notion)
                continue
            ref = sd[n].grad
            assert ref is not None and p.grad is not None, n
            rel = abs(p.grad.norm().item() - ref.norm().item()) / (ref.norm().item() + 1e-12)
            if rel > worst:
                worst, name = rel, n
        assert worst < (5e-3 if fp else 0.2), (name, worst)
    finally:
        _teardown()
