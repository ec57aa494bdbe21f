"""Torch restatement of the qkv-tail mode of esvit_layernorm_bwd (ops.attn_tail_bwd): the tail of a Swin block's attention-branch backward
-- qkv data gradient, qkv weight / bias gradient and norm1's backward -- with the kernel's rounding points: LayerNorm(x), recomputed from
the saved statistics, and dxw = dqkv Wqkv are rounded to the activation dtype before anything reads them; every sum is fp32 (fp64 here).
`exact` is fp64 autograd of LayerNorm -> linear on the same (activation-dtype) dqkv and Wqkv, the yardstick of both routes' errors."""
import torch


def attn_tail_bwd(dqkv, x, mean, rstd, gamma, beta, Wqkv, g_in, rowscale=None, rows_per_sample=1, want_act=False, wide=torch.float32):
    """-> (gx, gx_act or None, dWqkv, dbqkv, dgamma, dbeta); wide: the dtype of the sums (float64 for a yardstick of the restatement)"""
    dt = dqkv.dtype
    M, C = x.shape
    xh = (x - mean[:, None]) * rstd[:, None]                         # fp32, as ln_bwd_kernel forms it
    xw = ((x - mean[:, None]) * rstd[:, None] * gamma + beta).to(dt)  # ln_fwd_kernel's expression, rounded as its output is
    dxw = (dqkv.to(wide) @ Wqkv.to(wide)).to(torch.float32).to(dt).float()
    gd = dxw * gamma
    s1 = gd.to(wide).sum(1, keepdim=True).to(torch.float32) / C
    s2 = (gd * xh).to(wide).sum(1, keepdim=True).to(torch.float32) / C
    gx = (gd - s1 - xh * s2) * rstd[:, None] + g_in
    gxa = None
    if want_act:
        sc = 1.0 if rowscale is None else rowscale.repeat_interleave(rows_per_sample)[:M, None]
        gxa = (gx * sc).to(dt)
    dW = (dqkv.to(wide).t() @ xw.to(wide)).to(torch.float32)
    db = dqkv.to(wide).sum(0).to(torch.float32)
    dgamma = (dxw * xh).to(wide).sum(0).to(torch.float32)
    dbeta = dxw.to(wide).sum(0).to(torch.float32)
    return gx, gxa, dW, db, dgamma, dbeta


def exact(dqkv, x, gamma, beta, Wqkv, g_in, eps, rowscale=None, rows_per_sample=1):
    """fp64 autograd -> dict of the six outputs (gx_act unrounded)"""
    M, C = x.shape
    xa = x.double().requires_grad_(True)
    g, b, W = (t.double().clone().requires_grad_(True) for t in (gamma, beta, Wqkv))
    bias = torch.zeros(3 * C, dtype=torch.float64, device=x.device, requires_grad=True)
    qkv = torch.nn.functional.layer_norm(xa, (C,), g, b, eps) @ W.t() + bias
    qkv.backward(dqkv.double())
    gx = xa.grad + g_in.double()
    sc = 1.0 if rowscale is None else rowscale.double().repeat_interleave(rows_per_sample)[:M, None]
    return dict(gx=gx, dx_act=gx * sc, dWqkv=W.grad, dbqkv=bias.grad, dgamma=g.grad, dbeta=b.grad)


def inputs(M, C, seed, device, dt=torch.bfloat16, eps=1e-6):
    """one case's operands: x with an offset and a spread of row scales, statistics as the forward saves them"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = (r(M, C) * (0.5 + torch.rand(M, 1, generator=g) * 2.0) + 0.3 * r(M, 1)).to(device)
    dqkv = (r(M, 3 * C) * 0.2).to(device).to(dt)
    g_in = (r(M, C) * 0.5).to(device)
    gamma, beta = (1.0 + 0.2 * r(C)).to(device), (0.1 * r(C)).to(device)
    Wqkv = (r(3 * C, C) * 0.08).to(device).to(dt)
    mean = x.mean(1)
    rstd = torch.rsqrt(((x - mean[:, None]) ** 2).mean(1) + eps)
    return dict(x=x, dqkv=dqkv, g_in=g_in, gamma=gamma, beta=beta, Wqkv=Wqkv, mean=mean, rstd=rstd, eps=eps)
