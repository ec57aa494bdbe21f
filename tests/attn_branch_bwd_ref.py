"""fp64 statement of the attention branch of a Swin block for ONE resolution group, differentiated by autograd:

    y = x + rowscale * ( proj( window_attention( qkv( LayerNorm(x) ) ) ) + b_proj )

LayerNorm -> zero-pad AFTER the norm -> roll -> window partition -> attention with the table's bias and the shift mask -> window
reverse -> roll back -> crop -> residual with the DropPath row factors (swin_transformer.py:283-330 with 120-152 and the mask of
249-272).  Everything is torch on the CPU in float64; nothing here imports the library."""
import torch
import torch.nn.functional as F


def relative_position_index(ws):
    """swin_transformer.py:100-109"""
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def _partition(t, ws):
    B, Hp, Wp, C = t.shape
    t = t.view(B, Hp // ws, ws, Wp // ws, ws, C)
    return t.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws * ws, C)


def _reverse(w, ws, B, Hp, Wp):
    C = w.shape[-1]
    t = w.view(B, Hp // ws, Wp // ws, ws, ws, C)
    return t.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, Hp, Wp, C)


def shift_attn_mask(Hp, Wp, ws, shift):
    """swin_transformer.py:249-272 -> [nW, N, N] of 0 / -100"""
    img = torch.zeros((1, Hp, Wp, 1), dtype=torch.float64)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    mw = _partition(img, ws).view(-1, ws * ws)
    m = mw[:, None, :] - mw[:, :, None]
    return torch.where(m != 0, torch.full_like(m, -100.0), torch.zeros_like(m))


def branch(x, gamma, beta, Wqkv, bqkv, Wproj, bproj, table, nB, H, W, ws, shift, nH, rowscale=None, eps=1e-6):
    """x [nB * H * W, C] -> y [nB * H * W, C]; all float64"""
    C = x.shape[1]
    N, hd = ws * ws, C // nH
    h = F.layer_norm(x, (C,), gamma, beta, eps).view(nB, H, W, C)
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    h = F.pad(h, (0, 0, 0, Wp - W, 0, Hp - H))
    if shift:
        h = torch.roll(h, shifts=(-shift, -shift), dims=(1, 2))
    win = _partition(h, ws)  # [nB * nW, N, C]
    B_ = win.shape[0]
    qkv = (win @ Wqkv.t() + bqkv).view(B_, N, 3, nH, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * hd ** -0.5, qkv[1], qkv[2]
    attn = q @ k.transpose(-2, -1)
    bias = table[relative_position_index(ws).view(-1)].view(N, N, nH).permute(2, 0, 1)
    attn = attn + bias[None]
    if shift:
        mask = shift_attn_mask(Hp, Wp, ws, shift)
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, nH, N, N) + mask[None, :, None]).view(B_, nH, N, N)
    attn = attn.softmax(-1)
    out = (attn @ v).transpose(1, 2).reshape(B_, N, C)
    out = out @ Wproj.t() + bproj
    t = _reverse(out, ws, nB, Hp, Wp)
    if shift:
        t = torch.roll(t, shifts=(shift, shift), dims=(1, 2))
    t = t[:, :H, :W, :].contiguous().view(nB * H * W, C)
    return x + (t if rowscale is None else t * rowscale[:, None])


NAMES = ("gx", "dgamma", "dbeta", "dWqkv", "dbqkv", "dWproj", "dbproj", "dtable")


def branch_grads(x, gin, gamma, beta, Wqkv, bqkv, Wproj, bproj, table, nB, H, W, ws, shift, nH, rowscale=None, eps=1e-6):
    """gradients of sum(y * gin) for x, gamma, beta, Wqkv, bqkv, Wproj, bproj and the table (a dict over NAMES, float64, CPU)"""
    leaves = [t.detach().double().cpu().clone().requires_grad_(True) for t in (x, gamma, beta, Wqkv, bqkv, Wproj, bproj, table)]
    rs = None if rowscale is None else rowscale.detach().double().cpu()
    y = branch(*leaves, nB, H, W, ws, shift, nH, rs, eps)
    y.backward(gin.detach().double().cpu())
    return dict(zip(NAMES, (t.grad for t in leaves)))
