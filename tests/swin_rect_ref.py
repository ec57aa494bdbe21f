"""The fp64 statement of a Swin backbone on an explicit H x W token grid (models/swin_transformer.py of the reference, with the grid
handed down instead of recovered as int(sqrt(L))), which tests/test_swin_rect_cpu.py and tests/test_swin_rect_gpu.py hold the model
and the pad mode of the PatchMerging kernels against.

It is written the way the reference formulates the block: tensors are viewed as [B, H, W, C], padded with F.pad, rolled with
torch.roll, cut into windows with view / permute, and the region mask comes from labelled slices -- no index tables, so that it shares
nothing with the win2tok maps of the kernels or with the closed-form maps of oracle/esvit_oracle.py.  Everything runs in the dtype of
the state dict it is given (the tests pass fp64); gradients come from torch's autograd.

  block(sd, pre, x, H, W, heads, ws, shift)   LayerNorm -> zero-pad bottom / right to multiples of the window -> roll by -shift ->
                                              windows -> attention (+ relative-position bias, -100 region mask) -> reverse -> roll
                                              back -> crop -> residual -> LayerNorm -> MLP -> residual
  merge(sd, pre, x, H, W)                     zero row / column appended when H / W is odd -> four strided slices concatenated ->
                                              LayerNorm(4C) -> reduction
  features(sd, img, cfg)                      patch embedding (strided convolution: remainder rows / columns are lost), the stages, the
                                              final norm -> cls, region tokens, the attention maps and the grid of every stage

MUTANTS are wrong variants of the statement; each names the property it breaks, and `catches(mut, gh, gw, cfg)` says which image grids
must tell it from the statement (the tests assert both that those do and that every rectangular case catches at least one).
"""
import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-6
PATCH = 4

NANO2_96 = dict(embed_dim=96, depths=(2, 2), heads=(3, 6), window=7, img=224)  # fused attention-branch / MLP widths: C = 96, 192

MUTANTS = {
    "pad_before_norm": "the block zero-pads BEFORE its first LayerNorm: pad tokens become beta instead of 0",
    "swap_hw": "the block reads the token rows as a W x H grid",
    "merge_drops_odd_line": "PatchMerging drops the odd last row / column instead of padding it",
    "merge_pad_outside_stats": "the zeros of the pad quadrants are left out of the LayerNorm(4C) statistics",
    "shift_one_axis": "the cyclic shift is applied to the rows only",
}


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
def windows_of(x, ws):
    """[B, Hp, Wp, C] -> [B * nW, ws * ws, C], windows row-major"""
    B, Hp, Wp, C = x.shape
    x = x.view(B, Hp // ws, ws, Wp // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def grid_of(w, ws, Hp, Wp):
    """inverse of windows_of"""
    C = w.shape[-1]
    B = w.shape[0] // ((Hp // ws) * (Wp // ws))
    x = w.view(B, Hp // ws, Wp // ws, ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)


def region_mask(Hp, Wp, ws, shift, dtype):
    """0 / -100 [nW, N, N]: tokens of the rolled, padded grid attend only within their region of the un-rolled picture"""
    label = torch.zeros(1, Hp, Wp, 1, dtype=dtype)
    n = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            label[:, hs, wsl, :] = n
            n += 1
    lw = windows_of(label, ws).squeeze(-1)          # [nW, N]
    diff = lw[:, None, :] - lw[:, :, None]
    return torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff))


def relative_bias(table, ws, heads):
    """[heads, N, N] from the (2 ws - 1)^2 table"""
    c = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)  # [2, N]
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (ws - 1)
    idx = rel[..., 0] * (2 * ws - 1) + rel[..., 1]
    return table[idx.reshape(-1)].view(ws * ws, ws * ws, heads).permute(2, 0, 1)


def layer_norm(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, LN_EPS)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def block(sd, pre, x, H, W, heads, ws, shift, mut=None, maps=None):
    """x [B, H * W, C] -> the same shape; maps (a list) receives the softmax tensor [B * nW, heads, N, N]"""
    B, L, C = x.shape
    assert L == H * W
    if mut == "swap_hw":
        H, W = W, H
    pad_b, pad_r = (ws - H % ws) % ws, (ws - W % ws) % ws
    if mut == "pad_before_norm":
        h = F.pad(x.view(B, H, W, C), (0, 0, 0, pad_r, 0, pad_b))
        h = layer_norm(h, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"])
    else:
        h = layer_norm(x, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"]).view(B, H, W, C)
        h = F.pad(h, (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = H + pad_b, W + pad_r
    if shift > 0:
        h = torch.roll(h, shifts=(-shift,), dims=(1,)) if mut == "shift_one_axis" else torch.roll(h, shifts=(-shift, -shift), dims=(1, 2))
    w = windows_of(h, ws)
    N, hd = ws * ws, C // heads
    qkv = F.linear(w, sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]).view(-1, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * hd ** -0.5, qkv[1], qkv[2]
    att = q @ k.transpose(-2, -1) + relative_bias(sd[pre + "attn.relative_position_bias_table"], ws, heads).unsqueeze(0)
    if shift > 0:
        m = region_mask(Hp, Wp, ws, shift, att.dtype)
        att = (att.view(B, m.shape[0], heads, N, N) + m[None, :, None]).view(-1, heads, N, N)
    att = att.softmax(-1)
    if maps is not None:
        maps.append(att)
    o = (att @ v).transpose(1, 2).reshape(-1, N, C)
    o = F.linear(o, sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"])
    o = grid_of(o, ws, Hp, Wp)
    if shift > 0:
        o = torch.roll(o, shifts=(shift,), dims=(1,)) if mut == "shift_one_axis" else torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    x = x + o[:, :H, :W, :].reshape(B, L, C)
    h2 = layer_norm(x, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"])
    return x + F.linear(gelu(F.linear(h2, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])), sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"])


def merge_rows(x, H, W, mut=None):
    """[B, H * W, C] -> ([B, Ho * Wo, 4C] before the norm, live [Ho * Wo, 4C] bool or None, Ho, Wo)"""
    B, L, C = x.shape
    g = x.view(B, H, W, C)
    live = None
    if mut == "merge_drops_odd_line":
        g = g[:, :H - H % 2, :W - W % 2]
    elif H % 2 or W % 2:
        g = F.pad(g, (0, 0, 0, W % 2, 0, H % 2))
        live = F.pad(torch.ones(1, H, W, 1, dtype=torch.bool), (0, 0, 0, W % 2, 0, H % 2))
    Ho, Wo = g.shape[1] // 2, g.shape[2] // 2

    def cat4(t):
        return torch.cat([t[:, 0::2, 0::2], t[:, 1::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 1::2]], -1)
    rows = cat4(g).reshape(B, Ho * Wo, 4 * C)
    if live is not None:
        live = cat4(live.expand(1, -1, -1, C)).reshape(Ho * Wo, 4 * C)
    return rows, live, Ho, Wo


def merge_norm(rows, live, w, b, mut=None):
    if mut == "merge_pad_outside_stats" and live is not None:
        m = live.to(rows.dtype)
        n = m.sum(-1, keepdim=True)
        mu = (rows * m).sum(-1, keepdim=True) / n
        var = (((rows - mu) * m) ** 2).sum(-1, keepdim=True) / n
        return (rows - mu) * torch.rsqrt(var + LN_EPS) * w + b
    return layer_norm(rows, w, b)


def merge(sd, pre, x, H, W, mut=None):
    """-> ([B, Ho * Wo, 2C], Ho, Wo)"""
    rows, live, Ho, Wo = merge_rows(x, H, W, mut)
    return F.linear(merge_norm(rows, live, sd[pre + "norm.weight"], sd[pre + "norm.bias"], mut), sd[pre + "reduction.weight"]), Ho, Wo


def slots_to_grid(values, H, W, ws, shift):
    """a per-slot tensor of one block [B * nW, heads, ws * ws] back on its H x W grid, by the statement's own reverse / roll back /
    crop -> [B, heads, H, W]"""
    Hp, Wp = H + (ws - H % ws) % ws, W + (ws - W % ws) % ws
    g = grid_of(values.permute(0, 2, 1).contiguous(), ws, Hp, Wp)
    if shift > 0:
        g = torch.roll(g, shifts=(shift, shift), dims=(1, 2))
    return g[:, :H, :W, :].permute(0, 3, 1, 2)


def block_geometry(cfg, gh, gw):
    """(H, W, window, shift) of every block for an image whose patch grid is gh x gw"""
    out, h, w = [], gh, gw
    for depth, (ws, can_shift) in zip(cfg["depths"], stage_windows(cfg)):
        out += [(h, w, ws, cfg["window"] // 2 if (d % 2 and can_shift) else 0) for d in range(depth)]
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def stage_windows(cfg):
    """(window, can shift) per stage: fixed at construction from cfg["img"], whatever image arrives later"""
    out = []
    for s in range(len(cfg["depths"])):
        res = cfg.get("img", 224) // PATCH // 2 ** s
        out.append((res, False) if res <= cfg["window"] else (cfg["window"], True))
    return out


def features(sd, img, cfg, mut=None):
    """img [B, 3, Hi, Wi] -> (cls [B, Cf], region [B, T, Cf], attention maps per block, [(h, w) per stage])"""
    x = F.conv2d(img, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=PATCH)
    B, C, H, W = x.shape
    x = layer_norm(x.flatten(2).transpose(1, 2), sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"])
    maps, grids = [], []
    for s, (depth, (ws, can_shift)) in enumerate(zip(cfg["depths"], stage_windows(cfg))):
        grids.append((H, W))
        for d in range(depth):
            x = block(sd, "layers.%d.blocks.%d." % (s, d), x, H, W, cfg["heads"][s], ws, cfg["window"] // 2 if (d % 2 and can_shift) else 0, mut, maps)
        if s < len(cfg["depths"]) - 1:
            x, H, W = merge(sd, "layers.%d.downsample." % s, x, H, W, mut)
            if H * W == 0:  # (a mutant that dropped the only row: nothing is left to compute on)
                return x.new_zeros(B, x.shape[-1]), x, maps, grids + [(H, W)]
    region = layer_norm(x, sd["norm.weight"], sd["norm.bias"])
    return region.mean(1), region, maps, grids


def catches(mut, gh, gw, cfg):
    """must the image whose patch grid is gh x gw tell mutant `mut` from the statement?"""
    ws_of = stage_windows(cfg)
    grids, h, w = [], gh, gw
    for s in range(len(cfg["depths"])):
        grids.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    merged = grids[:-1]
    if mut == "pad_before_norm":
        return any(h % ws or w % ws for (h, w), (ws, _) in zip(grids, ws_of))
    if mut == "swap_hw":
        return gh != gw
    if mut in ("merge_drops_odd_line", "merge_pad_outside_stats"):
        return any(h % 2 or w % 2 for (h, w) in merged)
    if mut == "shift_one_axis":
        return any(sh and d >= 2 for (_, sh), d in zip(ws_of, cfg["depths"]))
    raise KeyError(mut)


# ---- running it ------------------------------------------------------------------------------------------------------------------
def to64(sd, grad=False):
    out = {k: v.detach().double().clone() for k, v in sd.items() if v.is_floating_point()}
    if grad:
        for v in out.values():
            v.requires_grad_(True)
    return out


def loss_of(cls, region, pr):
    """the scalar the tests differentiate: every output takes part"""
    return (cls * pr.to(cls.dtype)).sum() + region.sum() * 0.01


_CACHE = {}


def run(key, sd, img, cfg, pr, mut=None):
    """forward + backward of the statement in fp64, computed once per key -> dict(cls, region, grads, maps, grids)"""
    if key not in _CACHE:
        p = to64(sd, grad=True)
        cls, region, maps, grids = features(p, img.double(), cfg, mut)
        loss_of(cls, region, pr).backward()
        _CACHE[key] = dict(cls=cls.detach(), region=region.detach(), grads={k: v.grad for k, v in p.items() if v.grad is not None},
                           maps=[m.detach() for m in maps], grids=grids)
    return _CACHE[key]


def rel(a, b):
    """relative L2 error of a against the fp64 b"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()
