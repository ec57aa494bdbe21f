"""Analysis of trained backbones (the reference's analyze_models.py): attention entropy, attention maps of chosen queries, thresholded
attention masks, and the correspondence score between two views -- batched, on the device.

For a VisionTransformer nothing here forms an attention matrix: the entropy of every softmax row and the probability rows of a few
queries come from the statistics mode of the flash-attention kernels (csrc/flash_attn.hip, ops.global_attn_stats), on every
block in one backbone pass.  The reference loops over images at batch size 1 because `forward_selfattention` returns [B, nH, N, N] per
block.  Swin backbones have two routes (SWIN_STATS): "maps", the default, keeps the window maps of `forward_selfattention` and reduces
them in torch; "fused" takes the statistics mode of the window kernels (csrc/window_attn.hip, window_attn_big.hip,
ops.window_attn_stats) block by block in one backbone pass and forms no map.  `swin_attention_rows` puts the attention of
chosen pixel positions back on the token grid of any block.  A Vision Longformer (MsViT) goes block pair by block pair in one backbone
pass: its sliding-chunk stages through the statistics mode of the fused per-chunk kernels (csrc/chunk_attn.hip, ops.chunk_attn_stats;
DESIGN §11), its full-attention stages through the flash statistics, so no L x L tensor exists where the kernels support the shape;
`vil_attention_rows` returns the attention of pixel positions or global tokens on each stage's grid.  Plotting, the two augmented views and the per-head ordering of the figures
stay with the caller."""
import math
import os

import torch

from . import functional as Fn
from .models.swin_transformer import SwinTransformer, _grid, _hw_of
from .models.vision_longformer import Long2DSCSelfAttention, MsViT, _pair_params
from .models.vision_transformer import VisionTransformer

_LOG2E = 1.0 / math.log(2.0)
_UNITS = {"bits": _LOG2E, "nats": 1.0}

# how attention_entropy (and AttentionEntropyMeter through it) measures a SwinTransformer: "maps" reduces the maps of
# forward_selfattention(n=2), all blocks' [B * nW, nH, N, N] alive at once; "fused" asks every block for its statistics and forms no map
_SWIN_STATS_ROUTES = ("maps", "fused")
SWIN_STATS = os.environ.get("ESVIT_SWIN_ATTN_STATS", "maps")


def _swin_stats_route():
    if SWIN_STATS not in _SWIN_STATS_ROUTES:
        raise ValueError("ESVIT_SWIN_ATTN_STATS / analysis.SWIN_STATS: maps or fused, not %r" % (SWIN_STATS,))
    return SWIN_STATS


_swin_stats_route()


def _is_vit(model):
    return isinstance(model, VisionTransformer)


def _vit_block_stats(model, images, queries, blocks, want_rows):
    """one backbone pass under no_grad; the statistics of the chosen blocks' attention on those blocks' inputs"""
    depth = len(model.blocks)
    blocks = list(range(depth)) if blocks is None else [int(b) % depth for b in blocks]
    ents, rows = [], []
    # (crops beyond the one-window kernels advance through the flash forward where it exists: the batched-GEMM route would form P)
    with torch.no_grad(), Fn._long_attention("flash"):
        x = model._tokens(images)
        for i, blk in enumerate(model.blocks):
            if i in blocks:
                e, r = Fn.vit_block_attention_stats(x, blk.attn.num_heads, blk._params(), queries if want_rows else None)
                ents.append(e)
                rows.append(r)
            if i < max(blocks):
                x = blk(x, dp=None)
    order = [sorted(set(blocks)).index(b) for b in blocks]  # (blocks were visited in ascending order)
    return [ents[j] for j in order], [rows[j] for j in order]


def _query_index(queries, N, device):
    idx = torch.as_tensor(list(queries) if isinstance(queries, range) else queries).reshape(-1).long()
    if idx.numel() and not (0 <= int(idx.min()) and int(idx.max()) < N):
        raise ValueError("query indices must lie in [0, %d)" % N)
    return idx.to(device)


def _swin_block_stats(model, images, blocks, slots_of=None):
    """one backbone pass under no_grad that stops after the last chosen block: per chosen block (flat index over all stages, ascending)
    the statistics call on the block's input, then the block's ordinary forward -> {block: (entropy, rows, geometry)}.
    slots_of(block index, stage, geometry) -> the listed window slots of that block, or None"""
    want, out, i = set(blocks), {}, 0
    with torch.no_grad():
        x, hw = model._tokens(images), model._image_grid(images)
        for li, layer in enumerate(model.layers):
            for blk in layer.blocks:
                if i in want:
                    H, W = _grid(x.shape[1], hw)
                    geom = Fn.geometry(H, W, blk.window_size, blk.shift_size, x.device)
                    slots = None if slots_of is None else slots_of(i, li, geom)
                    ent, rows = Fn.swin_block_attention_stats(x, geom, blk.num_heads, blk.attn.relative_position_index, blk._params(), slots)
                    out[i] = (ent, rows, geom)
                if i == max(want):
                    return out
                x, _ = blk(x, hw=hw)
                i += 1
            x = layer._down(x, hw)
            hw = _hw_of(layer, hw)
    return out


def _vil_block_stats(model, images, blocks, queries_of=None):
    """one backbone pass under no_grad that walks the stages as MsViT._stage does and stops after the last chosen block pair: per chosen
    pair (flat index over all stages) the statistics call on the pair's input, then the pair's ordinary forward -> {pair: (entropy, rows,
    (nglo, nx, ny))}.  queries_of(pair index, stage, tokens) -> the listed query tokens of that pair, or None.  While it advances the
    pass asks for the fused chunk route (the fourth `chunk` entry) and the flash forward: no L x L tensor where the kernels exist"""
    want, out, i = set(blocks), {}, 0
    with torch.no_grad(), Fn._long_attention("flash"):
        nB, _, H, W = images.shape
        src, nchw = images, True
        for li, (layer, cfg) in enumerate(zip(model._layers(), model.layer_cfgs)):
            x, nx, ny = layer[0](src, nB, H, W, nchw)
            sparse = isinstance(layer[1].attn, Long2DSCSelfAttention)
            chunk = (model._chunk_table(cfg['g'], nx, ny, cfg['f'], x.device), cfg['g'], cfg['f'] * ny, cfg['f']) if sparse else None
            for b in range(1, len(layer), 2):
                prm = _pair_params(layer[b], layer[b + 1])
                if i in want:
                    q = None if queries_of is None else queries_of(i, li, x.shape[1])
                    ent, rows = Fn.vil_block_attention_stats(x, cfg['h'], chunk, prm, q)
                    out[i] = (ent, rows, (cfg['g'], nx, ny))
                if i == max(want):
                    return out
                x = Fn.vil_block(x, cfg['h'], None, chunk, prm)
                i += 1
            src, H, W, nchw = x[:, cfg['g']:].contiguous(), nx, ny, False
    return out


def attention_entropy(model, images, queries=None, unit="bits"):
    """Shannon entropy of the attention distribution of every query token, block by block.

    VisionTransformer: -> fp32 [depth, B, nH, N], or [depth, B, nH, len(queries)] for a list of query tokens (token 0 is the class
    token).  One backbone pass without gradients; the entropy is accumulated beside the running softmax statistics, no N x N tensor
    exists at any point.  SwinTransformer: -> a list with one tensor [B * nW, nH, ws^2] (or [..., len(queries)]) per block, from the
    window maps of `forward_selfattention(images, n=2)`; `swin_window_to_grid` puts such a tensor back on the token grid of its block
    (`model.feature_grid(H, W)` lists the grids).  MsViT (Vision Longformer): -> a list with one tensor [B, nH_l, N_l] (or
    [..., len(queries)], the indices checked against every pair's N_l) per (AttnBlock, MlpBlock) pair over all stages, tokens in the
    order [globals | grid row-major] (`vil_tokens_to_grid` splits such a tensor; `model.feature_grid(H, W)` lists (nglo, nx, ny)); a
    local token's entropy is over the keys it sees.  Any other backbone: TypeError.

    unit: "bits" (the reference's log2) or "nats".  Convention 0 log 0 = 0: a probability that underflowed to zero contributes nothing.
    The reference's `(-p * torch.log2(p)).sum(-1)` (analyze_models.py:116-135) evaluates 0 * -inf there and returns NaN for the row.

    images: one batch [B, 3, H, W] (H and W need not be equal), or a list of batches of different shapes --
    then a list of results in the same order, one pass per batch (the reference's loop feeds one picture at a time)."""
    if unit not in _UNITS:
        raise ValueError("unit: bits or nats, not %r" % (unit,))
    if isinstance(images, (list, tuple)):
        return [attention_entropy(model, im, queries, unit) for im in images]
    k = _UNITS[unit]
    if _is_vit(model):
        ents, _ = _vit_block_stats(model, images, None, None, False)
        ent = torch.stack(ents)
        if queries is not None:
            ent = ent.index_select(3, _query_index(queries, ent.shape[3], ent.device))
        return ent * k if k != 1.0 else ent
    if isinstance(model, SwinTransformer) and _swin_stats_route() == "fused":
        depth = sum(len(layer.blocks) for layer in model.layers)
        stats = _swin_block_stats(model, images, range(depth))
        out = []
        for i in range(depth):
            e = stats[i][0]
            if queries is not None:
                e = e.index_select(2, _query_index(queries, e.shape[2], e.device))
            out.append(e * k if k != 1.0 else e)
        return out
    if isinstance(model, SwinTransformer):
        with torch.no_grad():
            maps = model.forward_selfattention(images, n=2)
        out = []
        for p in maps:
            e = torch.special.entr(p.float()).sum(-1)
            if queries is not None:
                e = e.index_select(2, _query_index(queries, e.shape[2], e.device))
            out.append(e * k if k != 1.0 else e)
        return out
    if isinstance(model, MsViT):
        stats = _vil_block_stats(model, images, range(model.depth))
        out = []
        for i in range(model.depth):
            e = stats[i][0]
            if queries is not None:
                e = e.index_select(2, _query_index(queries, e.shape[2], e.device))
            out.append(e * k if k != 1.0 else e)
        return out
    raise TypeError("attention_entropy: VisionTransformer and SwinTransformer backbones (and MsViT) only, not %s (its attention is neither "
                    "one global softmax per image, nor Swin's window maps, nor Vision Longformer's sliding chunks)" % type(model).__name__)


def swin_window_to_grid(values, H, W, window, shift):
    """a per-window-slot tensor of one Swin block, [B * nW, nH, ws^2] (the window-ordered entropies of `attention_entropy`, one query
    row or column of an attention map), back on the block's H x W token grid -> [B, nH, H, W], through the slot -> token map the
    kernels walk (Fn.geometry: zero padding to a multiple of the window, the cyclic shift and the partition in one table).  The slots
    of the padding are dropped.  window, shift: the block's own (`blk.window_size`, `blk.shift_size`)."""
    geom = Fn.geometry(int(H), int(W), int(window), int(shift), values.device)
    N, nW = geom.N, geom.nW
    if values.dim() != 3 or values.shape[2] != N or values.shape[0] % nW:
        raise ValueError("swin_window_to_grid: expected [B * %d, nH, %d] for a %d x %d grid in %d x %d windows, got %s"
                         % (nW, N, H, W, window, window, tuple(values.shape)))
    B, nH = values.shape[0] // nW, values.shape[1]
    slots = values.reshape(B, nW, nH, N).permute(0, 2, 1, 3).reshape(B, nH, nW * N)
    return slots.index_select(2, geom.tok2win.long()).reshape(B, nH, H, W)  # (tok2win: the slot of every token)


def attention_rows(model, images, queries, blocks=None):
    """the attention maps of the listed query tokens, what `attentions[0, :, query, :]` reads of `forward_selfattention`, for every
    image and every chosen block: -> fp32 [len(blocks), B, nH, len(queries), N].  blocks: indices into model.blocks (default: the last
    block).  VisionTransformer only.  images: a batch of any (H, W), or a list of batches -> a list in the same order."""
    if isinstance(images, (list, tuple)):
        return [attention_rows(model, im, queries, blocks) for im in images]
    if not _is_vit(model):
        raise TypeError("attention_rows: VisionTransformer backbones only, not %s" % type(model).__name__)
    if queries is None or len(queries) == 0:
        raise ValueError("attention_rows: at least one query token")
    blocks = [len(model.blocks) - 1] if blocks is None else list(blocks)
    _, rows = _vit_block_stats(model, images, queries, blocks, True)
    return torch.stack(rows)


def swin_attention_rows(model, images, points, blocks=None):
    """what the pixel positions `points` = [(y, x), ...] attend to in the chosen blocks of a SwinTransformer, on each block's own token
    grid.  In stage l a point is the token (y // s, x // s), s = patch_size * 2^l, of the grid model.feature_grid(H, W)[l]; a point
    outside it is a ValueError.  blocks: flat block indices over all stages, negatives allowed (default: the last block).  One backbone
    pass that stops after the last chosen block; no attention map is formed where the window kernels have their statistics mode.
    -> one (rows, pad_mass) pair per chosen block, in the given order: rows fp32 [B, nH, nq, H_l, W_l], the probabilities of the query's
    window on the block's token grid (shift and padding undone through Fn.geometry's maps; zero outside the window), and pad_mass fp32
    [B, nH, nq], the probability on the zero-pad key slots of that window: rows.sum((-1, -2)) + pad_mass = 1.
    attention_mass_masks(rows.flatten(-2)) thresholds them.  images: a batch of any (H, W), or a list of batches -> a list of results."""
    if isinstance(images, (list, tuple)):
        return [swin_attention_rows(model, im, points, blocks) for im in images]
    if not isinstance(model, SwinTransformer):
        raise TypeError("swin_attention_rows: SwinTransformer backbones only, not %s" % type(model).__name__)
    pts = [(int(y), int(x)) for y, x in points]
    if not pts:
        raise ValueError("swin_attention_rows: at least one point")
    stage_of = [li for li, layer in enumerate(model.layers) for _ in layer.blocks]
    depth = len(stage_of)
    chosen = [depth - 1] if blocks is None else [int(b) for b in blocks]
    if not chosen or any(not -depth <= b < depth for b in chosen):
        raise ValueError("swin_attention_rows: block indices must lie in [%d, %d), got %r" % (-depth, depth, chosen))
    chosen = [b % depth for b in chosen]
    grids = model.feature_grid(images.shape[2], images.shape[3])
    P = model.patch_embed.patch_size[0]
    tokens = {}
    for li in sorted(set(stage_of[b] for b in chosen)):
        (gh, gw), s = grids[li], P << li
        for y, x in pts:
            if not (0 <= y // s < gh and 0 <= x // s < gw):
                raise ValueError("swin_attention_rows: point (%d, %d) lies outside the %d x %d token grid of stage %d (cell side %d)"
                                 % (y, x, gh, gw, li, s))
        tokens[li] = torch.tensor([(y // s) * gw + x // s for y, x in pts])

    def slots_of(i, li, geom):
        assert (geom.H, geom.W) == tuple(grids[li]), ((geom.H, geom.W), grids[li])
        return geom.tok2win.long()[tokens[li].to(geom.tok2win.device)]  # (tok2win: the slot of every token)

    stats = _swin_block_stats(model, images, chosen, slots_of)
    out = []
    for b in chosen:
        _, win_rows, geom = stats[b]
        B, nH, nq, N = win_rows.shape
        T = geom.tokens
        slots = slots_of(b, stage_of[b], geom)
        tok = geom.win2tok.long().view(geom.nW, N)[slots // N]  # [nq, N]: the token of every key slot of the query's window, -1 = pad
        pad = tok < 0
        dst = torch.where(pad, torch.full_like(tok, T), tok).view(1, 1, nq, N).expand(B, nH, nq, N)  # (pad slots: a column that is dropped)
        grid = win_rows.new_zeros(B, nH, nq, T + 1).scatter_(-1, dst, win_rows)[..., :T]
        out.append((grid.reshape(B, nH, nq, geom.H, geom.W), (win_rows * pad.view(1, 1, nq, N)).sum(-1)))
    return out


def vil_tokens_to_grid(values, nglo, nx, ny):
    """a per-token tensor of one Vision Longformer stage, [..., nglo + nx * ny] in the order [globals | grid row-major] (the entropies of
    `attention_entropy`, a probability row), split as `vil_attention_rows` returns it -> (grid [..., nx, ny], glob [..., nglo])"""
    nglo, nx, ny = int(nglo), int(nx), int(ny)
    if values.dim() < 1 or values.shape[-1] != nglo + nx * ny:
        raise ValueError("vil_tokens_to_grid: expected [..., %d] for %d global tokens and a %d x %d grid, got %s"
                         % (nglo + nx * ny, nglo, nx, ny, tuple(values.shape)))
    return values[..., nglo:].reshape(*values.shape[:-1], nx, ny), values[..., :nglo]


def vil_attention_rows(model, images, points, blocks=None):
    """what the `points` attend to in the chosen block pairs of an MsViT, on each stage's own token grid.  A point is a pixel position
    (y, x) -- in stage l the token (y // s_l, x // s_l), s_l the product of the stage patch sizes, of the grid
    model.feature_grid(H, W)[l]; a position outside it is a ValueError -- or an int g: global token g of the block's stage (a stage
    without it: ValueError).  blocks: flat pair indices over all stages, negatives allowed (default: the last pair).  One backbone pass
    that stops after the last chosen pair; no L x L tensor is formed where the kernels have their statistics modes.
    -> one (rows, glob) pair per chosen block, in the given order: rows fp32 [B, nH, nq, nx_l, ny_l], the probabilities on the stage's
    grid (zero outside the query's neighbourhood in a sliding-chunk stage), and glob fp32 [B, nH, nq, nglo_l], those on the stage's
    global tokens: rows.sum((-1, -2)) + glob.sum(-1) = 1.  attention_mass_masks(rows.flatten(-2)) thresholds them.
    images: a batch of any (H, W), or a list of batches -> a list of results."""
    if isinstance(images, (list, tuple)):
        return [vil_attention_rows(model, im, points, blocks) for im in images]
    if not isinstance(model, MsViT):
        raise TypeError("vil_attention_rows: MsViT backbones only, not %s" % type(model).__name__)
    pts = [int(p) if isinstance(p, int) or (torch.is_tensor(p) and p.dim() == 0) else (int(p[0]), int(p[1])) for p in points]
    if not pts:
        raise ValueError("vil_attention_rows: at least one point")
    stage_of = [li for li, cfg in enumerate(model.layer_cfgs) for _ in range(cfg['n'])]
    depth = len(stage_of)
    chosen = [depth - 1] if blocks is None else [int(b) for b in blocks]
    if not chosen or any(not -depth <= b < depth for b in chosen):
        raise ValueError("vil_attention_rows: block indices must lie in [%d, %d), got %r" % (-depth, depth, chosen))
    chosen = [b % depth for b in chosen]
    grids = model.feature_grid(images.shape[2], images.shape[3])
    tokens, s = {}, 1
    for li, cfg in enumerate(model.layer_cfgs):
        s *= cfg['p']
        if li not in set(stage_of[b] for b in chosen):
            continue
        nglo, nx, ny = grids[li]
        tok = []
        for p in pts:
            if isinstance(p, int):
                if not 0 <= p < nglo:
                    raise ValueError("vil_attention_rows: stage %d has %d global tokens, no global token %d" % (li, nglo, p))
                tok.append(p)
            else:
                y, x = p
                if not (0 <= y // s < nx and 0 <= x // s < ny):
                    raise ValueError("vil_attention_rows: point (%d, %d) lies outside the %d x %d token grid of stage %d (cell side %d)"
                                     % (y, x, nx, ny, li, s))
                tok.append(nglo + (y // s) * ny + x // s)
        tokens[li] = tok
    stats = _vil_block_stats(model, images, chosen, lambda i, li, N: tokens[li])
    out = []
    for b in chosen:
        _, rows, (nglo, nx, ny) = stats[b]
        assert (nglo, nx, ny) == tuple(grids[stage_of[b]]), ((nglo, nx, ny), grids[stage_of[b]])
        out.append(vil_tokens_to_grid(rows, nglo, nx, ny))
    return out


def attention_mass_masks(rows, threshold=0.6):
    """the thresholded masks of analyze_models.py:168-176 for any batch of attention rows [..., N]: sort each row ascending, normalise it
    to sum 1, and keep the entries whose cumulative sum exceeds 1 - threshold (the largest entries, holding `threshold` of the mass)
    -> bool, the shape of `rows`, in the rows' own order."""
    val, idx = torch.sort(rows, dim=-1)
    val = val / val.sum(-1, keepdim=True)
    keep = torch.cumsum(val, dim=-1) > (1 - threshold)
    return torch.zeros_like(keep).scatter_(-1, idx, keep)


class AttentionEntropyMeter:
    """per-(block, head) mean over images of the mean-over-queries attention entropy: the dataset-level figure of the reference
    (analyze_models.py:805-829: batch 1, `queries=range(49)`, a running mean over images), for batches of any size.  Sums are kept on the
    device in fp64; update() does not synchronise with the host."""

    def __init__(self, unit="bits"):
        self.unit = unit
        self.total = None
        self.images = 0

    def update(self, model, images, queries=None):
        """images: a batch, or a list of batches of different shapes (each image counts once whatever its size)"""
        if isinstance(images, (list, tuple)):
            for im in images:
                self.update(model, im, queries)
            return self
        ent = attention_entropy(model, images, queries, self.unit)
        if isinstance(ent, list):  # Swin: a window is a sample of its block; the heads differ from stage to stage -> a list per block
            # (MsViT: one row per image; mean(0) * B is the sum over the images)
            per = [e.double().mean(-1).mean(0) * images.shape[0] for e in ent]
            self.total = per if self.total is None else [a + b for a, b in zip(self.total, per)]
        else:
            per = ent.double().mean(-1).sum(1)  # [depth, nH]: summed over the images
            self.total = per if self.total is None else self.total + per
        self.images += images.shape[0]
        return self

    def update_from(self, model, loader, queries=None):
        """a GpuEvalLoader or any iterable of (images, ...) batches"""
        dev = next(model.parameters()).device
        for batch in loader:
            images = batch[0] if isinstance(batch, (tuple, list)) else batch
            self.update(model, images.to(dev, non_blocking=True), queries)
        return self

    def compute(self):
        """-> fp64 [depth, nH] (SwinTransformer: a list of [nH of the block] per block)"""
        if self.total is None:
            raise RuntimeError("AttentionEntropyMeter.compute: no update yet")
        if isinstance(self.total, list):
            return [t / self.images for t in self.total]
        return self.total / self.images


def correspondence_scores(fea1, fea2, grid_hw, cell, top=10, flipped=True):
    """the correspondence measurement of analyze_models.py:302-354 for a batch of image pairs.  fea1, fea2 [B, T, C]: region tokens of
    two views on a grid_hw = (rows, columns) grid, T = rows * columns (a class token is dropped by the caller); cell: the side of a grid
    cell in pixels.  Every token of view 1 is matched to its most similar token of view 2 (cosine similarity; the first index on
    ties); of the `top` matches with the highest similarity (stable descending order) the distance between the two cell centres
    (row, column) * cell + cell / 2 is taken -- to the horizontally mirrored centre of view 1 when `flipped` -- and a match is correct
    when that distance is 0.
    -> (accuracy [B], distance_error [B], sims_sorted [B, T]); the reference's third return value is sims_sorted[:, min(top, T - 1)]."""
    o = Fn.ops_module()
    B, T, C = fea1.shape
    gh, gw = grid_hw
    assert fea2.shape == fea1.shape and gh * gw == T, (fea1.shape, fea2.shape, grid_hw)
    z1 = o.l2norm_fwd(fea1.float().contiguous().view(B * T, C))[0].view(B, T, C)
    z2 = o.l2norm_fwd(fea2.float().contiguous().view(B * T, C))[0].view(B, T, C)
    ld = -(-T // 8) * 8
    sim = o.batched_nt(z1, z2, ld)[:, :, :T]
    best = sim.max(-1).values
    ar = torch.arange(T, device=sim.device)
    match = torch.where(sim == best.unsqueeze(-1), ar, T).min(-1).values  # the first index that holds the maximum
    sims_sorted, order = torch.sort(best, dim=-1, descending=True, stable=True)
    n = min(top, T)
    src = order[:, :n]
    dst = match.gather(1, src)
    y1, x1 = (src // gw) * cell + cell / 2.0, (src % gw) * cell + cell / 2.0
    y2, x2 = (dst // gw) * cell + cell / 2.0, (dst % gw) * cell + cell / 2.0
    if flipped:
        x1 = gw * cell - x1
    dist = ((x1 - x2) ** 2 + (y1 - y2) ** 2).sqrt()
    return (dist == 0).float().mean(-1), dist.mean(-1), sims_sorted
