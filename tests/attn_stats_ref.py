"""Not a test: fp64 statements that tests/test_attn_stats_cpu.py and tests/test_attn_stats_gpu.py compare against.

  stats64            entropy (nats), probability rows and log-sum-exp of softmax(scale q k^T), from the qkv values as they are
  blocked_entropy64  the kernel's online recurrence over 64-key blocks (csrc/flash_attn.hip: stats_entropy), in fp64
  correspondence_ref the per-image correspondence measurement, one Python loop per image"""
import math

import torch

BLOCK = 64  # keys per block of the kernels (flash_attn.hip: BLKT)


def scores64(qkv, B, N, nH, hd, scale):
    """fp64 scores [B, nH, N, N] of qkv [B N, 3C] (columns [3][nH][hd])"""
    q, k, _ = qkv.double().view(B, N, 3, nH, hd).permute(2, 0, 3, 1, 4)
    return scale * (q @ k.transpose(-2, -1))


def stats_of_scores64(s):
    """scores [..., N] -> (entropy in nats with 0 log 0 = 0, probabilities, log-sum-exp)"""
    s = s.double()
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    return torch.special.entr(p).sum(-1), p, lse


def stats64(qkv, B, N, nH, hd, scale, queries=None):
    """-> (entropy [B, nH, N], rows [B, nH, nq, N] or None, lse [B, nH, N]), all fp64"""
    ent, p, lse = stats_of_scores64(scores64(qkv, B, N, nH, hd, scale))
    rows = None
    if queries is not None:
        rows = p.index_select(2, torch.as_tensor(list(queries), dtype=torch.long, device=p.device))
    return ent, rows, lse


def blocked_entropy64(s, block=BLOCK):
    """the online recurrence of the entropy kernel on fp64 scores [..., N]: per row, over key blocks of `block`, a running maximum m,
    l = sum e^(s - m) and u = sum e^(s - m) (s - m); when the maximum moves to m', alpha = e^(m - m'):
    u <- alpha (u + (m - m') l), l <- alpha l, then the block's own terms are added.  H = ln l - u / l."""
    s = s.double()
    N = s.shape[-1]
    m = torch.full(s.shape[:-1], -3.0e38, dtype=torch.float64, device=s.device)
    l = torch.zeros_like(m)
    u = torch.zeros_like(m)
    for k0 in range(0, N, block):
        sb = s[..., k0:k0 + block]
        mn = torch.maximum(m, sb.max(-1).values)
        alpha = torch.exp(m - mn)
        d = sb - mn.unsqueeze(-1)
        e = torch.exp(d)
        u = alpha * (u + (m - mn) * l) + (e * d).sum(-1)
        l = alpha * l + e.sum(-1)
        m = mn
    return torch.log(l) - u / l, m + torch.log(l)


def correspondence_ref(fea1, fea2, grid_hw, cell, top=10, flipped=True):
    """one image pair: fea1, fea2 [T, C] on a (rows, columns) grid.  Cosine similarity of every token of view 1 with every token of
    view 2; a token's match is the FIRST token of view 2 that attains its row maximum.  The tokens of view 1 are ranked by that
    maximum, highest first, ties in their original order (Python's sorted is stable).  Over the first `top` of them: the distance between
    the centre of the token's cell -- mirrored left-right within the image when `flipped` -- and the centre of its match's cell;
    accuracy = the share with distance 0, error = the mean distance.  -> (accuracy, distance_error, the similarities in ranked order)"""
    gh, gw = grid_hw
    T = fea1.shape[0]
    assert T == gh * gw
    a = fea1.double() / fea1.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    b = fea2.double() / fea2.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    return correspondence_of_sim(a @ b.t(), grid_hw, cell, top, flipped)


def correspondence_of_sim(sim, grid_hw, cell, top=10, flipped=True):
    """the same from a given similarity matrix [T, T] (so that exact ties can be planted)"""
    gh, gw = grid_hw
    T = sim.shape[0]
    width = gw * cell
    best, match = [], []
    for i in range(T):
        row = sim[i].tolist()
        mx = max(row)
        best.append(mx)
        match.append(row.index(mx))
    ranked = sorted(range(T), key=lambda i: best[i], reverse=True)
    centre = lambda t: ((t // gw) * cell + cell / 2.0, (t % gw) * cell + cell / 2.0)  # noqa: E731  (y, x)
    dists = []
    for i in ranked[:top]:
        (y1, x1), (y2, x2) = centre(i), centre(match[i])
        if flipped:
            x1 = width - x1
        dists.append(math.sqrt((x1 - x2) ** 2 + (y1 - y2) ** 2))
    acc = sum(1.0 for d in dists if d == 0) / len(dists)
    return acc, sum(dists) / len(dists), [best[i] for i in ranked], match
