"""What tests/test_window_stats_{cpu,gpu}.py share: the fp64 entropy and listed rows of the window softmax, taken from the statement of
tests/window_attn_ref.py (its case table as it stands, its probabilities `attn` and their per-element bound `bd_attn`), the slot list of
every case, the bounds, and three mutants of the reduction.

Bounds (u = 2^-24; derived, none fitted, none read from a file).  P the fp64 probabilities of a row, x_k = s_k - m = ln P_k - ln P_max
(the row's maximum has x = 0), NK = 64 or 224 key columns of the kernel.
  rows      a listed row is the row of P the forward's probability variant stores, computed the same way: |row_k - P_k| <= bd_attn_k,
            the bound of window_attn_ref.py (derived bound, doubled in bf16, floor 2^-100, the allowance for the device's exp).
  entropy   H = -sum_k P_k ln P_k, so dH = -sum_k (ln P_k + 1) dP_k and to first order |dH| <= sum_k (|ln P_k| + 1) bd_attn_k.  (Below
            the floor, where P_k may be 0 in fp64, |ln P_k| is taken at 1e-300: p -> -p ln p is below 6e-29 on [0, 2^-100].)
            The kernels do not sum -p ln p: they form H = ln l - (sum_k e_k x_k) / l beside the softmax's own sum l.  The error of l and
            of ln l is the error of the normaliser, inside bd_attn (its (NK + 3) u term).  What is new is the second sum: NK products
            and additions, the reciprocal and the final product and difference, (NK + 4) u sum_k P_k |x_k|, doubled in bf16 like every
            bound of window_attn_ref.py, plus its floor.
            bd_ent = sum_k (|ln P_k| + 1) bd_attn_k + twice (NK + 4) u sum_k P_k |x_k| + 2^-100
  range     0 <= H <= ln N + bd_ent (sum >= 1 because the maximum contributes e^0 = 1, and x <= 0: both terms are non-negative).
The fp32 restatement (the fall-back route of functional.window_attention_stats over oracle/ops_ref.py: entr of its maps) is held to
these bounds on every case by the CPU test, so they are known to be achievable before a GPU sees them."""
import functools
import math
import types

import torch

from tests import window_attn_ref as WR

SENTINEL = -7.0e4


def slot_list(case):
    """the listed slots of a case: first and last slot of the first and of the last window, a slot whose 16-slot tile is otherwise all
    pad (the live slot of the tile with the fewest live slots; slot 48 of a 7 x 7 window is alone in its tile whatever the map), and
    that slot once more"""
    g = WR.geometry(case)
    N, nW, tok = g["N"], g["nW"], g["tok"]
    best = None
    for w in range(nW):
        for j in range(-(-N // 16)):
            live = [i for i in range(16 * j, min(16 * j + 16, N)) if int(tok[w, i]) >= 0]
            if live and (best is None or len(live) < best[0]):
                best = (len(live), w * N + live[-1])
    lonely = best[1]
    return [0, N - 1, (nW - 1) * N, nW * N - 1, lonely, lonely]


def lonely_tile_live(case):
    """live slots in the tile of slot_list's fifth entry (1 wherever the case has such a tile)"""
    g = WR.geometry(case)
    N, s = g["N"], slot_list(case)[4]
    w, i = s // N, s % N
    j = i // 16
    return sum(1 for k in range(16 * j, min(16 * j + 16, N)) if int(g["tok"][w, k]) >= 0)


def rows_of(attn, case, slots):
    """attn [Bw, nH, N, N] -> the listed rows [nB, nH, nq, N]"""
    g = WR.geometry(case)
    N, nW = g["N"], g["nW"]
    s = torch.as_tensor(slots)
    a = attn.view(case["nB"], nW, case["nH"], N, N)
    return a[:, s // N, :, s % N].permute(1, 2, 0, 3)


def _entropy(P):
    return torch.special.entr(P).sum(-1)


@functools.lru_cache(maxsize=None)
def _reference(name, dt):
    case = WR.BY_NAME[name]
    ref = WR.reference(case, dt)
    g = WR.geometry(case)
    P, bd = ref["attn"], ref["bd_attn"]
    twice = 2.0 if dt == torch.bfloat16 else 1.0
    lnP = torch.log(P.clamp(min=1e-300))
    x = (lnP - lnP.amax(-1, keepdim=True)).abs()
    bd_ent = ((lnP.abs() + 1) * bd).sum(-1) + twice * (g["NK"] + 4) * WR.U * (P * x).sum(-1) + WR.FLOOR
    slots = slot_list(case)
    return dict(ent=_entropy(P), bd_ent=bd_ent, rows=rows_of(P, case, slots), bd_rows=rows_of(bd, case, slots), slots=slots)


def reference(case, dt):
    """fp64 entropy [Bw, nH, N] and listed rows [nB, nH, nq, N] with their bounds, once per process"""
    return _reference(case["name"], dt)


MUTANTS = ("pad_keys_out", "mask_ignored", "neighbour_window")


def mutant(case, dt, which):
    """a restated reduction with one mistake -> (entropy, rows) in fp64
      pad_keys_out      the zero-pad key slots are left out of the entropy
      mask_ignored      the softmax without the additive -100 of the region labels
      neighbour_window  a listed row read at the same slot of the next window"""
    ref, g = WR.reference(case, dt), WR.geometry(case)
    N, nW, nB = g["N"], g["nW"], case["nB"]
    P = ref["attn"]
    slots = slot_list(case)
    if which == "pad_keys_out":
        live = ref["live"].view(nB * nW, 1, 1, N).double()
        return (torch.special.entr(P) * live).sum(-1), rows_of(P, case, slots)
    if which == "mask_ignored":
        if "masked" not in ref:
            return _entropy(P), rows_of(P, case, slots)
        lift = torch.where(ref["masked"], 100.0, 0.0).repeat(nB, 1, 1).view(nB * nW, 1, N, N)
        Q = P * torch.exp(lift)
        Q = Q / Q.sum(-1, keepdim=True)
        return _entropy(Q), rows_of(Q, case, slots)
    assert which == "neighbour_window"
    moved = [((s // N + 1) % nW) * N + s % N for s in slots]
    return _entropy(P), rows_of(P, case, moved)


def metrics(case, dt, ent, rows):
    """err / bound of the entropy and the rows, the range of the entropy, and row sums (a listed row sums to 1 within the sum of its bounds)"""
    ref = reference(case, dt)
    N = WR.geometry(case)["N"]
    ent, rows = ent.detach().cpu().double().view_as(ref["ent"]), rows.detach().cpu().double()
    m = dict(ratio_entropy=WR.ratio(ent, ref["ent"], ref["bd_ent"]), ratio_rows=WR.ratio(rows, ref["rows"], ref["bd_rows"]))
    m["equal_entropy_range"] = float(bool((ent >= 0).all()) and bool((ent <= math.log(N) + ref["bd_ent"]).all()))
    m["ratio_row_sum"] = float(((rows.sum(-1) - 1).abs() / ref["bd_rows"].sum(-1)).max())
    return m


def block_statement(qkv, qb, table, win2tok, region_ids, nB, L, nH, ws, scale, dt):
    """the statement of window_attn_ref.py for the qkv of a model's block instead of a case of the table: token-ordered qkv [nB L, 3C]
    (values of dt), qkv bias and table fp32, win2tok / region_ids flat [nW N] -> dict of fp64 P [nB nW, nH, N, N], its derived bound
    bd_attn (no allowance for the device's exp: the table's cases leave it a factor 2.5), the entropy and bd_ent as in _reference, and
    the pad key slots [nW, N].  A pad slot holds the bias as the kernels stage it: rounded to dt, q times scale."""
    N = ws * ws
    tok = win2tok.detach().cpu().long().view(-1, N)
    nW, hd = tok.shape[0], qkv.shape[1] // 3 // nH
    NK = 64 if N <= 64 else 224
    eq, _, _, twice = WR._eps(dt)
    X = qkv.detach().cpu().double().view(nB, L, 3, nH, hd)[:, tok.clamp(min=0).reshape(-1)].view(nB * nW, N, 3, nH, hd).clone()
    X[:, :, 0] *= scale
    pad = (tok < 0).repeat(nB, 1)
    padrow = qb.detach().cpu().to(dt).double().view(3, nH, hd).clone()
    padrow[0] *= scale
    X[pad] = padrow
    q, k = X[:, :, 0].permute(0, 2, 1, 3), X[:, :, 1].permute(0, 2, 1, 3)
    bias = table.detach().cpu().double()[WR.rel_index(ws).reshape(-1)].view(N, N, nH).permute(2, 0, 1)
    S = q @ k.transpose(-1, -2) + bias
    aqk = q.abs() @ k.abs().transpose(-1, -2)
    ab_S = aqk + bias.abs()
    if region_ids is not None:
        reg = region_ids.detach().cpu().long().view(nW, N)
        mask = torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0).repeat(nB, 1, 1).view(nB * nW, 1, N, N)
        S, ab_S = S + mask, ab_S + mask.abs()
    xs = S - S.max(-1, keepdim=True).values
    P = torch.softmax(S, -1)
    t = eq * aqk + (hd + 2) * WR.U * ab_S + (3 * xs.abs() + 2) * WR.U
    r = t + (P * t).sum(-1, keepdim=True) + (NK + 3) * WR.U
    bd = twice * P * r + WR.FLOOR
    lnP = torch.log(P.clamp(min=1e-300))
    first = ((lnP.abs() + 1) * bd).sum(-1)
    return dict(attn=P, bd_attn=bd, ent=_entropy(P), first_order=first,
                bd_ent=first + twice * (NK + 4) * WR.U * (P * xs.abs()).sum(-1) + WR.FLOOR, pad=tok < 0, tok=tok)


def geom_of(case, dev):
    """the fields of functional.WindowGeometry that window_attention_stats reads, from the case's own geometry"""
    g = WR.geometry(case)
    return types.SimpleNamespace(nW=g["nW"], N=g["N"], ws=g["ws"], win2tok=g["tok"].reshape(-1).to(torch.int32).to(dev),
                                 region_ids=g["reg"].reshape(-1).to(torch.int32).to(dev) if g["reg"] is not None else None)
