"""fp64 statement of the attention statistics of Vision Longformer's sliding-chunk softmax -- the mode ws | ESVIT_ATTN_SLIDING_CHUNK |
ESVIT_ATTN_CHUNK_STATS of esvit_window_attn_fwd (esvit_amd/csrc/chunk_attn.hip behind ops.chunk_attn_stats) -- for ARBITRARY inputs:
stats64(qkv, B, nH, hd, nglo, nx, ny, scale, queries) -> the entropy of every softmax row in nats, the probability rows of the listed
queries over all L tokens, and a bound for every element of both.  tests/test_chunk_stats_{cpu,gpu}.py compare against it.  The mask is
restated as index arithmetic on (nglo, nx, ny): tokens are [nglo globals | the nx x ny grid, (x, y) row-major], a local token lives in
chunk (x // 7, y // 7), a query sees a key when either is global or their chunks differ by at most one in both directions.  Constants and
the case table come from tests/chunk_attn_ref.py, whose fused-route bound chain is restated here (the CPU test holds the two equal on
every case).

Bounds (u = 2^-24; per element, none is tuned, none is read from a file).  S = scale q.k, m the row's maximum over the keys it sees,
x = S - m <= 0, Z = sum_k e^x_k, P = e^x / Z, ab_S = scale |q|.|k|.  From chunk_attn_ref (fused route; bf16 inputs are exact):
  scores        eS = (hd + 2) u ab_S + u |S|     (`mma(..)` resp. `row_dots` / the rows kernel's dot: the chain of hd products; `s[r] * scale`
                resp. `scale * (float)q`)
  exponent      t = eS + (3 |x| + 2) u           (`p[i][r] - m`, `__expf`); a global row adds (3 |m_range - M| + 2) u for `__expf(dm)` of
                chunk_stats_global_combine_kernel
  NK            additions per row: 448 columns of a local row; 512 per range, then nsplit in range order, of a global row.  (The rows
                kernel adds at most L / 256 terms per thread, six in the wave and four across the waves: fewer than either.)
  Ebar          log sum_k P_k exp(t_k): how far the exponents' errors move the log of the sum
  r             expm1(t + Ebar) + (NK + 3) u: the relative error of a probability e^x / Z formed from the device's exponentials and sum
Rows (`row[k] = row[k] / l` of chunk_stats_rows_kernel: its own maximum, its own sum l):
  bd_rows = P r  (bd_attn of that chain)  + 2 u P  (one fp32 ulp of the stored quotient)  + 2 u P  (one ulp of the normaliser l)
Entropy.  The kernel forms H = ln l - (sum_k e_k d_k) / l with d_k = s_k - m, e_k = __expf(d_k), l = sum e_k (`__logf(sum) - us / sum`).
A common shift of every d_k (the error of the maximum itself) changes ln l and the quotient by the same amount and cancels, so the
scores' own errors, the roundings and the device functions remain:
  (sum_k e_k d_k) / l = sum_k p_k d_k with p_k = e_k / l of relative error r_k and d_k of error eS_k + u |x_k| (the subtraction);
                the product e_k d_k rounds once more (u |x_k|):               A = sum_k P_k (r_k |x_k| + eS_k + 2 u |x_k|)
                its NK additions and the division:                             (NK + 2) u sum_k P_k |x_k|
  ln l          the exponents (Ebar), the NK additions of l, 3 ulp of `__logf`:  Ebar + (NK + 2) u + 3 u |ln Z|
  the final subtraction                                                          u (|ln Z| + sum_k P_k |x_k|)
  bd_ent = A + Ebar + (NK + 2) u + (NK + 3) u (sum_k P_k |x_k| + |ln Z|)        (4 u |ln Z| <= (NK + 3) u |ln Z|)
  a global row adds the combine's products: `wgt * (Tr + dm * lr)` and `wgt * lr` -- every term e^(s - m_r)(s - m_r) of range r becomes
                w_r e^(s - m_r) ((s - m_r) + (m_r - M)), two numbers of modulus <= |x_k| each, so the sum of moduli is <= 2 sum P |x|; three
                roundings of the products and the inner sum and one spare on it (8 u sum P |x|), and the two subtractions that form
                s - m_r and m_r - M in place of the one that forms x (2 u sum P |x|):    + 10 u sum_k P_k |x_k|
bf16 mode doubles every bound for the neglected higher-order terms, the error of an exponent BEFORE its exponential, as chunk_attn_ref
does (2 r = expm1(2 (t + Ebar)), Ebar = log(sum_k P_k exp(2 t_k)) / 2); every bound carries the floor 2^-100.  Device __expf / __logf:
their error cannot be derived here, so every bound is the larger of the derived one and 3 x the error of the fp32 restatement
(oracle/ops_ref.vit_attn_fwd on the CPU in fp32 on the same inputs, the entropy reduced in fp32 with torch.special.entr), that error
taken as its maximum over the same (image, head) block.

MUTANTS: wrong statements the comparison must catch, each in the cases named for it (the CPU test holds every one out of its bound by a
factor of 2).
"""
import torch

from tests.chunk_attn_ref import BF, BY_NAME, CASES, FLOOR, GSPLIT, NBS, U, W, _ebar, inputs, table  # noqa: F401  (re-exported for the tests)

MUTANTS = {
    # name: (the cases named for it, what it is)
    "dead_zero": (("sub_chunk_noglo", "cell"), "dead neighbourhood slots enter with score 0"),
    "combine_no_shift": (("range513", "range1025"), "the combine without the (m_r - M) l_r term"),
    "no_rescale": (("range513", "stress_513"), "ranges merged without exp(m_r - M)"),
    "ent_bf16_p": (("interior", "ragged"), "the entropy from bf16-rounded probabilities"),
    "row_no_glob": (("max_globals", "ragged"), "a listed local row misses the global columns"),
    "wide": (("interior", "ragged_t"), "the neighbourhood two chunks wide"),
    "pad_cols": (("cell", "strip"), "the 448 - live padded slots of a local row enter the sum with e = 1"),
}


def mask_of(nglo, nx, ny, reach=1):
    """[L, L] bool: may query i see key j, from index arithmetic alone"""
    L = nglo + nx * ny
    t = torch.arange(L) - nglo
    glob = t < 0
    cx, cy = torch.where(glob, -1, t // ny) // W, torch.where(glob, -1, t % ny) // W
    near = ((cx[:, None] - cx[None, :]).abs() <= reach) & ((cy[:, None] - cy[None, :]).abs() <= reach)
    return near | glob[:, None] | glob[None, :]


def heads64(qkv, B, nH, hd, L):
    """token-major [>= B L, 3 nH hd] -> fp64 q, k [B, nH, L, hd]"""
    x = qkv.detach().cpu().double()[:B * L].view(B, L, 3, nH, hd).permute(2, 0, 3, 1, 4)
    return x[0], x[1]


def default_queries(nglo, nx, ny):
    """every global, the first and the last local token, a chunk-corner token and an interior one, with one duplicate"""
    tok = lambda x, y: nglo + min(x, nx - 1) * ny + min(y, ny - 1)  # noqa: E731
    q = list(range(nglo)) + [nglo, nglo + nx * ny - 1, tok(W - 1, W), tok(W + 3, W + 2)]
    return q + [q[-1]]


def merge_ranges64(S, allowed, mutant=None):
    """the combine's recurrence in fp64 for rows of scores S [..., L] over the keys `allowed`: per 512-key range (m_r, l_r, T_r), then in
    range order with w_r = e^(m_r - M): l = sum w_r l_r, T = sum w_r (T_r + (m_r - M) l_r), H = ln l - T / l -> H"""
    L = S.shape[-1]
    parts = []
    for r0 in range(0, L, GSPLIT):
        s = S[..., r0:r0 + GSPLIT].masked_fill(~allowed[..., r0:r0 + GSPLIT], float("-inf"))
        mr = s.max(-1).values
        d = s - mr.unsqueeze(-1)
        e = torch.exp(d)
        parts.append((mr, e.sum(-1), torch.where(e > 0, e * d, 0.0).sum(-1)))
    M = torch.stack([p[0] for p in parts]).max(0).values
    l, T = torch.zeros_like(M), torch.zeros_like(M)
    for mr, lr, Tr in parts:
        dm = mr - M
        wgt = torch.ones_like(dm) if mutant == "no_rescale" else torch.exp(dm)
        l = l + wgt * lr
        T = T + wgt * (Tr + (0.0 if mutant == "combine_no_shift" else dm * lr))
    return torch.log(l) - T / l


def stats64(qkv, B, nH, hd, nglo, nx, ny, scale, queries=None, mutant=None, want_bounds=True):
    """-> dict of fp64 tensors: ent [B, nH, L], rows [B, nH, nq, L] (queries given), attn [B, nH, L, L], mask [L, L]; with want_bounds
    bd_ent, bd_rows, bd_attn (derived, before the restatement's allowance: bounds())."""
    assert mutant is None or mutant in MUTANTS
    L = nglo + nx * ny
    q, k = heads64(qkv, B, nH, hd, L)
    M0 = mask_of(nglo, nx, ny)
    Mm = mask_of(nglo, nx, ny, 2) if mutant == "wide" else M0
    glob = torch.arange(L) < nglo
    nsplit = -(-L // GSPLIT)
    rng = torch.arange(L) // GSPLIT
    S = scale * (q @ k.transpose(-1, -2))
    Sf = S.masked_fill(~Mm, float("-inf"))
    m = Sf.max(-1, keepdim=True).values
    x = Sf - m
    e = torch.exp(x)
    ex = torch.where(Mm, e * torch.where(Mm, x, 0.0), 0.0)
    Z, T = e.sum(-1, keepdim=True), ex.sum(-1, keepdim=True)
    if mutant in ("dead_zero", "pad_cols"):  # the slots of a local row's 448 that hold no token take part
        ndead = torch.where(glob, 0, NBS - M0.sum(-1)).double().view(1, 1, L, 1)
        if mutant == "dead_zero":  # with score 0: e = exp(0 - m'), d = -m', m' = max(m, 0)
            m2 = torch.where(ndead > 0, m.clamp(min=0.0), m)
            x = Sf - m2
            e = torch.exp(x)
            ex = torch.where(Mm, e * torch.where(Mm, x, 0.0), 0.0)
            Z = e.sum(-1, keepdim=True) + ndead * torch.exp(-m2)
            T = ex.sum(-1, keepdim=True) + ndead * torch.exp(-m2) * (-m2)
        else:
            Z = Z + ndead
    P = e / Z
    ent = (torch.log(Z) - T / Z).squeeze(-1)
    if mutant in ("combine_no_shift", "no_rescale") and nglo:
        ent = torch.cat([merge_ranges64(S[:, :, :nglo], Mm[:nglo].view(1, 1, nglo, L).expand(B, nH, nglo, L), mutant), ent[:, :, nglo:]], 2)
    if mutant == "ent_bf16_p":
        ent = torch.special.entr(P.float().to(torch.bfloat16).double()).sum(-1)
    res = dict(ent=ent, attn=P, mask=M0)
    qi = None
    if queries is not None:
        qi = torch.as_tensor(list(queries)).reshape(-1).long()
        rows = P.index_select(2, qi)
        if mutant == "row_no_glob" and nglo:
            local = (qi >= nglo).view(1, 1, -1, 1)
            cut = rows.clone()
            cut[..., :nglo] = 0.0
            rows = torch.where(local, cut / cut.sum(-1, keepdim=True), rows)
        res["rows"] = rows
    if not want_bounds:
        return res
    assert mutant is None

    twice = 2.0  # the kernels are bf16 only
    ab_S = scale * (q.abs() @ k.abs().transpose(-1, -2))
    Sa = torch.where(M0, S.abs(), 0.0)
    xs = torch.where(M0, x.abs(), 0.0)
    lz = torch.log(Z).abs()
    NK = torch.where(glob, GSPLIT + nsplit, NBS).double().view(1, 1, L, 1)
    eS = (hd + 2) * U * ab_S + U * Sa
    t = eS + (3 * xs + 2) * U
    if nglo:
        mr = torch.stack([S[:, :, :nglo, r * GSPLIT:(r + 1) * GSPLIT].max(-1).values for r in range(nsplit)], -1)
        t[:, :, :nglo] += (3 * (mr[..., rng] - m[:, :, :nglo]).abs() + 2) * U
    Ebar = _ebar(P, twice * t) / twice
    r = torch.expm1(twice * (t + Ebar)) / twice + (NK + 3) * U
    bd_P = P * r
    Px = (P * xs).sum(-1, keepdim=True)
    A = (P * (r * xs + torch.where(M0, eS, 0.0) + 2 * U * xs)).sum(-1, keepdim=True)
    bd_H = A + Ebar + (NK + 2) * U + (NK + 3) * U * (Px + lz) + torch.where(glob, 10.0, 0.0).view(1, 1, L, 1) * U * Px
    res.update(bd_attn=twice * bd_P + FLOOR, bd_ent=(twice * bd_H + FLOOR).squeeze(-1))
    if qi is not None:
        res["bd_rows"] = twice * (bd_P + 4 * U * P).index_select(2, qi) + FLOOR
    return res


def restatement32(qkv, B, nH, hd, nglo, nx, ny, scale, queries=None):
    """oracle/ops_ref.vit_attn_fwd in fp32 on the same inputs, the entropy reduced in fp32 -> fp64 ent [B, nH, L], rows or None"""
    from oracle import ops_ref
    L = nglo + nx * ny
    tab = table(dict(nx=nx, ny=ny, nglo=nglo))
    old = ops_ref.act_dtype()
    ops_ref.set_act_dtype(torch.float32)
    try:
        p = ops_ref.vit_attn_fwd(qkv.detach().cpu()[:B * L].float(), B, L, nH, scale, chunk=tab)[1][1]
    finally:
        ops_ref.set_act_dtype(old)
    p = p.view(B, nH, L, L)
    ent = torch.special.entr(p).sum(-1).double()
    rows = None if queries is None else p.index_select(2, torch.as_tensor(list(queries)).reshape(-1).long()).double()
    return ent, rows


def bounds(qkv, B, nH, hd, nglo, nx, ny, scale, queries=None):
    """the statement with its final bounds: the larger of the derived bound and 3 x the error of the fp32 restatement, that error's
    maximum over the (image, head) block -> (dict of stats64, the restatement's (ent, rows))"""
    ref = stats64(qkv, B, nH, hd, nglo, nx, ny, scale, queries)
    ent32, rows32 = restatement32(qkv, B, nH, hd, nglo, nx, ny, scale, queries)
    ref["bd_ent_derived"] = ref["bd_ent"]
    err = (ent32 - ref["ent"]).abs()
    ref["bd_ent"] = torch.maximum(ref["bd_ent"], 3 * err.amax(2, keepdim=True).expand_as(err))
    if queries is not None:
        ref["bd_rows_derived"] = ref["bd_rows"]
        err = (rows32 - ref["rows"]).abs()
        ref["bd_rows"] = torch.maximum(ref["bd_rows"], 3 * err.amax((2, 3), keepdim=True).expand_as(err))
    return ref, (ent32, rows32)


_CASE_REF = {}


def case_reference(case):
    """bounds() of a case of chunk_attn_ref.CASES on its bf16 inputs with default_queries, once per process (left unchanged)"""
    key = case["name"]
    if key not in _CASE_REF:
        x = inputs(case, torch.bfloat16)
        qs = default_queries(case["nglo"], case["nx"], case["ny"])
        ref, r32 = bounds(x["qkv"], case["B"], case["nH"], case["hd"], case["nglo"], case["nx"], case["ny"], x["scale"], qs)
        ref.pop("bd_attn")
        _CASE_REF[key] = (ref, r32, qs)
    return _CASE_REF[key]
