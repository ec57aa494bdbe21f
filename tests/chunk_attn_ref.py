"""fp64 statement of Vision Longformer's sliding-chunk attention on both routes -- the fused kernels of esvit_amd/csrc/chunk_attn.hip behind
ops.sliding_chunk_attn_fwd / _bwd, and the dense route ops.vit_attn_fwd / _bwd(chunk=...) (batched GEMMs + the row softmax of
esvit_amd/csrc/vit_attn.hip, which with chunk=None is every plain ViT) -- that tests/test_chunk_attn_exact_{cpu,gpu}.py compare against, the
case table both share, the bounds, and the mutants the CPU test proves the comparison catches.  Everything is plain index arithmetic on
(nglo, nx, ny, w): tokens are [nglo globals | the nx x ny grid, (x, y) row-major], a local token lives in chunk (x // w, y // w), a query
sees a key when either is global or their chunks differ by at most one in both directions.  The statement calls neither
oracle/ops_ref.chunk_mask nor chunk_geom.h (the CPU test proves its mask equal to both; the restatement enters only as the allowance for
the device's exp).  Inputs are made in the case's dtype and promoted, so bf16 inputs are exact in the reference.  Every output comes with
`ab_*`, the sum of |terms| of its element, and `bd_*`, its bound; all are [B, nH, L, .] and EVERY element of every output is compared.

Bounds (u = 2^-24, b = 2^-9; per element, none is tuned, none is read from a file).  S = scale q.k, x = S - max, P the fp64 probabilities,
ab_S = scale |q|.|k|, delta = dO . out, dS = scale P (dP - delta), dQ = dS k, dK = dS^T q, dV = P^T dO.

Fused route (bf16 only).  Q is not rescaled (eq = 0): the scale multiplies the fp32 scores (`s[r] * scale`, `load_global_rows(.., scale)`).
    ep  P and dS as MFMA operands  `frag_p_regs<bf16>(...)` in chunk_fwd_local / chunk_bwd_dq_local / chunk_bwd_dkv_local       b
        -- and 0 in the global-token kernels (chunk_fwd_global_part, chunk_bwd_global_part: fp32 on the VALU end to end).  A pair
        (query, key) goes through the local kernels when the query is local (out, dQ) resp. the key is local (dK, dV).
    eo  the stored outputs  `store_tile_rows<HD, HDP>(..)`, `(bf16)(num / den)`, `(bf16)s[w]` of the two combine kernels           b
    NK  additions per row: NBS = 448 columns of a local row; cnt <= 512 per range, then nsplit in range order, of a global row
  scores        eS = (hd + 2) u ab_S + u |S|          (the chain of hd products; the product with the scale)
  exponent      t = eS + (3 |x| + 2) u                 (the subtraction; __expf as exp2(x log2 e): |x| u twice, 1 ulp of v_exp_f32); a global
                row adds (3 |m_range - M| + 2) u for `__expf(pz[..64] - M)` of chunk_fwd_global_combine
  probabilities r = expm1(t + E) + (NK + 3) u, E = log sum_k P_k exp(t_k)   (the forward's P; the fused route does not store it).  An error
                of at most t in an exponent is a relative error of at most exp(t) - 1 in the exponential, and the sum of the row moves by
                a factor between exp(-E) and exp(E); to first order this is t + sum_k P_k t_k, and where bf16 stores a score of 300 (the
                dense route in the stress cases, t > 1) only the exact form holds
  lse           E + (NK + 2) u + 3 u (|max| + |log Z|)
  out           (P (r + ep)) |v| + (NK + 1) u ab_out + eo |out|
  backward P    rb = expm1(t + bd_lse)                       (`__expf(s[r] * scale - lq)`: the saved lse carries its own error into the exponent)
  dV            (P (rb + ep))^T |dO| + (NK + 1) u ab_dv + eo |dV|
  dP            (hd + 1) u ab_dP;   delta from the STORED bf16 out (chunk_delta_kernel): e_delta = |dO| . bd_out + (hd + 1) u |dO| . |out|
  dS            e_dS = scale (P rb |dP - delta| + P e_dP + 2 u P (|dP| + |delta|)), and the share of delta, scale P e_delta, apart:
                delta is ONE number per query, so its error reaches dQ as scale e_delta |sum_k P_k k_k| -- the sum, not the sum of
                moduli -- while in dK every query has its own and the moduli add;   as an operand: + ep |dS|
  dQ            (e_dS + ep |dS|) |k| + scale e_delta |P k| + (NK + 2) u ab_dq + eo |dQ|
  dK            (e_dS + scale P e_delta + ep |dS|)^T |q| + (NK + 2) u ab_dk + eo |dK|

Dense route (es = u in fp32, b in bf16: S, P, dP and dS are each stored in the activation dtype by the GEMM epilogue resp. `from_f32<T>`
of softmax_rows_*; GEMM chains of hd resp. Np = N rounded up to 16; the softmax fp32 over N terms).
  scores        eS = (hd + 1) u ab_S + (es + u) |S|
  exponent      t = eS + (3 |x| + 2) u;   r = expm1(t + E) + (N + 3 + 4 steps) u, steps = ceil(Np / (64 V)) rescalings of the running
                sum per lane in softmax_rows_fwd_long_kernel (`sum = sum * __expf(m - mn) + sv`; 0 in the short kernel)
  P             P (r + es)
  out, dV       (P (r + es)) |v| + (Np + 1) u ab_out + es |out|;   the same with |dO|
  dP            (hd + 1) u ab_dP + es |dP|;   dot = sum_j P_j dP_j: e_dot = sum_j (P (r + es) |dP| + P e_dP) + (N + 1) u sum_j P |dP|
  dS            e_dS = scale (P (r + es) |dP - dot| + P e_dP + 3 u P (|dP| + |dot|)) + es |dS|, the share of dot apart as above
  dQ, dK        as above with e_dot for e_delta, ep = 0, (Np + 1) u, es for eo
Both routes: bf16 mode doubles every bound for the neglected higher-order terms (the error of an exponent is doubled BEFORE its exponential:
2 r = expm1(2 (t + E)), E = log(sum_k P_k exp(2 t_k)) / 2, which is the plain doubling to first order); every bound carries the floor 2^-100.  Device __expf: its
error cannot be derived here, so every bound is the larger of the derived one and 3 x the error of the fp32 restatement
(oracle/ops_ref.vit_attn_fwd / _bwd on the CPU, same inputs, fp32 activations), that error taken as its maximum over the same (image, head) block.

Case -> kernel facts (facts() computes them; the CPU test holds this table to it).  nsplit ranges of GSPLIT = 512 keys for the global rows,
`last` the tokens of the last range, `live00` the live neighbourhood slots of chunk (0, 0) (of 448), `dead` the (chunk, wave) pairs that
return at tile_live (of 4 per chunk), the dense softmax by Np <= 256 (short) or not (long):
  case             grid   nglo    L    Np  hd  B nH  nsplit last live00 dead softmax
  cell             1x1       1     2    16  32  3  2       1    2      2    3 short
  sub_chunk_noglo  5x5       0    25    32  64  2  3       1   25     25    1 short
  strip            1x22      1    23    32  32  3  2       1   23     15   12 short
  ragged           8x15      1   121   128  48  2  3       1  121    113   10 short
  ragged_t         15x8      2   122   128  64  3  2       1  122    114    8 short
  max_globals      15x15     7   232   240  48  2  3       1  232    203   11 short
  interior         22x22     1   485   496  48  3  2       1  485    197   15 long
  range512         15x34     2   512   512  32  2  3       1  512    198   17 long
  range513         16x32     1   513   528  64  3  2       2    1    197   17 long
  range1025        32x32     1  1025  1040  32  2  3       3    1    197   14 long
  stress_small     15x15     2   227   240  32  3  2       1  227    198   11 short
  stress_513       16x32     1   513   528  64  2  3       2    1    197   17 long
"""
import functools
import math

import torch

from tests.window_attn_ref import BF, FLOOR, U, data, dt_name, ratio  # noqa: F401  (ratio, dt_name: for the tests)

W = 7
NBS, OWS, GSPLIT = 448, 64, 512
DTYPES = (torch.float32, torch.bfloat16)
ROUTES = ("fused", "dense")
OUTPUTS = {"fused": ("lse", "out", "dq", "dk", "dv"), "dense": ("attn", "out", "dq", "dk", "dv")}
ALIGN = 40.0    # standard deviation of the scores of the stress cases
PLANT, PLANT_OUT = 300.0, 700.0  # planted scores: the row maxima, and the key outside the neighbourhood


def _c(name, nx, ny, nglo, hd, B, nH, stress=False):
    return dict(name=name, nx=nx, ny=ny, nglo=nglo, hd=hd, B=B, nH=nH, L=nglo + nx * ny, stress=stress)


# B and nH are never equal and never both 2: z = b nH + h decodes to (z // nH, z % nH) only
CASES = [
    _c("cell", 1, 1, 1, 32, 3, 2),
    _c("sub_chunk_noglo", 5, 5, 0, 64, 2, 3),
    _c("strip", 1, 22, 1, 32, 3, 2),
    _c("ragged", 8, 15, 1, 48, 2, 3),
    _c("ragged_t", 15, 8, 2, 64, 3, 2),
    _c("max_globals", 15, 15, 7, 48, 2, 3),
    _c("interior", 22, 22, 1, 48, 3, 2),
    _c("range512", 15, 34, 2, 32, 2, 3),
    _c("range513", 16, 32, 1, 64, 3, 2),
    _c("range1025", 32, 32, 1, 32, 2, 3),
    _c("stress_small", 15, 15, 2, 32, 3, 2, stress=True),
    _c("stress_513", 16, 32, 1, 64, 2, 3, stress=True),
]
BY_NAME = {c["name"]: c for c in CASES}


def pad_tokens(N):
    return -(-N // 16) * 16


def table(case):
    """the int32 chunk table of the dense route: -1 for a global token, else (chunk row << 16) | chunk column"""
    x, y = torch.arange(case["nx"]).view(-1, 1), torch.arange(case["ny"]).view(1, -1)
    loc = ((x // W) << 16 | (y // W)).reshape(-1)
    return torch.cat([torch.full((case["nglo"],), -1, dtype=torch.long), loc]).to(torch.int32)


def layout(case, dev, span=True):
    """what ops.* take as `chunk`: the plain table, or (table, nglo, tokens per chunk row)"""
    tab = table(case).to(dev)
    return (tab, case["nglo"], W * case["ny"]) if span else tab


def _xy(case):
    """grid position of every token ([L] each; globals -1)"""
    nglo, ny, L = case["nglo"], case["ny"], case["L"]
    t = torch.arange(L) - nglo
    glob = t < 0
    return torch.where(glob, -1, t // ny), torch.where(glob, -1, t % ny), glob


MUTANTS = {
    # name: (route, the cases the table names for it, what it is)
    "a_wide": ("fused", ("interior", "ragged_t"), "neighbourhood two chunks wide"),
    "b_last_col": ("fused", ("ragged", "strip"), "the last grid column is dead"),
    "c_glob_last_row": ("fused", ("ragged", "ragged_t"), "the globals are invisible to the last chunk row"),
    "d_skip_range_fwd": ("fused", ("range513", "range1025"), "global queries skip the last 512-range, forward"),
    "e_skip_range_bwd": ("fused", ("range513", "range1025"), "the same, in the backward"),
    "f_no_rescale": ("fused", ("range513", "stress_513"), "range partials combined without exp(m_range - M)"),
    "g_lse_no_log": ("fused", ("cell", "interior"), "log(sum) left out of the lse"),
    "h_p_102": ("fused", ("cell",), "P x 1.02 in the backward"),
    "i_q_bf16": ("fused", ("stress_small",), "scale * q rounded to bf16"),
    "j_z_decode": ("fused", ("strip", "ragged"), "b = z % B in place of z / nH"),
    "k_hd48_pad": ("fused", ("ragged", "max_globals"), "channels 48..63 of a head_dim-48 head read from the next head"),
    "l_glob_glob": ("fused", ("cell", "max_globals"), "global keys receive nothing from the global queries in dK / dV"),
    "m_dead_zero": ("fused", ("sub_chunk_noglo", "cell"), "dead key slots score 0 instead of being removed"),
    "n_span": ("dense", ("interior", "range513"), "b_lo / b_hi not widened to the vector width"),
    "o_pad_cols": ("dense", ("cell", "max_globals"), "pad columns j >= N take part in the sum"),
}


def mask(case, mutant=None, vec=8):
    """[L, L] bool: may query i see key j, from index arithmetic alone (mutants a, b, c, n change it)"""
    x, y, glob = _xy(case)
    cx, cy = x // W, y // W
    reach = 2 if mutant == "a_wide" else 1
    near = ((cx[:, None] - cx[None, :]).abs() <= reach) & ((cy[:, None] - cy[None, :]).abs() <= reach)
    m = near | glob[:, None] | glob[None, :]
    loc = ~glob
    if mutant == "b_last_col":
        m = m & ~(loc[:, None] & (y == case["ny"] - 1)[None, :])
    if mutant == "c_glob_last_row":
        m = m & ~((loc & (cx == (case["nx"] - 1) // W))[:, None] & glob[None, :])
    if mutant == "n_span":  # a local query's scan [lo, hi) shrunk to whole vectors instead of widened
        rowtok, nglo, L = W * case["ny"], case["nglo"], case["L"]
        lo = nglo + (cx - 1).clamp(min=0) * rowtok
        hi = (nglo + (cx + 2) * rowtok).clamp(max=L)
        lo_in, hi_in = -(-lo // vec) * vec, (hi // vec) * vec
        j = torch.arange(L)[None, :]
        lost = ((j >= lo[:, None]) & (j < lo_in[:, None])) | ((j >= hi_in[:, None]) & (j < hi[:, None]))
        m = m & ~(loc[:, None] & lost)
    return m


def facts(case):
    """what the case table claims of the kernels: nsplit, tokens of the last range, live neighbourhood slots of chunk (0, 0), (chunk, wave)
    pairs without a live own slot, the dense softmax kernel"""
    nx, ny, nglo, L = case["nx"], case["ny"], case["nglo"], case["L"]
    nsplit = -(-L // GSPLIT)
    live00 = nglo + sum(1 for t in range(9 * W * W) if 0 <= t // (3 * W) - W < nx and 0 <= t % (3 * W) - W < ny)
    slot447 = NBS - 1 - nglo
    live447 = nglo == 7 and 0 <= slot447 // (3 * W) - W < nx and 0 <= slot447 % (3 * W) - W < ny
    dead = 0
    for cr in range(-(-nx // W)):
        for cc in range(-(-ny // W)):
            for wave in range(OWS // 16):
                if not any(s < W * W and cr * W + s // W < nx and cc * W + s % W < ny for s in range(16 * wave, 16 * wave + 16)):
                    dead += 1
    Np = pad_tokens(L)
    return dict(grid="%dx%d" % (nx, ny), nglo=nglo, L=L, Np=Np, hd=case["hd"], B=case["B"], nH=case["nH"], nsplit=nsplit, last=L - (nsplit - 1) * GSPLIT,
                live00=live00, dead=dead, softmax="short" if Np <= 256 else "long", slot447=bool(live447))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _walsh(hd, p):
    """+-1 pattern of period 2^(p + 1): mutually orthogonal, and orthogonal to the constant"""
    return 1.0 - 2.0 * ((torch.arange(hd) >> p) & 1).double()


def plants(case):
    """the planted maxima of a stress case: (image, query, key, pattern, score, what).  Each pair gets its score through a direction of its
    own (the head's sign vector times a Walsh pattern), which no other token has a component in"""
    nglo, ny, nx, L = case["nglo"], case["ny"], case["nx"], case["L"]
    tok = lambda x, y: nglo + x * ny + y  # noqa: E731
    out = [(0, 0, L - 1 if L > GSPLIT else tok(3, 3), 0, PLANT, "global query on the last token (the single token of the last range)"),
           (1, 0, tok(2, 5), 0, PLANT, "global query on a token of the first range"),
           (0, tok(9, 9), nglo - 1, 1, PLANT, "local query on a global key"),
           (1, tok(7, 7), tok(0, 0), 1, PLANT, "local query on the far corner of its neighbourhood"),
           (0, tok(12, 3), tok(12, 3), 2, PLANT, "local query on itself"),
           (1, tok(8, 6), tok(8, 14), 3, PLANT_OUT, "the largest q.k of the image on a key just outside the neighbourhood")]
    assert nx >= 15 and ny >= 15
    return out


@functools.lru_cache(maxsize=None)
def _inputs(name, dt):
    c = BY_NAME[name]
    B, nH, hd, L = c["B"], c["nH"], c["hd"], c["L"]
    C = nH * hd
    qkv = data((name, "qkv"), (B * L, 3 * C), torch.float32)
    dout = data((name, "dout"), (B * L, C), torch.float32)
    scale = float(torch.tensor(hd ** -0.5, dtype=torch.float32))
    if c["stress"]:
        # q = a s + noise, k = b s + noise with one sign vector s per head, a, b ~ N(0, ALIGN / sqrt(hd)): scores of deviation ALIGN
        sig = math.sqrt(ALIGN / math.sqrt(hd))
        s = torch.sign(data((name, "s"), (1, 1, nH, hd), torch.float32))
        ab = data((name, "ab"), (B * L, 2, nH, 1), torch.float32, sig)
        x = qkv.view(B * L, 3, nH, hd)
        for (img, qi, kj, pat, score, _) in plants(c):
            # the planted query carries a = sig and no noise (its other scores keep the deviation ALIGN), the planted key b = 0 (no other
            # query finds it); the pair meets in w, the sign vector times the plant's Walsh pattern, with scale hd amp^2 = score
            w = s[0, 0] * _walsh(hd, pat).float()  # [nH, hd]
            amp = math.sqrt(score / (scale * hd))
            ab[img * L + qi, 0] = sig
            ab[img * L + kj, 1] = 0.0
            x[img * L + qi, 0] = amp * w
            x[img * L + kj, 1] += amp * w
        x[:, :2] += ab * s
    return dict(qkv=qkv.to(dt), dout=dout.to(dt), scale=scale)


def inputs(case, dt):
    """qkv [B L, 3C] / dout [B L, C] in dt, scale as the fp32 the kernel receives"""
    return _inputs(case["name"], dt)


def heads(t, case, parts):
    """token-major [>= B L, parts nH hd] -> fp64 [parts, B, nH, L, hd] (parts = 1 drops the first axis)"""
    B, nH, hd, L = case["B"], case["nH"], case["hd"], case["L"]
    x = t.detach().cpu().double()[:B * L].view(B, L, parts, nH, hd).permute(2, 0, 3, 1, 4)
    return x[0] if parts == 1 else x


# ---- the statement -----------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.float().to(torch.bfloat16).double()


def _ebar(P, t):
    """log sum_k P_k exp(t_k): how far errors of at most t_k in the exponents move the log of the sum (>= sum_k P_k t_k, equal to first order)"""
    return torch.log((P * torch.exp(t.clamp(max=700.0))).sum(-1, keepdim=True))


def statement(case, dt, route, mutant=None, want_bounds=True):
    """-> dict of fp64 tensors: attn [B, nH, L, L], lse [B, nH, L], out / dq / dk / dv [B, nH, L, hd], mask [L, L]; with want_bounds the
    ab_* and (derived) bd_* companions for `route`.  mutant: a key of MUTANTS"""
    assert route in ROUTES and (mutant is None or mutant in MUTANTS)
    x = inputs(case, dt)
    B, nH, hd, L, nglo = case["B"], case["nH"], case["hd"], case["L"], case["nglo"]
    scale, Np = x["scale"], pad_tokens(L)
    bf = dt == torch.bfloat16
    vec = 8 if bf else 4
    q, k, v = heads(x["qkv"], case, 3)
    do = heads(x["dout"], case, 1)
    M0 = mask(case)
    Mm = mask(case, mutant, vec)
    glob = torch.arange(L) < nglo
    nsplit = -(-L // GSPLIT)
    last0 = (nsplit - 1) * GSPLIT
    rng = torch.arange(L) // GSPLIT  # range of every key

    S = scale * (q @ k.transpose(-1, -2))
    if mutant == "i_q_bf16":
        S = _bf16(scale * q) @ k.transpose(-1, -2)
    if mutant == "k_hd48_pad" and hd == 48:  # columns 48..63 of the staged rows hold what follows the head in the token's row
        rows = x["qkv"].double().view(B, L, 3 * nH * hd)
        C = nH * hd
        for h in range(nH):
            eq_ = rows[:, :, h * hd + hd:h * hd + hd + 16]
            ek_ = rows[:, :, C + h * hd + hd:C + h * hd + hd + 16]
            S[:, h] += scale * (eq_ @ ek_.transpose(-1, -2))
    ninf = float("-inf")
    Mf = Mm.clone()
    if mutant == "d_skip_range_fwd" and nsplit > 1:
        Mf[:nglo, last0:] = False
    Sf = S.masked_fill(~Mf, ninf)
    m = Sf.max(-1, keepdim=True).values
    e = torch.exp(Sf - m)
    Z = e.sum(-1, keepdim=True)
    if mutant == "m_dead_zero":  # the dead slots of a local row's 448 take part with score 0 (their v is 0)
        ndead = torch.where(glob, 0, NBS - M0.sum(-1)).double().view(1, 1, L, 1)
        Z = Z + ndead * torch.exp(-m)
    if mutant == "o_pad_cols":
        Z = Z + (Np - L) * torch.exp(-m)
    if mutant == "f_no_rescale" and nglo:  # every range keeps the weights relative to its own maximum
        mr = torch.stack([Sf[:, :, :nglo, r * GSPLIT:(r + 1) * GSPLIT].max(-1).values for r in range(nsplit)], -1)  # [B, nH, nglo, nsplit]
        eg = torch.exp(Sf[:, :, :nglo] - mr[..., rng])
        e = torch.cat([eg, e[:, :, nglo:]], 2)
        Z = torch.cat([eg.sum(-1, keepdim=True), Z[:, :, nglo:]], 2)
    P = e / Z
    lse = (m + (0.0 if mutant == "g_lse_no_log" else torch.log(Z))).squeeze(-1)
    if mutant == "j_z_decode":  # unit z reads image z % B: the output rows land right, the lse, indexed by z, does not
        z = torch.arange(B * nH)
        lse = lse[z % B, z % nH].view(B, nH, L)
    O = P @ v
    # backward: the fused route rebuilds P from the saved lse under the backward's mask; the dense route reads the stored P
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    if mutant is None or route == "dense":
        Pb = P
    else:
        Pb = torch.exp(S.masked_fill(~Mm, ninf) - lse.unsqueeze(-1))
    if mutant == "h_p_102":
        Pb = Pb * 1.02
    Pq, Pkv = Pb, Pb
    if mutant == "e_skip_range_bwd" and nsplit > 1:  # the last range's block of chunk_bwd_global_part does nothing
        Pq, Pkv = Pb.clone(), Pb.clone()
        Pq[:, :, :nglo, last0:] = 0.0
        Pkv[:, :, last0:, :nglo] = 0.0
    if mutant == "l_glob_glob":
        Pkv = Pb.clone()
        Pkv[:, :, :nglo, :nglo] = 0.0
    dSq, dSkv = scale * Pq * (dP - delta), scale * Pkv * (dP - delta)
    dQ, dK, dV = dSq @ k, dSkv.transpose(-1, -2) @ q, Pkv.transpose(-1, -2) @ do
    res = dict(attn=P, lse=lse, out=O, dq=dQ, dk=dK, dv=dV, mask=M0)
    if not want_bounds:
        return res
    assert mutant is None

    aq, ak, av, ado = q.abs(), k.abs(), v.abs(), do.abs()
    ab_S = scale * (aq @ ak.transpose(-1, -2))
    Sa = torch.where(M0, S.abs(), 0.0)
    xs = torch.where(M0, (S - m).abs(), 0.0)
    mx, lz = m.abs(), torch.log(Z).abs()
    ab_O, ab_dV, ab_dP = P @ av, P.transpose(-1, -2) @ ado, ado @ av.transpose(-1, -2)
    dS = dSq
    ab_dS = scale * P * (dP.abs() + delta.abs())
    ab_dQ, ab_dK = ab_dS @ ak, ab_dS.transpose(-1, -2) @ aq
    Pk = (P @ k).abs()
    twice = 2.0 if bf else 1.0
    if route == "fused":
        assert bf, "the fused route is bf16 only"
        NK = torch.where(glob, GSPLIT + nsplit, NBS).double().view(1, 1, L, 1)
        NKc = NK.view(1, 1, 1, L)
        ep_q = torch.where(glob, 0.0, BF).view(1, 1, L, 1)
        ep_kv = torch.where(glob, 0.0, BF).view(1, 1, 1, L)
        eo = BF
        t = (hd + 2) * U * ab_S + U * Sa + (3 * xs + 2) * U
        if nglo:
            mr = torch.stack([S[:, :, :nglo, r * GSPLIT:(r + 1) * GSPLIT].max(-1).values for r in range(nsplit)], -1)
            t[:, :, :nglo] += (3 * (mr[..., rng] - m[:, :, :nglo]).abs() + 2) * U
        Ebar = _ebar(P, twice * t) / twice
        r = torch.expm1(twice * (t + Ebar)) / twice + (NK + 3) * U
        bd_lse = Ebar + (NK + 2) * U + 3 * U * (mx + lz)
        bd_O = (P * (r + ep_q)) @ av + (NK + 1) * U * ab_O + eo * O.abs()
        rb = torch.expm1(twice * (t + bd_lse)) / twice
        bd_dV = (P * (rb + ep_kv)).transpose(-1, -2) @ ado + (NKc.transpose(-1, -2) + 1) * U * ab_dV + eo * dV.abs()
        e_dP = (hd + 1) * U * ab_dP
        e_delta = (ado * bd_O).sum(-1, keepdim=True) + (hd + 1) * U * (ado * O.abs()).sum(-1, keepdim=True)
        e_dS = scale * (P * rb * (dP - delta).abs() + P * e_dP + 2 * U * P * (dP.abs() + delta.abs()))
        bd_dQ = (e_dS + ep_q * dS.abs()) @ ak + scale * e_delta * Pk + (NK + 2) * U * ab_dQ + eo * dQ.abs()
        bd_dK = (e_dS + scale * P * e_delta + ep_kv * dS.abs()).transpose(-1, -2) @ aq + (NKc.transpose(-1, -2) + 2) * U * ab_dK + eo * dK.abs()
        bd_P = P * r
    else:
        es = BF if bf else U
        steps = -(-Np // (64 * vec)) if Np > 256 else 0
        t = (hd + 1) * U * ab_S + (es + U) * Sa + (3 * xs + 2) * U
        Ebar = _ebar(P, twice * t) / twice
        r = torch.expm1(twice * (t + Ebar)) / twice + (L + 3 + 4 * steps) * U
        bd_lse = Ebar + (L + 2) * U + 3 * U * (mx + lz)
        rP = P * (r + es)
        bd_P = rP
        bd_O = rP @ av + (Np + 1) * U * ab_O + es * O.abs()
        bd_dV = rP.transpose(-1, -2) @ ado + (Np + 1) * U * ab_dV + es * dV.abs()
        e_dP = (hd + 1) * U * ab_dP + es * dP.abs()
        e_dot = (rP * dP.abs() + P * e_dP).sum(-1, keepdim=True) + (L + 1) * U * (P * dP.abs()).sum(-1, keepdim=True)
        e_dS = scale * (rP * (dP - delta).abs() + P * e_dP + 3 * U * P * (dP.abs() + delta.abs())) + es * dS.abs()
        bd_dQ = e_dS @ ak + scale * e_dot * Pk + (Np + 1) * U * ab_dQ + es * dQ.abs()
        bd_dK = (e_dS + scale * P * e_dot).transpose(-1, -2) @ aq + (Np + 1) * U * ab_dK + es * dK.abs()
    res.update(ab_attn=P, ab_lse=(mx + lz).squeeze(-1), ab_out=ab_O, ab_dq=ab_dQ, ab_dk=ab_dK, ab_dv=ab_dV)
    for kk, bd in (("attn", bd_P), ("lse", bd_lse.squeeze(-1)), ("out", bd_O), ("dq", bd_dQ), ("dk", bd_dK), ("dv", bd_dV)):
        res["bd_" + kk] = twice * bd + FLOOR
    return res


# ---- the fp32 restatement's error (the device's __expf) and the final bounds -------------------------------------------------------
def restatement(case, dt):
    """oracle/ops_ref.vit_attn_fwd / _bwd in fp32 on the dt-valued inputs -> the statement's layout"""
    from oracle import ops_ref
    x = inputs(case, dt)
    B, nH, L, scale = case["B"], case["nH"], case["L"], x["scale"]
    tab = table(case)
    old = ops_ref.act_dtype()
    ops_ref.set_act_dtype(torch.float32)
    try:
        out, saved = ops_ref.vit_attn_fwd(x["qkv"].float(), B, L, nH, scale, chunk=tab)
        dqkv = ops_ref.vit_attn_bwd(x["dout"].float(), saved, B, L, nH, scale)
    finally:
        ops_ref.set_act_dtype(old)
    qh, kh = saved[0][0], saved[0][1]
    s = (scale * (qh @ kh.transpose(-2, -1))).masked_fill(~ops_ref.chunk_mask(tab), float("-inf"))
    return unpack(case, out=out, dqkv=dqkv, attn=saved[1], lse=torch.logsumexp(s, -1))


def unpack(case, out=None, dqkv=None, attn=None, lse=None):
    """a library's tensors -> fp64 CPU tensors in the statement's layout (attn: [B nH, Np, Np] or [B, nH, L, L]; pads cut off)"""
    B, nH, L = case["B"], case["nH"], case["L"]
    res = {}
    if out is not None:
        res["out"] = heads(out, case, 1)
    if dqkv is not None:
        d3 = heads(dqkv, case, 3)
        res.update(dq=d3[0], dk=d3[1], dv=d3[2])
    if attn is not None:
        a = attn.detach().cpu().double()
        res["attn"] = a.view(B, nH, a.shape[-2], a.shape[-1])[:, :, :L, :L]
    if lse is not None:
        res["lse"] = lse.detach().cpu().double().view(B, nH, L)
    return res


@functools.lru_cache(maxsize=None)
def _reference(name, dt, route):
    case = BY_NAME[name]
    ref = statement(case, dt, route)
    got = restatement(case, dt)
    for kk in ("attn", "lse", "out", "dq", "dk", "dv"):
        err = (got[kk] - ref[kk]).abs()
        dims = (2,) if kk == "lse" else (2, 3)
        ref["bd_" + kk] = torch.maximum(ref["bd_" + kk], 3 * err.amax(dims, keepdim=True).expand_as(err))
    return {kk: vv for kk, vv in ref.items() if not kk.startswith("ab_")}  # (kept for the process: the [L, L] companions are dropped)


def reference(case, dt, route):
    """the statement with its final bounds, once per process"""
    return _reference(case["name"], dt, route)


def metrics(case, dt, route, got, outputs=None):
    """err / bound over EVERY element of every output the run has"""
    ref = reference(case, dt, route)
    return {"ratio_" + kk: ratio(got[kk], ref[kk], ref["bd_" + kk]) for kk in (outputs or OUTPUTS[route]) if kk in got}


def check(entry, case, dt, route, m, record=None, where="cpu"):
    """print (and record) every figure, then assert: ratios <= 1, equalities 1"""
    tag = dict(test="chunk_attn_exact", entry=entry, route=route, case=case["name"], dtype=dt_name(dt), where=where)
    if record is not None:
        record(**tag, **m)
    print("OBSERVED", tag, m)
    bad = ["%s = %.4g" % (kk, vv) for kk, vv in m.items() if (kk.startswith("equal") and vv != 1.0) or (kk.startswith("ratio") and not vv <= 1.0)]
    assert not bad, (entry, route, case["name"], tag["dtype"], bad)
