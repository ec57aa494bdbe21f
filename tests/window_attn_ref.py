"""fp64 statement of shifted-window attention (esvit_amd/csrc/window_attn.hip, window_attn_big.hip behind ops.window_attn_fwd / window_attn_bwd /
relpos_bias_bwd) that tests/test_window_attn_{cpu,gpu}.py compare against, the case table both share, and the bounds.  Everything here is
plain index arithmetic: slot -> token by the roll-and-partition formula, pad slots equal to the qkv bias with q scaled, relative-position
bias by the index table, an additive -100 where region labels differ, softmax, P V, the hand-written backward, the scatter of the bias
gradient into the table, the pad-slot dK / dV sums, lse and the probabilities.  The statement calls nothing of oracle/ops_ref.py (the
restatement enters only as the allowance for the device's exp, below, and as one of the libraries run_attention drives).  Inputs are made
in the case's dtype and promoted, so bf16 inputs (the qkv bias included) are exact in the reference.  Every output comes with `ab_*`, the
sum of |terms| of its element, and `bd_*`, its bound.  All per-slot outputs are in window order [Bw, nH, N, head_dim] (to_win below brings
token-ordered tensors there; every token sits in exactly one slot, pad slots read 0).

Bounds (u = 2^-24, b = 2^-9 the half-ulp of bf16; per element, none is tuned, none is read from a file).  NK = 64 or 224 key columns of
the kernel, hd = head_dim, P the fp64 probabilities, x = S - max.  Three rounding points differ by mode:
    eq  staged scale * q            window_attn.hip `xq.set(e, xq.get(e) * scale)` + st16 / window_attn_big.hip `sq.store(Qs, scale, lane)`    u | b
    ep  P and dS as MFMA operands   window_attn.hip `store_frag4<T>(Ps + ...)` (P, then dS), frag_p_regs in both forwards and dq4             0 | b
    eo  the stored outputs          esvit_pack_tile_pair_bf16 / `(float)(bf16)v[dt][r]` in emit, store_tile_rows_t                          0 | b
  scores        eS = eq |q'||k|^T + (hd + 2) u ab_S       (the MFMA chain of hd products started from bias + mask)
  exponent      t = eS + (3 |x| + 2) u                    (the subtraction; __expf modelled as exp2(x log2 e): |x| u twice, 1 ulp of v_exp_f32)
  probabilities r = t + sum_k P_k t_k + (NK + 3) u        (d log P_j = dS_j - sum_k P_k dS_k; NK additions, reciprocal, product)   bd_attn = P r
  lse           sum_k P_k t_k + (NK + 2) u + 3 u (|max| + |log Z|)
  out           (P (r + ep)) |v| + (NK + 1) u ab_out + eo |out|
  dV            (P (r + ep))^T |dO| + (NK + 1) u ab_dv + eo |dV|
  dP            (hd + 1) u ab_dP;   delta: the larger of the two ways the kernels form it -- sum_j P_j dP_j with P from LDS (<= 64 tokens),
                dO . out with the stored forward output (224 slots)
  dS            P (r + ep) |dP - delta| + P (e_dP + e_delta) + 2 u P (|dP| + |delta|);  as an operand: + ep |dS|
  dQ            scale (e_dS |k|) + (NK + 2) u ab_dq + eo |dQ|;      dK: e_dS^T |q'| + (eq + (NK + 1) u) ab_dk + eo |dK|
  dbias         sum over windows of e_dS + (iters + parts + 9) u ab_dbias   (a wave pair adds `iters` windows, the fold adds `parts` slabs
                in eight slices);   dtable: the scatter of that + N u scatter(ab_dbias) (at most N atomics per table row and head)
  dpad          sum over pad slots of the dK / dV bound + (pad slots of the call) u ab_dpad
  bf16 mode doubles every bound for the neglected higher-order terms.  Every bound carries the floor 2^-100: fp32 flushes what lies
  below 2^-126 (exp(-100 - ...) of a masked key), so a difference under the floor does not exist in fp32 -- a mutant that changes
  nothing above it does not apply to the case.
  Device __expf: its error cannot be derived here, so every bound is the larger of the derived one and 3 x the error of the fp32
  restatement (oracle/ops_ref.window_attn_* on the CPU, same inputs, fp32 activations), that error taken as its maximum over the same
  (window, head) block (over the head for dbias / dtable / dpad).

Case -> kernel instance, parts, iters, active wave pairs in the last round (host formulas: forward 1536 / nH pairs at head_dim 32, 1024 / nH at
64; backward 1024 / nH; the 224-slot dQ (+ bias-gradient) kernel 512 / nH, its forward and dK / dV kernels one workgroup per window-head):
  case                 forward                                 parts iters last | backward                             parts iters last
  walk7                attn_fwd4<T, 32>                           64     2   36 | attn_bwd3<T, 32>                        42     3   16
  walk7_hd64           attn_fwd4<T, 64>                           85     2   15 | attn_bwd3<T, 64>                        85     2   15
  walk7_noshift        attn_fwd4<T, 32>                           64     2   36 | attn_bwd3<T, 32>                        42     3   16
  walk_small_w6        attn_fwd4<T, 64>                           42     3   16 | attn_bwd3<T, 64>                        42     3   16
  walk_small_w3        attn_fwd4<T, 64>                           42     3   16 | attn_bwd3<T, 64>                        42     3   16
  walk14               attn_big_fwd3<T, 32>                       48     1   48 | attn_big_bwd_dq4<T, 32> (+ dkv2)        21     3    6
  walk14_hd64          attn_big_fwd3<bf16, 64>                    48     1   48 | dq4<bf16, 64> + bwd_dbias + dkv2        42     2    6
  range7_hd32 / _bias  attn_fwd4<T, 32>                           12     1   12 | attn_bwd3<T, 32>                        12     1   12
  range7_hd64          attn_fwd4<T, 64>                           12     1   12 | attn_bwd3<T, 64>                        12     1   12
  range14 / _bias      attn_big_fwd3<T, 32>                        8     1    8 | attn_big_bwd_dq4<T, 32> (+ dkv2)         8     1    8
  partial_grid         attn_fwd4<T, 64>, N = 37 of a 7 x 7 grid  170     2   30 | attn_bwd3<T, 64>                       170     2   30
(walk() computes the figures; the CPU test holds them to this table, the GPU test holds the backward parts to ops.query(Q_ATTN_BWD_PARTS).)
"""
import functools
import math
import zlib

import torch

U = 2.0 ** -24
BF = 2.0 ** -9
FLOOR = 2.0 ** -100
EXP_OVERFLOW = 88.72  # fp32 exp overflows above log(2^128)
DTYPES = (torch.float32, torch.bfloat16)


def dt_name(dt):
    return {torch.float32: "fp32", torch.bfloat16: "bf16"}[dt]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()) % (2 ** 31))


def data(key, shape, dt, scale=1.0, shift=0.0):
    """seeded values stored as dt (on the CPU)"""
    return (torch.randn(*shape, generator=_gen(*key)) * scale + shift).to(dt)


def _f32(v):
    """a Python float as the kernel receives it"""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- the case table ----------------------------------------------------------------------------------------------------------------
def _c(name, ws, H, shift, nH, hd, nB, W=None, N=None, qk=1.0, align=0.0, tab=0.5, do_shift=0.0, dts=DTYPES, serves=""):
    return dict(name=name, ws=ws, H=H, W=H if W is None else W, shift=shift, nH=nH, hd=hd, nB=nB, N=N, qk=qk, align=align, tab=tab,
                do_shift=do_shift, common=do_shift != 0.0, dts=dts, serves=serves)


# The bf16 bound of a sum over windows (bias gradient, pad rows) is linear in the number of terms, and a dropped round or part is one
# share of that sum: with independent images the share is a random walk and drowns in it.  So in the cases that walk, every image is
# 0.8 x a component all images share + 0.6 x its own (a row taken from the wrong image is still off by 0.6 sigma; the sums over windows
# are coherent), q and k are drawn at scale 0.5 (eS small) and dO around +1 (the pad-slot dV terms of one sign).
# The range cases make scores large the way trained heads do, by alignment: q = a u + noise, k = b u + noise with one sign vector u per
# head and a, b ~ N(0, align / (scale hd)), so that scores have the standard deviation `align` and |q|.|k| is about |q.k|.  Independent
# q and k at scale 5 to 8 reach 89 as well, but through sums that cancel: |q|.|k| is then sqrt(hd) times the score, the bf16 rounding of
# scale q moves a score of 100 by more than 0.5, the bound of a probability exceeds the probability, and nothing separates -100 from -inf
# (measured here: range7_hd64 and range14 in bf16 at scale 8 had no masked key above its bound; at scale 5 the largest masked probability
# at head_dim 64 was 2e-10).
CASES = [
    _c("walk7", 7, 12, 3, 24, 32, 25, qk=0.5, do_shift=1.0, serves="mask, pads and the walk together, both ways"),
    _c("walk7_hd64", 7, 12, 3, 12, 64, 25, qk=0.5, do_shift=1.0, serves="the head_dim-64 instances with a tail"),
    _c("walk7_noshift", 7, 14, 0, 24, 32, 25, qk=0.5, do_shift=1.0, serves="no pads, no mask: dpad exactly 0"),
    _c("walk_small_w6", 6, 6, 0, 24, 64, 100, qk=0.5, do_shift=1.0, serves="one window per image, key tile 3 all -1e30"),
    _c("walk_small_w3", 3, 3, 0, 24, 64, 100, qk=0.5, do_shift=1.0, serves="one window per image, key tiles 1..3 all -1e30"),
    _c("walk14", 14, 24, 7, 24, 32, 12, qk=0.5, do_shift=1.0, serves="mask, pad and walk in the 224-slot kernels; lse"),
    _c("walk14_hd64", 14, 24, 7, 12, 64, 12, qk=0.5, do_shift=1.0, dts=(torch.bfloat16,), serves="the separate bias-gradient kernel"),
    _c("range7_hd32", 7, 12, 3, 24, 32, 3, align=40.0, serves="scores beyond 89; masked keys that keep probability"),
    _c("range7_hd64", 7, 12, 3, 12, 64, 3, align=40.0, serves="the same at head_dim 64"),
    _c("range7_bias", 7, 12, 3, 24, 32, 3, tab=30.0, serves="bias-dominated scores"),
    _c("range14", 14, 24, 7, 6, 32, 2, align=40.0, serves="large scores in the 224-slot kernels"),
    _c("range14_bias", 14, 24, 7, 6, 32, 2, tab=30.0, serves="bias-dominated scores, 224 slots"),
    _c("partial_grid", 7, None, 0, 6, 64, 200, N=37, qk=0.5, do_shift=1.0, serves="N = 37 of a 7 x 7 grid with a non-zero table"),
]
RANGE_QK = ("range7_hd32", "range7_hd64", "range14")
BY_NAME = {c["name"]: c for c in CASES}


def cases(dt):
    return [c for c in CASES if dt in c["dts"]]


def params():
    return [(c, dt) for c in CASES for dt in DTYPES if dt in c["dts"]]


def ids(ps):
    return ["%s-%s" % (c["name"], dt_name(dt)) for c, dt in ps]


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def window_geometry(H, W, ws, shift):
    """-> (tok [nW, ws^2]: token of every window slot or -1, region labels [nW, ws^2] or None).  The padded grid Hp x Wp is rolled by
    -shift and cut into windows: slot (i, j) of window (wi, wj) sits at rolled position (wi ws + i, wj ws + j) and shows the grid
    position ((py + shift) % Hp, (px + shift) % Wp); labels are the 3 x 3 bands of the rolled frame (below Hp - ws, below Hp - shift, rest)"""
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    ar = torch.arange
    py = (ar(Hp // ws).view(-1, 1, 1, 1) * ws + ar(ws).view(1, 1, -1, 1)).expand(Hp // ws, Wp // ws, ws, ws)
    px = (ar(Wp // ws).view(1, -1, 1, 1) * ws + ar(ws).view(1, 1, 1, -1)).expand(Hp // ws, Wp // ws, ws, ws)
    y, x = (py + shift) % Hp, (px + shift) % Wp
    tok = torch.where((y < H) & (x < W), y * W + x, torch.full_like(y, -1)).reshape(-1, ws * ws)
    if not shift:
        return tok, None
    band = lambda p, n: (p >= n - ws).long() + (p >= n - shift).long()  # noqa: E731
    return tok, (3 * band(py, Hp) + band(px, Wp)).reshape(-1, ws * ws)


def rel_index(ws):
    """[ws^2, ws^2]: (qy - ky + ws - 1) (2 ws - 1) + (qx - kx + ws - 1)"""
    p = torch.arange(ws * ws)
    y, x = p // ws, p % ws
    return (y[:, None] - y[None, :] + ws - 1) * (2 * ws - 1) + (x[:, None] - x[None, :] + ws - 1)


@functools.lru_cache(maxsize=None)
def _geometry(name):
    c = BY_NAME[name]
    ws = c["ws"]
    if c["N"] is not None:  # the partial grid: one window per image holding tokens 0 .. N-1, the first N positions of the ws x ws grid
        N, L = c["N"], c["N"]
        tok, reg = torch.arange(N).view(1, N), None
    else:
        N, L = ws * ws, c["H"] * c["W"]
        tok, reg = window_geometry(c["H"], c["W"], ws, c["shift"])
    return dict(tok=tok, reg=reg, nW=tok.shape[0], N=N, L=L, ws=ws, index=rel_index(ws), trows=(2 * ws - 1) ** 2, NK=64 if N <= 64 else 224)


def geometry(case):
    return _geometry(case["name"])


def walk(case):
    """parts / iters / active pairs of the last round, from the host code's formulas"""
    g = geometry(case)
    Bw, nH = case["nB"] * g["nW"], case["nH"]
    if g["N"] <= 64:
        fwd, bwd = max((1536 if case["hd"] == 32 else 1024) // nH, 1), max(1024 // nH, 1)
    else:
        fwd, bwd = Bw, max(512 // nH, 1)
    out = {}
    for k, p in (("fwd", fwd), ("bwd", bwd)):
        p = min(p, Bw)
        it = -(-Bw // p)
        out[k] = (p, it, Bw - (it - 1) * p)
    return out


@functools.lru_cache(maxsize=None)
def _inputs(name, dt):
    c, g = BY_NAME[name], _geometry(name)
    C, rows = c["nH"] * c["hd"], c["nB"] * g["L"]
    qkv, dout = data((name, "qkv"), (rows, 3 * C), torch.float32), data((name, "dout"), (rows, C), torch.float32)
    if c["common"]:
        qkv = 0.6 * qkv + 0.8 * data((name, "qkv0"), (g["L"], 3 * C), torch.float32).repeat(c["nB"], 1)
        dout = 0.6 * dout + 0.8 * data((name, "dout0"), (g["L"], C), torch.float32).repeat(c["nB"], 1)
    qkv[:, :2 * C] *= c["qk"]
    if c["align"]:
        u = torch.sign(data((name, "u"), (1, 1, c["nH"], c["hd"]), torch.float32))
        ab = data((name, "ab"), (rows, 2, c["nH"], 1), torch.float32, math.sqrt(c["align"] / (c["hd"] ** 0.5)))
        qkv[:, :2 * C] += (ab * u).reshape(rows, 2 * C)
    return dict(qkv=qkv.to(dt), qb=data((name, "qb"), (3 * C,), dt, 0.5).float(), table=data((name, "table"), (g["trows"], c["nH"]), torch.float32, c["tab"]),
                dout=(dout + c["do_shift"]).to(dt), scale=_f32(c["hd"] ** -0.5))


def inputs(case, dt):
    """qkv / dout in dt, the qkv bias dt-valued fp32, the table fp32, scale as the fp32 the kernel receives"""
    return _inputs(case["name"], dt)


def to_win(t, case, parts=1):
    """token-ordered [nB L, parts nH hd] -> window order [parts, Bw, nH, N, hd] in fp64 (pad slots 0); parts = 1 drops the first axis"""
    g = geometry(case)
    nB, nH, hd, N, nW = case["nB"], case["nH"], case["hd"], g["N"], g["nW"]
    tok = g["tok"].reshape(-1)
    rows = (torch.arange(nB).view(nB, 1) * g["L"] + tok.clamp(min=0).view(1, -1)).reshape(-1)
    x = t.detach().cpu().double()[rows].view(nB, nW, N, parts, nH, hd) * (tok >= 0).view(1, nW, N, 1, 1, 1)
    x = x.permute(3, 0, 1, 4, 2, 5).reshape(parts, nB * nW, nH, N, hd)
    return x[0] if parts == 1 else x


# ---- the statement -----------------------------------------------------------------------------------------------------------------
MUTANTS = ("prev_mask", "prev_map", "mask_inf", "no_max", "pad_kv_zero", "pad_q_unscaled", "dbias_last_round", "pad_query_dout", "dpad_part",
           "index_stride", "lse_no_max", "pad_keys_kept", "bias_transposed")
OUTPUTS = ("attn", "lse", "out", "dq", "dk", "dv", "dbias", "dtable", "dpad")


def _eps(dt):
    return (BF, BF, BF, 2.0) if dt == torch.bfloat16 else (U, 0.0, 0.0, 1.0)


def statement(case, dt, mutant=None, parts=None, want_bounds=True, images=None):
    """-> dict of fp64 tensors: attn [Bw, nH, N, N], lse [Bw, nH, N], out / dq / dk / dv [Bw, nH, N, hd] (dq of the unscaled q), dbias
    [nH, N, N], dtable [(2 ws - 1)^2, nH], dpad [2 C] (dK then dV summed over the pad slots), masked [nW, N, N] bool; with want_bounds the
    ab_* and (derived) bd_* companions.  Mutants (parts = the wave pairs of the walk being mutated):
      prev_mask / prev_map  window bw >= parts takes the region labels / the slot map of window bw - parts (the prefetch rotation not made)
      mask_inf              the mask is -inf instead of -100
      no_max                exp(S) without the running maximum: inf above the fp32 overflow point
      pad_kv_zero / pad_q_unscaled   pad-slot k, v are 0 / pad-slot q is the bias without the scale
      dbias_last_round      the bias gradient misses the windows of the last round
      pad_query_dout        pad-slot queries read dO of token 0 instead of 0: their dS enters the bias gradient (and dK, dV)
      dpad_part             the pad-row sums miss the windows of the last part
      index_stride          the table gradient reads the full [ws^2, ws^2] index with row stride N
      lse_no_max            lse = log Z without the maximum
      pad_keys_kept         the NK - N padded key columns keep score 0 (their v is 0) instead of -1e30
      bias_transposed       bias[key, q] for bias[q, key]
    images: only the windows of these images (the per-slot outputs of a mutant; the sums over windows are then partial)"""
    g, x = geometry(case), inputs(case, dt)
    nB, nH, hd = case["nB"], case["nH"], case["hd"]
    N, nW, L, NK = g["N"], g["nW"], g["L"], g["NK"]
    C, Bw, scale = nH * hd, nB * nW, x["scale"]
    eq, ep, eo, twice = _eps(dt)
    wk = walk(case)["bwd"]
    parts = wk[0] if parts is None else parts
    iters = -(-Bw // parts)
    index = g["index"][:N, :N]
    bias = x["table"].double()[index.reshape(-1)].view(N, N, nH).permute(2, 0, 1)
    if mutant == "bias_transposed":
        bias = bias.transpose(1, 2)
    qkv = x["qkv"].double().view(nB * L, 3, nH, hd)
    dout = x["dout"].double().view(nB * L, nH, hd)
    qb = x["qb"].double().view(3, nH, hd)
    padrow = torch.stack([qb[0] * (1.0 if mutant == "pad_q_unscaled" else scale), qb[1] * (0.0 if mutant == "pad_kv_zero" else 1.0),
                          qb[2] * (0.0 if mutant == "pad_kv_zero" else 1.0)])  # [3, nH, hd]
    true_rows = (torch.arange(nB).view(nB, 1) * L + g["tok"].reshape(1, -1).clamp(min=0)).view(Bw, N)
    true_pad = (g["tok"] < 0).repeat(nB, 1)  # [Bw, N]
    res = {k: [] for k in ("attn", "lse", "out", "dq", "dk", "dv")}
    if want_bounds:
        for k in list(res):
            res["bd_" + k] = []
            if k != "attn":
                res["ab_" + k] = []
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    dbias, ab_dbias, e_dbias = z(nH, N, N), z(nH, N, N), z(nH, N, N)
    dpad, ab_dpad, e_dpad = z(2, nH, hd), z(2, nH, hd), z(2, nH, hd)
    step = max(1, (1 << 22) // (nW * nH * N * N))  # images per pass
    imgs = torch.arange(nB) if images is None else torch.as_tensor(sorted(images))
    for b0 in range(0, imgs.numel(), step):
        bw = (imgs[b0:b0 + step].view(-1, 1) * nW + torch.arange(nW).view(1, -1)).reshape(-1)
        B = bw.numel()
        lag = torch.where(bw >= parts, (bw - parts) % nW, bw % nW)
        tok = g["tok"][lag if mutant == "prev_map" else bw % nW]  # [B, N]
        pad = tok < 0
        rows = (bw // nW).view(B, 1) * L + tok.clamp(min=0)
        X = qkv[rows]  # [B, N, 3, nH, hd]
        X[:, :, 0] *= scale
        X[pad] = padrow
        q, k, v = (X[:, :, i].permute(0, 2, 1, 3) for i in range(3))  # [B, nH, N, hd]
        do = dout[rows]
        if mutant != "pad_query_dout":
            do[pad] = 0.0
        do = do.permute(0, 2, 1, 3)
        S0 = q @ k.transpose(-1, -2)
        S = S0 + bias
        mask = None
        if g["reg"] is not None:
            ids_ = g["reg"][lag if mutant == "prev_mask" else bw % nW]
            mask = torch.where(ids_[:, :, None] != ids_[:, None, :], float("-inf") if mutant == "mask_inf" else -100.0, 0.0).view(B, 1, N, N)
            S = S + mask
        m = S.max(-1, keepdim=True).values
        xs = S - m
        e = torch.exp(xs)
        if mutant == "no_max":
            e = torch.where(S > EXP_OVERFLOW, torch.full_like(e, float("inf")), e)
        Z = e.sum(-1, keepdim=True)
        if mutant == "pad_keys_kept":
            Z = Z + (NK - N) * torch.exp(-m)
        P = e / Z
        lse = (0.0 if mutant == "lse_no_max" else m) + torch.log(Z)
        O = P @ v
        dV = P.transpose(-1, -2) @ do
        dP = do @ v.transpose(-1, -2)
        delta = (P * dP).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        dQ = scale * (dS @ k)
        dK = dS.transpose(-1, -2) @ q
        outs = dict(attn=P, lse=lse.squeeze(-1), out=O, dq=dQ, dk=dK, dv=dV)
        if want_bounds:
            aq, ak, av, ado = q.abs(), k.abs(), v.abs(), do.abs()
            aqk = aq @ ak.transpose(-1, -2)
            ab_S = aqk + bias.abs() + (mask.abs() if mask is not None else 0.0)
            t = eq * aqk + (hd + 2) * U * ab_S + (3 * xs.abs() + 2) * U
            Ebar = (P * t).sum(-1, keepdim=True)
            r = t + Ebar + (NK + 3) * U
            rP = P * (r + ep)
            ab_O, ab_dV, ab_dP = P @ av, P.transpose(-1, -2) @ ado, ado @ av.transpose(-1, -2)
            bd_O = rP @ av + (NK + 1) * U * ab_O + eo * O.abs()
            e_dP = (hd + 1) * U * ab_dP
            e_delta = torch.maximum((rP * dP.abs() + P * e_dP).sum(-1, keepdim=True) + (NK + 1) * U * (P * dP.abs()).sum(-1, keepdim=True),
                                    (ado * bd_O).sum(-1, keepdim=True) + (hd + 1) * U * (ado * O.abs()).sum(-1, keepdim=True))
            e_dS = rP * (dP - delta).abs() + P * (e_dP + e_delta) + 2 * U * P * (dP.abs() + delta.abs())
            e_dSr = e_dS + ep * dS.abs()
            ab_dS = P * (dP.abs() + delta.abs())  # dS = P dP - P delta: where one key holds the row the two cancel
            ab_dQ, ab_dK = scale * (ab_dS @ ak), ab_dS.transpose(-1, -2) @ aq
            outs.update(
                bd_attn=P * r, bd_lse=(Ebar + (NK + 2) * U + 3 * U * (m.abs() + torch.log(Z).abs())).squeeze(-1), bd_out=bd_O, ab_out=ab_O,
                ab_lse=(m.abs() + torch.log(Z).abs()).squeeze(-1),
                bd_dv=rP.transpose(-1, -2) @ ado + (NK + 1) * U * ab_dV + eo * dV.abs(), ab_dv=ab_dV,
                bd_dq=scale * (e_dSr @ ak) + (NK + 2) * U * ab_dQ + eo * dQ.abs(), ab_dq=ab_dQ,
                bd_dk=e_dSr.transpose(-1, -2) @ aq + (eq + (NK + 1) * U) * ab_dK + eo * dK.abs(), ab_dk=ab_dK)
        if mutant == "prev_map":  # the results land on the tokens of the wrong map; read them back through the true one (unwritten: 0)
            flat, sel = rows.reshape(-1), ~pad.reshape(-1)
            for kk in ("out", "dq", "dk", "dv"):
                buf = torch.zeros(nB * L, nH, hd, dtype=torch.float64)
                buf[flat[sel]] = outs[kk].permute(0, 2, 1, 3).reshape(-1, nH, hd)[sel]
                outs[kk] = (buf[true_rows[bw]] * (~true_pad[bw]).view(B, N, 1, 1)).permute(0, 2, 1, 3)
        live = (bw < (iters - 1) * parts) if mutant == "dbias_last_round" else torch.ones(B, dtype=torch.bool)
        wsel = live.view(B, 1, 1, 1).double()
        dbias += (dS * wsel).sum(0)
        psel = (pad & ((bw % parts != parts - 1) if mutant == "dpad_part" else torch.ones(B, dtype=torch.bool)).view(B, 1)).view(B, 1, N, 1).double()
        dpad += torch.stack([(dK * psel).sum((0, 2)), (dV * psel).sum((0, 2))])
        if want_bounds:
            ab_dbias += (ab_dS * wsel).sum(0)
            e_dbias += e_dS.sum(0)
            ab_dpad += torch.stack([(ab_dK * psel).sum((0, 2)), (ab_dV * psel).sum((0, 2))])
            e_dpad += torch.stack([(outs["bd_dk"] * psel).sum((0, 2)), (outs["bd_dv"] * psel).sum((0, 2))])
        else:
            outs = {kk: vv for kk, vv in outs.items() if kk in res}
        if not mutant:  # pad slots of the per-slot outputs read 0 in window order (to_win)
            keep = (~pad).view(B, 1, N, 1).double()
            for kk in outs:
                if kk.split("_")[-1] in ("out", "dq", "dk", "dv"):
                    outs[kk] = outs[kk] * keep
        elif mutant != "prev_map":
            keep = (~true_pad[bw]).view(B, 1, N, 1).double()
            for kk in ("out", "dq", "dk", "dv"):
                outs[kk] = outs[kk] * keep
        for kk, vv in outs.items():
            res[kk].append(vv)
    res = {kk: torch.cat(vv) for kk, vv in res.items()}

    def scatter(dense, idx):
        return torch.zeros(g["trows"], nH, dtype=torch.float64).index_add_(0, idx, dense.permute(1, 2, 0).reshape(N * N, nH))
    idx = index.reshape(-1)
    if mutant == "index_stride":
        idx = g["index"].reshape(-1)[torch.arange(N).view(N, 1) * N + torch.arange(N).view(1, N)].reshape(-1)
    res.update(dbias=dbias, dtable=scatter(dbias, idx), dpad=dpad.reshape(2 * C), live=~true_pad)
    if g["reg"] is not None:
        res["masked"] = g["reg"][:, :, None] != g["reg"][:, None, :]
    if want_bounds:
        n_pad = int(true_pad.sum())
        bd_dbias = e_dbias + (iters + parts + 9) * U * ab_dbias
        res.update(ab_dbias=ab_dbias, bd_dbias=bd_dbias, ab_dtable=scatter(ab_dbias, idx), bd_dtable=scatter(bd_dbias, idx) + N * U * scatter(ab_dbias, idx),
                   ab_dpad=ab_dpad.reshape(2 * C), bd_dpad=(e_dpad + n_pad * U * ab_dpad).reshape(2 * C))
        for kk in OUTPUTS:
            res["bd_" + kk] = twice * res["bd_" + kk] + FLOOR
    return res


# ---- the fp32 restatement's error (the device's __expf) and the final bounds -------------------------------------------------------
def _block_max(err, block_dims):
    return err.amax(block_dims, keepdim=True).expand_as(err) if err.numel() else err


BLOCKS = dict(attn=(2, 3), lse=(2,), out=(2, 3), dq=(2, 3), dk=(2, 3), dv=(2, 3), dbias=(1, 2), dtable=(0,), dpad=(0,))


@functools.lru_cache(maxsize=None)
def _reference(name, dt):
    from oracle import ops_ref
    case = BY_NAME[name]
    ref = statement(case, dt)
    old = ops_ref.act_dtype()
    ops_ref.set_act_dtype(torch.float32)
    try:
        got = run_attention(ops_ref, torch.device("cpu"), case, dt, cast=torch.float32)
    finally:
        ops_ref.set_act_dtype(old)
    hd, nH = case["hd"], case["nH"]
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        err = (got[k] - ref[k]).abs()
        if k == "dpad":
            allow = 3 * err.view(2, nH, hd).amax(2, keepdim=True).expand(2, nH, hd).reshape(-1)
        else:
            allow = 3 * _block_max(err, BLOCKS[k])
        ref["bd_" + k] = torch.maximum(ref["bd_" + k], allow)
    return ref


def reference(case, dt):
    """the statement with its final bounds, once per process"""
    return _reference(case["name"], dt)


# ---- running a library (esvit_amd.ops on the device, oracle.ops_ref on the CPU) ---------------------------------------------------------------
SENTINEL = -7.0e4  # bf16- and fp32-representable; survives around every output
GUARD = 3  # rows


def _guarded(rows, cols, dt, dev):
    buf = torch.full((rows + 2 * GUARD, cols), SENTINEL, dtype=dt, device=dev)
    return buf, buf[GUARD:GUARD + rows]


def _moat_ok(buf):
    return float(bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()))


def run_attention(o, dev, case, dt, cast=None, want_attn=True, ws_flags=0, want_dbias=True, repeat=False):
    """forward (probability or training variant), backward on the forward's own output and lse, table gradient -> dict of fp64 CPU
    tensors in the statement's layout (None where the library gives none), with `moat` (sentinels intact), `repeat` (a second launch gave
    the same bits), `written` (slabs and pad rows written in full) and `parts`.  cast: the dtype the inputs are handed over in (the fp32 restatement takes bf16-valued fp32)"""
    g, x = geometry(case), inputs(case, dt)
    nH, hd, nB = case["nH"], case["hd"], case["nB"]
    N, nW, L, ws = g["N"], g["nW"], g["L"], g["ws"]
    C, rows, Bw = nH * hd, nB * L, nB * nW
    adt = cast or dt
    qkv, dout = x["qkv"].to(adt).to(dev), x["dout"].to(adt).to(dev)
    qb, table = x["qb"].to(dev), x["table"].to(dev)
    w2t = g["tok"].reshape(-1).to(torch.int32).to(dev)
    reg = g["reg"].reshape(-1).to(torch.int32).to(dev) if g["reg"] is not None else None
    index = g["index"].to(dev)
    device_lib = hasattr(o, "query")
    parts = o.query(o.Q_ATTN_BWD_PARTS, N, Bw, nH) if device_lib else 1
    frag = o.attn_frag_elems(N)

    def once():
        obuf, out = _guarded(rows, C, adt, dev)
        fwd = o.window_attn_fwd(qkv, qb, w2t, L, table, ws, reg, nW, N, nH, x["scale"], want_attn=want_attn, out=out)
        lse, attn = fwd[1], (fwd[2] if want_attn else None)
        gbuf, dq_out = _guarded(rows, 3 * C, adt, dev)
        kw = {}
        sbuf = None
        if want_dbias:
            sbuf = torch.full((parts + 2, nH, frag), SENTINEL, dtype=torch.float32, device=dev)
            kw["dbias_out"] = sbuf[1:parts + 1]
        if device_lib:
            if not want_dbias:
                kw["want_dbias"] = False
            # what torch.empty hands out next for the pad-row slab is poisoned: the <= 64-token kernel must write all of it
            prows = o.query(o.Q_ATTN_BWD_PAD_ROWS, N, Bw, nH | (({torch.float32: 0, torch.bfloat16: 1}[adt]) << 32))
            junk = torch.full((prows, 2 * C), float("nan"), dtype=torch.float32, device=dev)
            del junk
        dqkv, slabs, pad = o.window_attn_bwd(qkv, qb, w2t, L, dout, out, lse, table, ws | ws_flags, reg, nW, N, nH, x["scale"], dqkv_out=dq_out, **kw)
        dtable = o.relpos_bias_bwd(slabs, index, N, g["trows"]) if want_dbias else None
        moat = _moat_ok(obuf) * _moat_ok(gbuf)
        if sbuf is not None:
            moat *= float(bool((sbuf[0] == SENTINEL).all()) and bool((sbuf[-1] == SENTINEL).all()))
        return dict(out=out, lse=lse, attn=attn, dqkv=dqkv, slabs=slabs, pad=pad, dtable=dtable), moat

    raw, moat = once()
    res = dict(moat=moat, parts=parts, repeat=1.0)
    if repeat:  # (the table gradient is a scatter with atomics: its order of additions is free)
        again, moat2 = once()
        res["moat"] *= moat2
        res["repeat"] = float(all(torch.equal(raw[k], again[k]) for k in ("out", "lse", "attn", "dqkv", "slabs", "pad") if raw[k] is not None))
    res["out"] = to_win(raw["out"], case)
    d3 = to_win(raw["dqkv"], case, parts=3)
    res.update(dq=d3[0], dk=d3[1], dv=d3[2])
    res["attn"] = raw["attn"].detach().cpu().double().view(Bw, nH, N, N) if raw["attn"] is not None else None
    res["lse"] = raw["lse"].detach().cpu().double().view(Bw, nH, -1)[:, :, :N] if raw["lse"] is not None else None
    res["dtable"] = raw["dtable"].detach().cpu().double() if raw["dtable"] is not None else None
    res["dpad"] = raw["pad"].detach().cpu().double().sum(0)
    # written in full: no sentinel left in the caller's slab slice, no NaN of the poisoned allocation left in the pad-row slab
    res["written"] = float(raw["slabs"] is None or bool(torch.isfinite(raw["slabs"]).all() and (raw["slabs"] != SENTINEL).all())) * float(
        bool(torch.isfinite(raw["pad"]).all()))
    return res


def ratio(got, ref, bound, where=None):
    """max |got - ref| / bound over the elements (`where`: a mask of the elements that count); a non-finite value counts as inf"""
    if where is not None:
        got, ref, bound = got[where], ref[where], bound[where]
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bound).max()) if got.numel() else 0.0


def metrics(case, dt, got, training=False):
    """err / bound of every output the run has.  lse counts on the live queries (the training variant of the 224-slot forward leaves a
    placeholder in query tiles without a live token); attn on every query of the window"""
    ref = reference(case, dt)
    m = {}
    for k in OUTPUTS:
        if k == "dbias" or got.get(k) is None:
            continue
        where = ref["live"].view(ref["live"].shape[0], 1, -1).expand_as(ref["lse"]) if k == "lse" else None
        m["ratio_" + k] = ratio(got[k], ref[k], ref["bd_" + k], where)
    if bool(ref["live"].all()):  # no pad slot: the sums are exactly 0
        m["equal_dpad_zero"] = float(bool((got["dpad"] == 0).all()))
    for k in ("moat", "repeat", "written"):
        if k in got:
            m["equal_" + k] = got[k]
    return m


def failures(m):
    return ["%s = %.4g" % (k, v) for k, v in m.items() if (k.startswith("equal") and v != 1.0) or (k.startswith("ratio") and not v <= 1.0)]


def check(entry, case, dt, m, record=None, where="cpu", limit=1.0):
    """print (and record) every figure, then assert"""
    tag = dict(test="window_attn", entry=entry, case=case["name"], dtype=dt_name(dt), where=where)
    if record is not None:
        record(**tag, **m)
    print("OBSERVED", tag, m)
    bad = failures(m) + ["%s = %.4g > %.2g" % (k, v, limit) for k, v in m.items() if k.startswith("ratio") and limit < 1.0 and v > limit]
    assert not bad, (entry, case["name"], tag["dtype"], bad)
