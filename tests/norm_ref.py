"""fp64 statement of the row-normalisation kernels (esvit_amd/csrc/norm.hip behind ops.layernorm_fwd / layernorm_bwd / layernorm_bwd_cast /
layernorm_bwd_to_act / merge_ln_fwd / merge_ln_bwd / l2norm_fwd / l2norm_bwd / weightnorm_fwd / weightnorm_bwd) that
tests/test_norm_{cpu,gpu}.py compare against, the case table both share, the bounds, a host restatement of ln_cfg / ln_dispatch /
ln_bwd_nblk / row_iters_dispatch, and a plain fp32 emulation that reduces in the kernels' order (with the mutants the CPU test needs).
The statement is plain torch in float64 and calls nothing of oracle/ops_ref.py (the restatement enters only as the allowance for the
device's rsqrtf and division, below, and as one of the libraries run() drives).  Inputs are made in the case's dtype and promoted, so
bf16 inputs are exact in the reference.  The backward kernels take mean / rstd / z / inv_norm as fp32 tensors: the statement's own
values rounded to fp32, which the reference promotes again, so each backward is judged on its own.  Every output comes with `ab_*`, the
same expression with every term replaced by its absolute value, and `bd_*`, its bound.

Bounds (u = 2^-24, b = 2^-9; g(n) = n u / (1 - n u); per element, none is tuned, none is read from a file).  A row reduction of the
LayerNorm kernels is hsum4 (two additions deep), ITERS sequential additions, log2 G shuffle steps: ns = 2 + ITERS + log2 G roundings on
every term.  The L2 / weight_norm kernels reduce over a whole wave: nw = 2 + ITERS + 6.
  LayerNorm forward (ln_fwd_kernel)
    `mu = s / C`                      e_mu = g(ns + 2) mean|x|                                   (the division counted twice: not correctly rounded)
    `d = v[it] - mu`                  e_d  = e_mu + u (|d| + e_mu)                               (the variance is formed from x - mu-hat)
    `q += hsum4(d * d)`, `q / C`      e_var = mean(2 |d| e_d + e_d^2) + g(ns + 3) mean((|d| + e_d)^2)
    `rsqrtf(q / C + eps)`             t = var + eps, e_t = e_var + u (t + e_var);  e_rs = (t - e_t)^-1/2 - t^-1/2 + 2 u (rstd + ...)
                                      -- grows with |mean| / std through e_d = O(u |mean|), never with (mean / std)^2
    `(v[it] - mu) * rs * gm + bt`     A = (|d| + e_d)(rstd + e_rs);  e_y = |gamma| (A - |d| rstd + g(2) A) + u (|gamma| A + |beta|)
    a constant row has d = 0, var = 0: rstd is held to eps^-1/2 within e_rs, y to beta within |gamma| e_d (rstd + e_rs) (1 + ...)
    `store4<bf16>`                    bf16 y: 2 (e_y + b |y|);  y_f32 keeps e_y;  pad rows of the row-mapped y: exactly 0 (the floor)
  LayerNorm backward (ln_bwd_kernel; mean, rstd given)
    `xh = (xv - mu) * rs`             2 roundings;  `gd = d * gm` 1
    `s1 = group_sum(s1) / C`          e_s1 = g(ns + 3) ab_s1, ab_s1 = mean|gd|
    `s2 = group_sum(s2) / C`          e_s2 = g(ns + 6) ab_s2, ab_s2 = mean|gd xh|                (gd 1, xh 2, the product 1, the division 2)
    `o = (gd - s1 - xh * s2) * rs`    ab_dx = rstd (|gd| + ab_s1 + |xh| ab_s2) + |g_in|;  bd_dx = rstd (e_s1 + |xh| e_s2) + g(7) ab_dx
                                      (at most 6 roundings on a term: xh 2, the product, two subtractions, the scale; `o += g_in` 1)
    `store4<TA>(dx_act + off, o * sc)`  |sc| bd_dx + u |sc dx|;  bf16: 2 (|sc| bd_dx + (u + b) |sc dx|);  sc = 0 gives exactly 0
    `dgam[it] += d * xh[it]`          a lane group adds `trips` rows, `s += sm[g2 ...]` folds RPB groups, partial_reduce_kernel adds
    `dbet[it] += d`                   ceil(ceil(nblk / SLICES) / 4) partial rows in four chains, the chains (2), then SLICES slices (32 from
                                      256 blocks, else 8): ng = trips + RPB + ceil(ceil(nblk / SLICES) / 4) + 2 + SLICES
                                      bd_dgamma = g(ng + 3) sum_rows |dy xh|,  bd_dbeta = g(ng) sum_rows |dy|  (both scale with the rows)
    `out[c] + t` (accumulate)         the bounds of the two calls add, + u (|first| + |second|)
  Merge LayerNorm: the same kernels on the gathered row [x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)] of 4 Cin channels
  L2 normalise (l2norm_fwd_kernel / l2norm_bwd_kernel)
    `q += hsum4(v * v)`, `sqrtf(q)`   e_n = n (g(nw + 1) / 2 + u) + sqrt(D) 2^-63                (squares below 2^-126 may flush)
    `1.f / fmaxf(sqrtf(q), 1e-12f)`   e_inv = [n + e_n >= 1e-12] e_n / (max(n, c) max(n - e_n, c)) + 3 u inv   (both sides clamped: exact)
    `v[it] * inv`                     e_z = |x| e_inv + u |z|;  bf16: 2 (e_z + b |z|);  a zero row gives exactly 0
    `(g - zz * dot) * inv`            e_dot = g(nw + 1) ab_dot;  ab_dx = inv (|g| + |z| ab_dot);  bd_dx = inv |z| e_dot + g(3) ab_dx (+ b |dx|, doubled)
  weight_norm (weightnorm_fwd_kernel / weightnorm_bwd_kernel)
    `inv = 1.f / sqrtf(q)`            e_inv = inv (g(nw + 1) / 2 + 3 u);  `sc = g[k] * inv`, `x[it] * sc`: bd_w = |v g| e_inv + g(2) |w| (+ b |w|, doubled)
    `vh = v * inv`, `dot`             e_dot = g(nw + 2) ab_dot = bd_dg;  ab_dv = |sc| (|dw| + |vh| ab_dot);  bd_dv = |sc vh| e_dot + g(5) ab_dv
  Every bound carries the floor 2^-100.
  Device rsqrtf and division are not correctly rounded and their error cannot be derived here, so every bound is the larger of the
  derived one and 3 x the error of the fp32 restatement (oracle/ops_ref on the CPU, same inputs, fp32 activations), that error taken as
  its maximum over the same row (per element for the per-row statistics and for dgamma / dbeta).

Case -> instantiation (ln_fwd_kernel / ln_bwd_kernel <T, G, ITERS>, T = float and bf16; WIDTHS below is the table the tests hold to
ln_cfg and to ops.query(Q_LN_BWD_BLOCKS)):
  ln_w4_*, ln_w48_*, ln_w64_*   <16,1>  (1 / 12 / 16 of 16 lanes)        ln_w96_*, ln_var_*_w96, ln_map_*, ln_num_*_w96_*, ln_pass_w96    <8,3>
  ln_w128_*, ln_pass_w128       <32,1>                                   ln_w160_*                                                        <64,1>  (40 of 64 lanes)
  ln_w192_*                     <16,3>                                   ln_w256_*, ln_pass_w256                                          <16,4>
  ln_w320_*, ln_w512_*, ln_var_*_w512, merge_2x4x6x128   <64,2>           ln_w384_*, merge_1x2x2x96, merge_3x6x10x96                       <32,3>
  ln_w576_*, ln_w768_*, ln_pass_w768   <64,3>                            ln_w1024_*, ln_num_*_w1024_*, merge_1x4x2x256                    <64,4>
  ln_w1280_*, ln_w1536_*        <64,6>  (LDS of the backward 40 / 48 KiB)   ln_w1792_*, ln_w2048_*, merge_1x2x4x512                        <64,8>  (56 / 64 KiB: hipFuncSetAttribute)
  ln_var_toact_*: ln_bwd_kernel<float, G, ITERS, float | bf16> with dx = NULL.  *_r1: one row; otherwise 2 RPB + 1 rows (a ragged last
  block); ln_pass_*: more than 1024 RPB rows, so that 1024 blocks walk the grid-stride loop twice for some lane groups and once for others.
  l2_d{4,256} / wn_d{4,256}: row ITERS 1;  d{260,384}: 2;  d{768,1024}: 4;  d{1028,2048}: 8   (l2norm_*_kernel<T, ITERS>, weightnorm_fwd_kernel<T, ITERS>,
  weightnorm_bwd_kernel<ITERS>; the backward of weight_norm is fp32 only)
"""
import functools
import math
import zlib

import torch

from tests.window_attn_ref import window_geometry

U = 2.0 ** -24
BF = 2.0 ** -9
FLOOR = 2.0 ** -100
L2_CLAMP = 1e-12
DTYPES = (torch.float32, torch.bfloat16)
SENTINEL = -7.0e4  # bf16- and fp32-representable
LN_THREADS = 256


def dt_name(dt):
    return {torch.float32: "fp32", torch.bfloat16: "bf16"}[dt]


def g(n):
    return n * U / (1.0 - n * U)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()) % (2 ** 31))


def data(key, shape, dt=torch.float32, scale=1.0, shift=0.0):
    """seeded values stored as dt (on the CPU)"""
    return (torch.randn(*shape, generator=_gen(*key)) * scale + shift).to(dt)


def _f32(v):
    """a Python float as the kernel receives it"""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- the host code of norm.hip, restated --------------------------------------------------------------------------------------------
LN_INSTANCES = ((8, 3), (16, 3), (16, 4), (16, 1), (32, 3), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4), (64, 6), (64, 8))


def ln_cfg(C):
    """ln_cfg: (G, ITERS) for width C, or None where the library refuses"""
    if C <= 0 or C % 4:
        return None
    C4 = C // 4
    if C4 % 3 == 0 and C4 // 3 in (8, 16, 32, 64):
        return (C4 // 3, 3)
    if C4 == 64:
        return (16, 4)
    G = 16 if C4 <= 16 else (32 if C4 <= 32 else 64)
    it = -(-C4 // G)
    for a in (1, 2, 3, 4, 6, 8):
        if it <= a:
            return (G, a)
    return None


def ln_dispatch(G, it):
    """ln_dispatch: the <G, ITERS> instantiation launched for a configuration (its else-chain, in its order)"""
    if G == 8:
        return (8, 3)
    if G == 16:
        return (16, it if it in (3, 4) else 1)
    if G == 32:
        return (32, 3 if it == 3 else 1)
    return (64, it if it in (1, 2, 3, 4, 6) else 8)


def ln_shape(C):
    """(G, ITERS, RPB = rows per 256-thread block) of the instantiation launched for width C"""
    G, it = ln_dispatch(*ln_cfg(C))
    return G, it, LN_THREADS // G


def ln_bwd_blocks(rows, C):
    """ln_bwd_nblk"""
    if ln_cfg(C) is None:
        return 0
    rpb = ln_shape(C)[2]
    return max(1, min(1024, -(-rows // rpb)))


def row_iters(D):
    """row_iters_dispatch"""
    d4 = D // 4
    return 1 if d4 <= 64 else (2 if d4 <= 128 else (4 if d4 <= 256 else 8))


def fold_depth(rows, C, accumulate=False):
    """ng: roundings on one term of dgamma / dbeta on its way through the row loop, the LDS fold and partial_reduce_kernel"""
    rpb, nblk = ln_shape(C)[2], ln_bwd_blocks(rows, C)
    trips = -(-rows // (nblk * rpb))
    slices = 32 if nblk >= 256 else 8
    return trips + rpb + -(-(-(-nblk // slices)) // 4) + 2 + slices + (1 if accumulate else 0)


# ---- the case table -------------------------------------------------------------------------------------------------------------------
# width, instantiation, why it is there
WIDTHS = [(4, (16, 1), "1 of 16 lanes"), (48, (16, 1), "12 of 16 lanes"), (64, (16, 1), "CvT"), (96, (8, 3), ""), (128, (32, 1), ""),
          (160, (64, 1), "40 of 64 lanes"), (192, (16, 3), ""), (256, (16, 4), ""), (320, (64, 2), "second iteration 16 of 64 lanes"),
          (384, (32, 3), ""), (512, (64, 2), ""), (576, (64, 3), "third iteration 16 lanes"), (768, (64, 3), ""), (1024, (64, 4), ""),
          (1280, (64, 6), "last iteration idle"), (1536, (64, 6), "LDS exactly 48 KiB"), (1792, (64, 8), "it = 7 of 8; LDS above 48 KiB"),
          (2048, (64, 8), "")]
MULTI_PASS = [(96, 32768 + 37), (256, 16384 + 19), (128, 8192 + 11), (768, 4096 + 5)]  # one per lane-group width: G 8, 16, 32, 64
VARIANT_WIDTHS = (96, 512)
NUMERIC_WIDTHS = (96, 1024)
ROW_MAPS = [(6, 7, 3), (14, 7, 0)]  # (H, ws, shift), 2 samples; the first has pads
MERGES = [(1, 2, 2, 96), (3, 6, 10, 96), (2, 4, 6, 128), (1, 4, 2, 256), (1, 2, 4, 512)]  # (nB, H, W, Cin)
ROW_WIDTHS = (4, 256, 260, 384, 768, 1024, 1028, 2048)  # L2 / weight_norm; 260 and 1028: one lane in the last iteration
ROW_COUNTS = (1, 5, 9)  # 4 rows per block: 1, 4 + 1, 4 * 2 + 1
REFUSED_LN = (98, 2052)
REFUSED_ROW = (2052, 6)


def _ln(name, C, rows, **kw):
    c = dict(kind="ln", name=name, C=C, rows=rows, eps=1e-6, fill="normal", want_f32=False, g_in=False, bwd="plain", rowscale=None, gb=None,
             map=None, dts=DTYPES)
    c.update(kw)
    return c


def _two_blocks(C):
    return 2 * ln_shape(C)[2] + 1


def _build_cases():
    cs = []
    for C, _, _ in WIDTHS:
        cs.append(_ln("ln_w%d_r1" % C, C, 1))
        cs.append(_ln("ln_w%d_r%d" % (C, _two_blocks(C)), C, _two_blocks(C)))
    for C, rows in MULTI_PASS:
        cs.append(_ln("ln_pass_w%d" % C, C, rows))
    for C in VARIANT_WIDTHS:
        r = _two_blocks(C)
        cs += [_ln("ln_var_f32_w%d" % C, C, r, want_f32=True),
               _ln("ln_var_gin_w%d" % C, C, r, g_in=True),
               _ln("ln_var_act_w%d" % C, C, r, g_in=True, bwd="cast"),
               _ln("ln_var_act_rs1_w%d" % C, C, r, g_in=True, bwd="cast", rowscale=1),  # samples of 1 row, a factor 0 among them
               _ln("ln_var_act_rs%d_w%d" % (3 if C == 512 else 5, C), C, r, g_in=True, bwd="cast", rowscale=3 if C == 512 else 5),
               _ln("ln_var_toact_w%d" % C, C, r, bwd="to_act"),
               _ln("ln_var_gb_adjacent_w%d" % C, C, r, gb="adjacent"),
               _ln("ln_var_gb_separate_w%d" % C, C, r, gb="separate")]
    for H, ws, shift in ROW_MAPS:
        cs.append(_ln("ln_map_h%d_s%d" % (H, shift), 96, 2 * H * H, map=(H, ws, shift, 2)))
    for C in NUMERIC_WIDTHS:
        for eps in (1e-6, 1e-5):
            for fill in ("mean1000", "mean300", "const", "scales"):
                cs.append(_ln("ln_num_%s_w%d_e%d" % (fill, C, round(-math.log10(eps))), C, _two_blocks(C), eps=eps, fill=fill))
    for nB, H, W, Cin in MERGES:
        cs.append(dict(kind="merge", name="merge_%dx%dx%dx%d" % (nB, H, W, Cin), nB=nB, H=H, W=W, Cin=Cin, C=4 * Cin, rows=nB * (H // 2) * (W // 2),
                       eps=1e-6, dts=DTYPES))
    for D in ROW_WIDTHS:
        for R in ROW_COUNTS:
            cs.append(dict(kind="l2", name="l2_d%d_r%d" % (D, R), D=D, rows=R, edge=R == 9, dts=DTYPES))  # edge: a zero row and a row of norm 1e-20
            cs.append(dict(kind="wn", name="wn_d%d_k%d" % (D, R), D=D, rows=R, dts=DTYPES))
    return cs


CASES = _build_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def params(kinds=None):
    return [(c, dt) for c in CASES for dt in c["dts"] if kinds is None or c["kind"] in kinds]


def ids(ps):
    return ["%s-%s" % (c["name"], dt_name(dt)) for c, dt in ps]


# ---- geometry --------------------------------------------------------------------------------------------------------------------------
def merge_rows(nB, H, W, swap=False):
    """[nB H/2 W/2, 4] token row of every quadrant of a merged row, in the order (0,0) (1,0) (0,1) (1,1): quadrant q sits at
    (2 i + (q & 1), 2 j + (q >> 1)).  swap: the mutant with (1,0) and (0,1) exchanged"""
    Ho, Wo = H // 2, W // 2
    r = torch.arange(nB * Ho * Wo)
    b, i, j = r // (Ho * Wo), (r % (Ho * Wo)) // Wo, r % Wo
    q = torch.arange(4)
    di, dj = (q >> 1, q & 1) if swap else (q & 1, q >> 1)
    return (b[:, None] * H + 2 * i[:, None] + di[None, :]) * W + 2 * j[:, None] + dj[None, :]


@functools.lru_cache(maxsize=None)
def row_map(H, ws, shift):
    """(tok2win int64 [H H], slots per sample)"""
    tok = window_geometry(H, H, ws, shift)[0].reshape(-1)
    t2w = torch.empty(H * H, dtype=torch.int64)
    slots = torch.nonzero(tok >= 0).reshape(-1)
    t2w[tok[slots]] = slots
    return t2w, tok.numel()


def _map_rows(case):
    """mapped row of every row, rows of the mapped tensor; None without a map"""
    if case.get("map") is None:
        return None, case["rows"]
    H, ws, shift, nB = case["map"]
    t2w, period = row_map(H, ws, shift)
    r = torch.arange(case["rows"])
    return (r // (H * H)) * period + t2w[r % (H * H)], nB * period


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _ln_x(case):
    n, rows, C, fill = case["name"], case["rows"], case["C"], case["fill"]
    z = data((n, "x"), (rows, C))
    if fill == "normal":
        return z * 1.5 + data((n, "xm"), (rows, 1), scale=0.5)
    if fill == "mean1000":
        return 1000.0 + z
    if fill == "mean300":
        return -300.0 + 0.01 * z
    if fill == "const":
        return (data((n, "xc"), (rows, 1), scale=3.0)).expand(rows, C).contiguous()
    assert fill == "scales"
    return z * torch.where(torch.arange(rows) % 2 == 0, 1e-4, 1e4).view(rows, 1)


@functools.lru_cache(maxsize=4)
def _inputs(name, dt):
    c = BY_NAME[name]
    kind = c["kind"]
    if kind in ("ln", "merge"):
        C, rows = c["C"], c["rows"]
        if kind == "merge":
            x = data((name, "x"), (c["nB"], c["H"] * c["W"], c["Cin"])) * 1.5 + 0.3
            xg = x.view(-1, c["Cin"])[merge_rows(c["nB"], c["H"], c["W"])].reshape(rows, C)
            tokens = c["nB"] * c["H"] * c["W"]
            rs = data((name, "rs"), (tokens,)).abs() + 0.5
            rs[1] = 0.0
            extra = dict(dy2=data((name, "dy2"), (rows, C), dt), rowscale=rs, gb_prev=data((name, "gbp"), (2, C)))
            drows = rows
        else:
            x = xg = _ln_x(c)
            ri, drows = _map_rows(c)
            extra = dict(g_in=data((name, "gin"), (rows, C)), dy_f32=data((name, "dy32"), (rows, C)))
            if c["rowscale"]:
                rs = data((name, "rs"), (-(-rows // c["rowscale"]),)).abs() + 0.5
                rs[min(1, rs.numel() - 1)] = 0.0
                extra["rowscale"] = rs
        x64 = xg.double()
        mean = x64.mean(1)
        rstd = (((x64 - mean[:, None]) ** 2).mean(1) + _f32(c["eps"])) ** -0.5
        return dict(x=x, gamma=1.0 + data((name, "gamma"), (C,), scale=0.2), beta=data((name, "beta"), (C,), scale=0.1),
                    dy=data((name, "dy"), (drows, C), dt), mean=mean.float(), rstd=rstd.float(), **extra)
    D, R = c["D"], c["rows"]
    if kind == "l2":
        x = data((name, "x"), (R, D))
        if c["edge"]:
            x[3] = 0.0
            x[6] *= 1e-20 / float(x[6].double().norm())
        x = x.to(dt)
        n = x.double().norm(dim=1)
        inv = 1.0 / n.clamp(min=L2_CLAMP)
        return dict(x=x, dz=data((name, "dz"), (R, D), dt), z=(x.double() * inv[:, None]).to(dt), inv=inv.float())
    v = data((name, "v"), (R, D), scale=0.05)
    return dict(v=v, g=1.0 + data((name, "g"), (R, 1), scale=0.1), dw=data((name, "dw"), (R, D)), inv=(1.0 / v.double().norm(dim=1)).float())


def inputs(case, dt):
    """the case's tensors on the CPU: activations in dt, parameters / x / statistics fp32"""
    return _inputs(case["name"], dt)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def _store(e, val, dt):
    """bound of a value stored as dt, from the bound e of the fp32 value"""
    return 2.0 * (e + BF * val.abs()) + FLOOR if dt == torch.bfloat16 else e + FLOOR


def ln_forward(x, gamma, beta, eps, C, dt):
    """x [rows, C] fp64 (the gathered rows for merge) -> mean, rstd, y (= y_f32) with ab_ / bd_ (bd_y for a store in dt, bd_y_f32 fp32)"""
    G, it, _ = ln_shape(C)
    ns = 2 + it + int(math.log2(G))
    ga, be = gamma.abs(), beta.abs()
    mu = x.mean(1, keepdim=True)
    ab_mu = x.abs().mean(1, keepdim=True)
    e_mu = g(ns + 2) * ab_mu
    d = x - mu
    e_d = e_mu + U * (d.abs() + e_mu)
    var = (d * d).mean(1, keepdim=True)
    e_var = (2 * d.abs() * e_d + e_d ** 2).mean(1, keepdim=True) + g(ns + 3) * ((d.abs() + e_d) ** 2).mean(1, keepdim=True)
    t = var + eps
    e_t = e_var + U * (t + e_var)
    rstd = t ** -0.5
    e_rs = torch.where(e_t < t, (t - e_t).clamp(min=1e-300) ** -0.5 - rstd, torch.full_like(t, float("inf")))
    e_rs = e_rs + 2 * U * (rstd + e_rs)
    A = (d.abs() + e_d) * (rstd + e_rs)
    y = d * rstd * gamma + beta
    e_y = ga * ((A - d.abs() * rstd) + g(2) * A) + U * (ga * A + be)
    return dict(mean=mu[:, 0], ab_mean=ab_mu[:, 0], bd_mean=e_mu[:, 0] + FLOOR, rstd=rstd[:, 0], ab_rstd=rstd[:, 0], bd_rstd=e_rs[:, 0] + FLOOR,
                y=y, ab_y=d.abs() * rstd * ga + be, bd_y=_store(e_y, y, dt), bd_y_f32=e_y + FLOOR)


def ln_backward(x, d, mean, rstd, gamma, C, g_in=None, rows_total=None, accumulate=False):
    """the hand-written backward on rows x [rows, C] with upstream rows d (already read through the map), statistics as given -> dx (with
    g_in added), dgamma, dbeta with ab_ / bd_ (fp32 stores)"""
    G, it, _ = ln_shape(C)
    ns = 2 + it + int(math.log2(G))
    mu, rs = mean.view(-1, 1), rstd.view(-1, 1)
    xh = (x - mu) * rs
    gd = d * gamma
    s1, ab_s1 = gd.mean(1, keepdim=True), gd.abs().mean(1, keepdim=True)
    s2, ab_s2 = (gd * xh).mean(1, keepdim=True), (gd * xh).abs().mean(1, keepdim=True)
    dx = rs * (gd - s1 - xh * s2)
    ab_dx = rs.abs() * (gd.abs() + ab_s1 + xh.abs() * ab_s2)
    if g_in is not None:
        dx, ab_dx = dx + g_in, ab_dx + g_in.abs()
    bd_dx = rs.abs() * (g(ns + 3) * ab_s1 + xh.abs() * g(ns + 6) * ab_s2) + g(7) * ab_dx
    ng = fold_depth(x.shape[0] if rows_total is None else rows_total, C, accumulate)
    ab_dg, ab_db = (d * xh).abs().sum(0), d.abs().sum(0)
    return dict(dx=dx, ab_dx=ab_dx, bd_dx=bd_dx + FLOOR, dgamma=(d * xh).sum(0), ab_dgamma=ab_dg, bd_dgamma=g(ng + 3) * ab_dg + FLOOR,
                dbeta=d.sum(0), ab_dbeta=ab_db, bd_dbeta=g(ng) * ab_db + FLOOR)


def act_copy(dx, bd_dx, scale, dt):
    """dx_act = cast(scale dx) -> value, bound"""
    v = dx * scale
    e = scale.abs() * bd_dx + U * v.abs()
    return v, _store(e, v, dt)


def l2_forward(x, D, dt):
    nw = 2 + row_iters(D) + 6
    n = (x * x).sum(1).sqrt()
    e_n = n * (g(nw + 1) / 2 + U) + math.sqrt(D) * 2.0 ** -63
    c = L2_CLAMP
    inv = 1.0 / n.clamp(min=c)
    e_inv = torch.where(n + e_n >= c, e_n / (n.clamp(min=c) * (n - e_n).clamp(min=c)), torch.zeros_like(n)) + 3 * U * inv
    z = x * inv[:, None]
    e_z = x.abs() * e_inv[:, None] + U * z.abs()
    return dict(inv=inv, ab_inv=inv, bd_inv=e_inv + FLOOR, z=z, ab_z=z.abs(), bd_z=_store(e_z, z, dt))


def l2_backward(dz, z, inv, D, dt):
    nw = 2 + row_iters(D) + 6
    iv = inv.view(-1, 1)
    dot, ab_dot = (dz * z).sum(1, keepdim=True), (dz * z).abs().sum(1, keepdim=True)
    dx = (dz - z * dot) * iv
    ab_dx = iv.abs() * (dz.abs() + z.abs() * ab_dot)
    e = iv.abs() * z.abs() * g(nw + 1) * ab_dot + g(3) * ab_dx
    return dict(dx=dx, ab_dx=ab_dx, bd_dx=_store(e, dx, dt))


def wn_forward(v, gw, D, dt):
    nw = 2 + row_iters(D) + 6
    inv = 1.0 / (v * v).sum(1).sqrt()
    e_inv = inv * (g(nw + 1) / 2 + 3 * U)
    w = v * (gw.view(-1, 1) * inv[:, None])
    e_w = (v * gw.view(-1, 1)).abs() * e_inv[:, None] + g(2) * w.abs()
    return dict(inv=inv, ab_inv=inv, bd_inv=e_inv + FLOOR, w=w, ab_w=w.abs(), bd_w=_store(e_w, w, dt))


def wn_backward(dw, v, gw, inv, D):
    nw = 2 + row_iters(D) + 6
    iv = inv.view(-1, 1)
    vh = v * iv
    dot, ab_dot = (dw * vh).sum(1, keepdim=True), (dw * vh).abs().sum(1, keepdim=True)
    sc = gw.view(-1, 1) * iv
    dv = (dw - vh * dot) * sc
    ab_dv = sc.abs() * (dw.abs() + vh.abs() * ab_dot)
    e_dot = g(nw + 2) * ab_dot
    return dict(dv=dv, ab_dv=ab_dv, bd_dv=(sc * vh).abs() * e_dot + g(5) * ab_dv + FLOOR, dg=dot, ab_dg=ab_dot, bd_dg=e_dot + FLOOR)


def _put(res, src, keys, rename=None):
    for k in keys:
        for p in ("", "ab_", "bd_"):
            res[p + (rename or {}).get(k, k)] = src[p + k]


def statement(case, dt):
    """-> dict of fp64 tensors, the keys of run()'s outputs with their ab_ and bd_ companions"""
    x, kind, res = inputs(case, dt), case["kind"], {}
    f64 = lambda t: t.double()  # noqa: E731
    if kind == "ln":
        C, rows = case["C"], case["rows"]
        fw = ln_forward(f64(x["x"]), f64(x["gamma"]), f64(x["beta"]), _f32(case["eps"]), C, dt)
        _put(res, fw, ("mean", "rstd"))
        ri, drows = _map_rows(case)
        if ri is None:
            _put(res, fw, ("y",))
        else:  # the row-mapped store into a zero-initialised output: pad rows stay exactly 0
            for p, fill in (("", 0.0), ("ab_", 0.0), ("bd_", FLOOR)):
                buf = torch.full((drows, C), fill, dtype=torch.float64)
                buf[ri] = fw[p + "y"]
                res[p + "y"] = buf
        if case["want_f32"]:
            res.update(y_f32=fw["y"], ab_y_f32=fw["ab_y"], bd_y_f32=fw["bd_y_f32"])
        d = f64(x["dy_f32"] if case["bwd"] == "to_act" else x["dy"])
        if ri is not None:
            d = d[ri]
        bw = ln_backward(f64(x["x"]), d, f64(x["mean"]), f64(x["rstd"]), f64(x["gamma"]), C, g_in=f64(x["g_in"]) if case["g_in"] else None)
        _put(res, bw, ("dgamma", "dbeta"))
        if case["bwd"] != "to_act":
            _put(res, bw, ("dx",))
        if case["bwd"] in ("cast", "to_act"):
            sc = torch.ones(rows, 1, dtype=torch.float64)
            if case["rowscale"]:
                sc = f64(x["rowscale"])[torch.arange(rows) // case["rowscale"]].view(rows, 1)
            res["dx_act"], res["bd_dx_act"] = act_copy(bw["dx"], bw["bd_dx"], sc, dt)
            res["ab_dx_act"] = sc.abs() * bw["ab_dx"]
    elif kind == "merge":
        nB, H, W, Cin, C, rows = case["nB"], case["H"], case["W"], case["Cin"], case["C"], case["rows"]
        src = merge_rows(nB, H, W)
        xt = f64(x["x"]).view(-1, Cin)
        xg = xt[src].reshape(rows, C)
        fw = ln_forward(xg, f64(x["gamma"]), f64(x["beta"]), _f32(case["eps"]), C, dt)
        _put(res, fw, ("mean", "rstd", "y"))
        bw = ln_backward(xg, f64(x["dy"]), f64(x["mean"]), f64(x["rstd"]), f64(x["gamma"]), C)
        b2 = ln_backward(xg, f64(x["dy2"]), f64(x["mean"]), f64(x["rstd"]), f64(x["gamma"]), C, accumulate=True)
        _put(res, bw, ("dgamma", "dbeta"))
        for p in ("", "ab_", "bd_"):  # the scatter to the un-merged token rows: every token row is written once
            buf = torch.zeros(nB * H * W, Cin, dtype=torch.float64)
            buf[src.reshape(-1)] = bw[p + "dx"].reshape(rows * 4, Cin)
            res[p + "dx"] = buf
        one = torch.ones(nB * H * W, 1, dtype=torch.float64)
        res["act"], res["bd_act"] = act_copy(res["dx"], res["bd_dx"], one, dt)
        res["act_rs"], res["bd_act_rs"] = act_copy(res["dx"], res["bd_dx"], f64(x["rowscale"]).view(-1, 1), dt)
        res["ab_act"], res["ab_act_rs"] = res["ab_dx"], f64(x["rowscale"]).view(-1, 1) * res["ab_dx"]
        for k in ("dgamma", "dbeta"):  # the first call overwrites what gb_out held, the second adds: reference of first + reference of second
            res["acc_" + k] = bw[k] + b2[k]
            res["ab_acc_" + k] = bw["ab_" + k] + b2["ab_" + k]
            res["bd_acc_" + k] = bw["bd_" + k] + b2["bd_" + k] + U * (bw[k].abs() + b2[k].abs())
    elif kind == "l2":
        D = case["D"]
        _put(res, l2_forward(f64(x["x"]), D, dt), ("z", "inv"))
        _put(res, l2_backward(f64(x["dz"]), f64(x["z"]), f64(x["inv"]), D, dt), ("dx",))
    else:
        D = case["D"]
        _put(res, wn_forward(f64(x["v"]), f64(x["g"]), D, dt), ("w", "inv"))
        if dt == torch.float32:  # the backward is fp32 only
            _put(res, wn_backward(f64(x["dw"]), f64(x["v"]), f64(x["g"]), f64(x["inv"]), D), ("dv", "dg"))
            res["dg"], res["ab_dg"], res["bd_dg"] = (res[k].reshape(-1) for k in ("dg", "ab_dg", "bd_dg"))
    return res


def outputs(ref):
    return [k for k in ref if "bd_" + k in ref]


@functools.lru_cache(maxsize=4)
def _reference(name, dt):
    from oracle import ops_ref
    case = BY_NAME[name]
    ref = statement(case, dt)
    got = run(ops_ref, torch.device("cpu"), case, dt, cast=torch.float32)
    for k in outputs(ref):
        err = (got[k] - ref[k]).abs()
        err = torch.where(torch.isfinite(err), err, torch.zeros_like(err))
        if err.dim() == 2:
            err = err.amax(1, keepdim=True).expand_as(err)
        ref["bd_" + k] = torch.maximum(ref["bd_" + k], 3 * err)
    return ref


def reference(case, dt):
    """the statement with its final bounds (the larger of the derived bound and 3 x the restatement's error over the row)"""
    return _reference(case["name"], dt)


# ---- running a library (esvit_amd.ops on the device, oracle.ops_ref or Emulation on the CPU) -------------------------------------------
class _ActDtype:
    """layernorm_bwd_to_act writes the library's activation dtype"""

    def __init__(self, o, dt):
        self.o, self.dt = o, dt

    def __enter__(self):
        self.old = self.o.act_dtype()
        self.o.set_act_dtype(self.dt)

    def __exit__(self, *a):
        self.o.set_act_dtype(self.old)


def _moat(buf, rows):
    return float(all(bool((buf[r] == SENTINEL).all()) for r in rows))


def _run_ln(o, dev, case, dt, adt):
    x = {k: v.to(dev) for k, v in inputs(case, dt).items()}
    C, rows = case["C"], case["rows"]
    ri, drows = _map_rows(case)
    kw, bkw, flags = dict(dtype=adt, want_f32=case["want_f32"]), {}, {}
    if ri is not None:
        H, ws, shift, nB = case["map"]
        t2w, period = row_map(H, ws, shift)
        t2w = t2w.to(torch.int32).to(dev)
        kw.update(rowmap=t2w, period_out=period, out_rows=drows)
        bkw.update(rowmap=t2w, period_in=period)
    y, yf, mean, rstd = o.layernorm_fwd(x["x"], x["gamma"], x["beta"], case["eps"], **kw)
    out = dict(y=y, mean=mean, rstd=rstd)
    if ri is not None:
        pad = torch.ones(drows, dtype=torch.bool)
        pad[ri] = False
        flags["equal_pad_zero"] = float(bool((y[pad.to(dev)] == 0).all()))
    if case["want_f32"]:
        out["y_f32"] = yf
    gbuf = None
    if case["gb"]:
        gbuf = torch.full((5, C), SENTINEL, dtype=torch.float32, device=dev)
        bkw["gb_out"] = (gbuf[1], gbuf[2] if case["gb"] == "adjacent" else gbuf[3])
    dy = x["dy"].to(adt)
    gin = x["g_in"] if case["g_in"] else None
    if case["bwd"] == "plain":
        out["dx"], out["dgamma"], out["dbeta"] = o.layernorm_bwd(dy, x["x"], x["mean"], x["rstd"], x["gamma"], g_in=gin, **bkw)
    elif case["bwd"] == "cast":
        out["dx"], out["dx_act"], out["dgamma"], out["dbeta"] = o.layernorm_bwd_cast(
            dy, x["x"], x["mean"], x["rstd"], x["gamma"], g_in=gin, rowscale=x.get("rowscale"), rows_per_sample=case["rowscale"] or 0, **bkw)
    else:
        with _ActDtype(o, adt):
            out["dx_act"], out["dgamma"], out["dbeta"] = o.layernorm_bwd_to_act(x["dy_f32"], x["x"], x["mean"], x["rstd"], x["gamma"], **bkw)
    if gbuf is not None:
        flags["equal_moat"] = _moat(gbuf, (0, 4) + ((3,) if case["gb"] == "adjacent" else (2,)))
        flags["equal_gb_alias"] = float(out["dgamma"].data_ptr() == gbuf[1].data_ptr())
    return out, flags


def _run_merge(o, dev, case, dt, adt):
    x = {k: v.to(dev) for k, v in inputs(case, dt).items()}
    nB, H, W, Cin, C, rows = case["nB"], case["H"], case["W"], case["Cin"], case["C"], case["rows"]
    y, mean, rstd = o.merge_ln_fwd(x["x"], x["gamma"], x["beta"], case["eps"], H, W, dtype=adt)
    # the out= form: row slices of larger buffers take the bits of the plain call, the rows around them stay
    yb = torch.full((rows + 4, C), SENTINEL, dtype=adt, device=dev)
    sb = torch.full((2, rows + 4), SENTINEL, dtype=torch.float32, device=dev)
    got = o.merge_ln_fwd(x["x"], x["gamma"], x["beta"], case["eps"], H, W, dtype=adt, out=(yb[2:2 + rows], sb[0, 2:2 + rows], sb[1, 2:2 + rows]))
    flags = dict(equal_out_slice=float(torch.equal(yb[2:2 + rows], y) and torch.equal(sb[0, 2:2 + rows], mean) and torch.equal(sb[1, 2:2 + rows], rstd)
                                       and got[0].data_ptr() == yb[2].data_ptr()),
                 equal_moat=_moat(yb, (0, 1, rows + 2, rows + 3)) * float(bool((sb[:, :2] == SENTINEL).all() and (sb[:, rows + 2:] == SENTINEL).all())))
    out = dict(y=y, mean=mean, rstd=rstd)
    dy, dy2 = x["dy"].to(adt), x["dy2"].to(adt)
    st = (x["x"], x["mean"], x["rstd"], x["gamma"], H, W)
    dx, out["dgamma"], out["dbeta"] = o.merge_ln_bwd(dy, *st)
    out["dx"] = dx.reshape(-1, Cin)
    act = torch.full((nB * H * W + 2, Cin), SENTINEL, dtype=adt, device=dev)
    dxo = torch.full((nB * H * W + 2, Cin), SENTINEL, dtype=torch.float32, device=dev)
    o.merge_ln_bwd(dy, *st, dx_out=dxo[1:-1], act_out=act[1:-1])
    out["act"] = act[1:-1].clone()
    flags["equal_dx_out"] = float(torch.equal(dxo[1:-1], out["dx"]))
    o.merge_ln_bwd(dy, *st, dx_out=dxo[1:-1], act_out=act[1:-1], rowscale=x["rowscale"])
    out["act_rs"] = act[1:-1].clone()
    flags["equal_moat"] *= _moat(act, (0, -1)) * _moat(dxo, (0, -1))
    gb = torch.full((4, C), SENTINEL, dtype=torch.float32, device=dev)
    gb[1:3] = x["gb_prev"]
    o.merge_ln_bwd(dy, *st, gb_out=gb[1:3], accumulate=False)
    flags["equal_overwrite"] = float(torch.equal(gb[1], out["dgamma"]) and torch.equal(gb[2], out["dbeta"]))
    o.merge_ln_bwd(dy2, *st, gb_out=gb[1:3], accumulate=True)
    out["acc_dgamma"], out["acc_dbeta"] = gb[1].clone(), gb[2].clone()
    flags["equal_moat"] *= _moat(gb, (0, 3))
    return out, flags


def _run_l2(o, dev, case, dt, adt):
    x = {k: v.to(dev) for k, v in inputs(case, dt).items()}
    z, inv = o.l2norm_fwd(x["x"].to(adt))
    dx = o.l2norm_bwd(x["dz"].to(adt), x["z"].to(adt), x["inv"])
    flags = {}
    if case["edge"]:
        flags["equal_zero_row"] = float(bool((z[3] == 0).all()) and bool(torch.isfinite(dx).all()))
    return dict(z=z, inv=inv, dx=dx), flags


def _run_wn(o, dev, case, dt, adt):
    x = {k: v.to(dev) for k, v in inputs(case, dt).items()}
    w, inv = o.weightnorm_fwd(x["v"], x["g"], dtype=adt)
    out = dict(w=w, inv=inv)
    if dt == torch.float32:
        dv, dg = o.weightnorm_bwd(x["dw"], x["v"], x["g"], x["inv"], True)
        out.update(dv=dv, dg=dg.reshape(-1))
    return out, {}


def run(o, dev, case, dt, cast=None, repeat=False):
    """every entry point of the case through library o -> dict of fp64 CPU tensors (the statement's keys) and equal_* flags.  cast: the
    dtype activations are handed over and stored in (the fp32 restatement takes bf16-valued fp32).  repeat: a second launch of everything
    on the same inputs gave the same bits (these kernels have no atomics)"""
    fn = dict(ln=_run_ln, merge=_run_merge, l2=_run_l2, wn=_run_wn)[case["kind"]]
    raw, flags = fn(o, dev, case, dt, cast or dt)
    if repeat:
        again, _ = fn(o, dev, case, dt, cast or dt)
        flags["equal_repeat"] = float(all(torch.equal(raw[k], again[k]) for k in raw))
    res = {k: v.detach().cpu().double() for k, v in raw.items()}
    res.update(flags)
    return res


def ratio(got, ref, bound):
    """max |got - ref| / bound over every element; a non-finite value counts as inf"""
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bound).max()) if got.numel() else 0.0


def metrics(case, dt, got, ref=None):
    """err / bound of every output, with no exclusions, and the run's equal_* flags"""
    ref = reference(case, dt) if ref is None else ref
    m = {}
    for k in outputs(ref):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        m["ratio_" + k] = ratio(got[k], ref[k], ref["bd_" + k])
    m.update({k: v for k, v in got.items() if k.startswith("equal_")})
    return m


def failures(m):
    return ["%s = %.4g" % (k, v) for k, v in m.items() if (k.startswith("equal") and v != 1.0) or (k.startswith("ratio") and not v <= 1.0)]


def check(entry, case, dt, m, record=None, where="cpu"):
    """print (and record) every figure, then assert"""
    tag = dict(test="norm", entry=entry, case=case["name"], dtype=dt_name(dt), where=where)
    if record is not None:
        record(**tag, **m)
    print("OBSERVED", tag, m)
    bad = failures(m)
    assert not bad, (entry, case["name"], tag["dtype"], bad)


# ---- fp32 emulation in the kernels' order, and its mutants ----------------------------------------------------------------------------
MUTANTS = ("onepass_var", "unbiased_var", "eps_outside", "drop_last_iter", "garbage_lanes", "skip_second_trip", "fold_rpb_minus_1",
           "merge_swap", "rowscale_by_row", "gin_act_only", "accumulate_overwrites", "l2_clamp_sq", "wn_dg_no_inv")
# the cases that must catch each mutant (tests/test_norm_cpu.py asserts every one of them does, in every dtype of the case)
MUTANT_CASES = {
    "onepass_var": ("ln_num_mean1000_w96_e6", "ln_num_mean300_w1024_e5"),
    "unbiased_var": ("ln_w4_r1", "ln_w96_r65", "ln_w2048_r9"),
    "eps_outside": ("ln_num_const_w96_e6", "ln_num_const_w1024_e5", "ln_num_scales_w96_e5"),
    "drop_last_iter": ("ln_w320_r9", "ln_w576_r9", "l2_d260_r5", "wn_d1028_k5"),
    "garbage_lanes": ("ln_w4_r1", "ln_w48_r33", "ln_w160_r9", "ln_w320_r9", "ln_w1280_r9", "l2_d4_r1", "wn_d260_k9"),
    "skip_second_trip": ("ln_pass_w96", "ln_pass_w256", "ln_pass_w128", "ln_pass_w768"),
    "fold_rpb_minus_1": ("ln_w96_r65", "ln_w512_r9", "merge_3x6x10x96"),
    "merge_swap": ("merge_1x2x2x96", "merge_3x6x10x96", "merge_1x2x4x512"),
    "rowscale_by_row": ("ln_var_act_rs5_w96", "ln_var_act_rs3_w512"),
    "gin_act_only": ("ln_var_act_w96", "ln_var_act_rs1_w512"),
    "accumulate_overwrites": ("merge_1x2x2x96", "merge_2x4x6x128"),
    "l2_clamp_sq": ("l2_d4_r9", "l2_d2048_r9"),
    "wn_dg_no_inv": ("wn_d4_k1", "wn_d1028_k9"),
}
MUTANT_DTS = {"wn_dg_no_inv": (torch.float32,)}  # the backward of weight_norm is fp32 only
GARBAGE = 7.0


class Emulation:
    """the kernels in fp32 torch on the CPU: the same reduction shapes (hsum4, ITERS sequential additions, the shuffle butterfly; the row
    loop, the LDS fold and partial_reduce_kernel for dgamma / dbeta), the same rounding points up to the compiler's contractions"""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant
        self._act = torch.float32

    def set_act_dtype(self, dt):
        self._act = dt

    def act_dtype(self):
        return self._act

    # -- reductions --
    def _live(self, C, G):
        """channels the kernel reads: all of them, or (mutant) without the partly filled last iteration"""
        live = torch.ones(C)
        C4 = C // 4
        used = -(-C4 // G)
        if self.mutant == "drop_last_iter" and used > 1 and C4 % G:
            live[(used - 1) * G * 4:] = 0.0
        return live

    def _rowsum(self, X, G, it, garbage=False):
        """X [R, C] fp32 -> [R]: lane gl holds the vectors c4 = gl + it G (0 beyond C / 4), hsum4, ITERS additions, log2 G xor-shuffles"""
        R, C = X.shape
        P = torch.full((R, it * G * 4), GARBAGE if (garbage and self.mutant == "garbage_lanes") else 0.0)
        P[:, :C] = X
        V = P.view(R, it, G, 4)
        h = (V[..., 0] + V[..., 1]) + (V[..., 2] + V[..., 3])
        s = torch.zeros(R, G)
        for i in range(it):
            s = s + h[:, i]
        idx, o = torch.arange(G), G // 2
        while o:
            s = s + s[:, idx ^ o]
            o //= 2
        return s[:, 0].clone()

    @staticmethod
    def _partial_reduce(ws):
        """partial_reduce_kernel on ws [nblk, N]"""
        nblk, N = ws.shape
        SL = 32 if nblk >= 256 else 8
        t = torch.zeros(N)
        for ty in range(SL):
            acc = [torch.zeros(N) for _ in range(4)]
            b = ty
            while b + 3 * SL < nblk:
                for k in range(4):
                    acc[k] = acc[k] + ws[b + k * SL]
                b += 4 * SL
            while b < nblk:
                acc[0] = acc[0] + ws[b]
                b += SL
            t = t + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
        return t

    # -- LayerNorm --
    def _fwd(self, x, gamma, beta, eps, C):
        G, it, _ = ln_shape(C)
        live = self._live(C, G)
        xs = x * live
        mu = (self._rowsum(xs, G, it, garbage=True) / C).view(-1, 1)
        d = (xs - mu) * live
        q = self._rowsum(d * d, G, it)
        e = torch.tensor(eps, dtype=torch.float32)
        if self.mutant == "onepass_var":
            var = self._rowsum(xs * xs, G, it) / C - mu[:, 0] * mu[:, 0]
        elif self.mutant == "unbiased_var":
            var = q / (C - 1)
        else:
            var = q / C
        rs = 1.0 / (torch.sqrt(var) + e) if self.mutant == "eps_outside" else torch.rsqrt(var + e)
        y = ((x - mu) * rs.view(-1, 1) * gamma + beta) * live
        return y, mu[:, 0].clone(), rs

    def layernorm_fwd(self, x, gamma, beta, eps, *, rowmap=None, period_out=0, out_rows=None, want_f32=False, dtype=None):
        C = x.shape[-1]
        y, mean, rstd = self._fwd(x.reshape(-1, C), gamma, beta, eps, C)
        dt = dtype or self._act
        out = y.to(dt)
        if rowmap is not None:
            T = rowmap.numel()
            r = torch.arange(y.shape[0])
            out = torch.zeros((out_rows, C), dtype=dt)
            out[(r // T) * period_out + rowmap.long()[r % T]] = y.to(dt)
        return out, (y if want_f32 else None), mean, rstd

    def _bwd(self, x, d, mean, rstd, gamma, C, g_in=None, accumulate_into=None):
        """-> (dx before g_in, dx with it, dgamma, dbeta)"""
        G, it, rpb = ln_shape(C)
        rows = x.shape[0]
        live = self._live(C, G)
        nblk = ln_bwd_blocks(rows, C)
        mu, rs = mean.view(-1, 1), rstd.view(-1, 1)
        xh = (x - mu) * rs * live
        gd = d * gamma * live
        s1 = (self._rowsum(gd, G, it) / C).view(-1, 1)
        s2 = (self._rowsum(gd * xh, G, it) / C).view(-1, 1)
        o = (gd - s1 - xh * s2) * rs * live
        contrib = torch.cat([d * xh, d * live], 1)  # [rows, 2C]
        if self.mutant == "skip_second_trip":
            o[nblk * rpb:] = 0.0
            contrib[nblk * rpb:] = 0.0
        trips = -(-rows // (nblk * rpb))
        P = torch.zeros(trips * nblk * rpb, 2 * C)
        P[:rows] = contrib
        P = P.view(trips, nblk, rpb, 2 * C)
        acc = torch.zeros(nblk, rpb, 2 * C)
        for t in range(trips):
            acc = acc + P[t]
        s = torch.zeros(nblk, 2 * C)
        for g2 in range(rpb - (1 if self.mutant == "fold_rpb_minus_1" else 0)):
            s = s + acc[:, g2]
        gb = self._partial_reduce(s)
        if accumulate_into is not None and self.mutant != "accumulate_overwrites":
            gb = accumulate_into + gb
        return o, (o + g_in if g_in is not None else o), gb[:C].clone(), gb[C:].clone()

    @staticmethod
    def _to_gb(dg, db, gb_out):
        if gb_out is not None:
            gb_out[0].view(-1).copy_(dg)
            gb_out[1].view(-1).copy_(db)
            return gb_out[0].view(-1), gb_out[1].view(-1)
        return dg, db

    def layernorm_bwd(self, dy, x, mean, rstd, gamma, *, g_in=None, rowmap=None, period_in=0, gb_out=None):
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        d = dy.float().reshape(-1, C)
        if rowmap is not None:
            T = rowmap.numel()
            r = torch.arange(x2.shape[0])
            d = d[(r // T) * period_in + rowmap.long()[r % T]]
        _, dx, dg, db = self._bwd(x2, d, mean, rstd, gamma, C, g_in=None if g_in is None else g_in.reshape(-1, C))
        return (dx.reshape(x.shape),) + self._to_gb(dg, db, gb_out)

    def layernorm_bwd_cast(self, dy, x, mean, rstd, gamma, *, g_in=None, rowscale=None, rows_per_sample=0, gb_out=None):
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        o, dx, dg, db = self._bwd(x2, dy.float().reshape(-1, C), mean, rstd, gamma, C, g_in=None if g_in is None else g_in.reshape(-1, C))
        act = dx
        if self.mutant == "gin_act_only":
            dx = o
        if rowscale is not None:
            r = torch.arange(x2.shape[0])
            act = act * rowscale[(r % rowscale.numel()) if self.mutant == "rowscale_by_row" else r // rows_per_sample].view(-1, 1)
        return (dx.reshape(x.shape), act.to(dy.dtype)) + self._to_gb(dg, db, gb_out)

    def layernorm_bwd_to_act(self, dy, x, mean, rstd, gamma, *, gb_out=None):
        C = x.shape[-1]
        _, dx, dg, db = self._bwd(x.reshape(-1, C), dy.float().reshape(-1, C), mean, rstd, gamma, C)
        return (dx.to(self._act),) + self._to_gb(dg, db, gb_out)

    # -- merge --
    def _src(self, nB, H, W):
        return merge_rows(nB, H, W, swap=self.mutant == "merge_swap")

    def merge_ln_fwd(self, x, gamma, beta, eps, H, W, dtype=None, out=None):
        nB, L, Cin = x.shape
        xg = x.reshape(-1, Cin)[self._src(nB, H, W)].reshape(-1, 4 * Cin)
        y, mean, rstd = self._fwd(xg, gamma, beta, eps, 4 * Cin)
        y = y.to(dtype or self._act)
        if out is not None:
            out[0].copy_(y), out[1].copy_(mean), out[2].copy_(rstd)
            return out
        return y, mean, rstd

    def merge_ln_bwd(self, dy, x, mean, rstd, gamma, H, W, dx_out=None, gb_out=None, accumulate=False, act_out=None, rowscale=None):
        nB, L, Cin = x.shape
        src = self._src(nB, H, W)
        xg = x.reshape(-1, Cin)[src].reshape(-1, 4 * Cin)
        prev = torch.cat([gb_out[0], gb_out[1]]).clone() if (accumulate and gb_out is not None) else None
        _, dg, dgamma, dbeta = self._bwd(xg, dy.float(), mean, rstd, gamma, 4 * Cin, accumulate_into=prev)
        dx = torch.zeros(nB * L, Cin)
        dx[src.reshape(-1)] = dg.reshape(-1, Cin)
        if gb_out is not None:
            gb_out[0].copy_(dgamma), gb_out[1].copy_(dbeta)
            dgamma, dbeta = gb_out[0], gb_out[1]
        if act_out is not None:
            act_out.view(nB * L, Cin).copy_((dx if rowscale is None else dx * rowscale.view(-1, 1)).to(act_out.dtype))
        if dx_out is not None:
            dx_out.view(nB * L, Cin).copy_(dx)
            return dx_out, dgamma, dbeta
        return dx.view(nB, L, Cin), dgamma, dbeta

    # -- L2 normalise, weight_norm: one wave per row --
    def _wave(self, X, D, garbage=False):
        it = row_iters(D)
        live = self._live(D, 64)
        return self._rowsum(X * live, 64, it, garbage=garbage), live

    def l2norm_fwd(self, x):
        xf = x.float()
        q, live = self._wave(xf * xf, xf.shape[1], garbage=True)
        c = torch.tensor(L2_CLAMP, dtype=torch.float32)
        inv = 1.0 / torch.sqrt(torch.clamp(q, min=c)) if self.mutant == "l2_clamp_sq" else 1.0 / torch.clamp(torch.sqrt(q), min=c)
        return (xf * inv[:, None] * live).to(x.dtype), inv

    def l2norm_bwd(self, dz, z, inv):
        gg, zz = dz.float(), z.float()
        dot, live = self._wave(gg * zz, zz.shape[1])
        return ((gg - zz * dot[:, None]) * inv[:, None] * live).to(z.dtype)

    def weightnorm_fwd(self, v, g_, dtype=None):
        q, live = self._wave(v * v, v.shape[1], garbage=True)
        inv = 1.0 / torch.sqrt(q)
        return (v * (g_.view(-1) * inv)[:, None] * live).to(dtype or self._act), inv

    def weightnorm_bwd(self, dw, v, g_, inv, need_dg, dv_out=None):
        vh = v * inv[:, None]
        dot, live = self._wave(dw * vh, v.shape[1])
        dg = self._wave(dw * v, v.shape[1])[0] if self.mutant == "wn_dg_no_inv" else dot
        dv = (dw - vh * dot[:, None]) * (g_.view(-1) * inv)[:, None] * live
        if dv_out is not None:
            dv_out.copy_(dv)
            dv = dv_out
        return dv, (dg.view(-1, 1) if need_dg else None)
