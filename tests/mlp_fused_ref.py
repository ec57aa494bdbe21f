"""fp64 statement of the fused MLP branch  y = x + rowscale (GELU(LN(x) W1^T + b1) W2^T + b2)  and of its backward
(esvit_amd/csrc/mlp_fused.hip, mlp_fused16.hip, mlp_fused32p.hip, mlp_fused_dw.hip behind esvit_mlp_fused_fwd / _fwd_train / _bwd,
esvit_ln_fold_finish, esvit_cast_weight) that tests/test_mlp_fused_{cpu,gpu}.py compare against, the case table both share, the bounds,
the three GELU forms transcribed from the source, a host restatement of the launch geometry, and an fp32 emulation of every kernel with the
kernels' rounding points and 32-hidden chunking (with the mutants the CPU test needs).  The statement is plain torch in float64 and calls
nothing of oracle/ops_ref.py.  x, gy, the row scales and the parameters are fp32 and promoted; the bf16 weights are the statement's own
fp32 -> bf16 cast (round to nearest even) of the fp32 masters, the cast esvit_cast_weight performs on the device.

Bounds (u = 2^-24, b = 2^-9, g(n) = n u / (1 - n u); per element, none is tuned, none is read from a file).  ab_* is the expression with
every term replaced by its absolute value.  Errors propagate linearly; every bf16 pipeline's bound is doubled.  That doubling is what makes
the first-order bound right and leaves no slack of second order: round-to-nearest bf16 has unit roundoff 2^-8 and b = 2^-9 is half of
it, so an output that is one bf16 rounding of an accurate fp32 value (h, xhat, xw, gx_act, a1) sits at 1 / (1 + 2^-8) = 0.996 of its bound.
  LayerNorm (row statistics in registers: mlp_fused16.hip fused16.h row_stats, mlp_fused.hip:151-173, mlp_fused32p.hip:209-231,
  mlp_fused_dw.hip:131-149): the statement and bound of tests/norm_ref.py's ln_forward, restated with the depth of these kernels'
  reductions (ns = C / 4 + 2: a quarter row in one lane and two shuffles; C / 2 + 1 for the 32-token kernels) and with an input error
  e_in for the next-norm outputs:   e_mu = g(ns + 2) mean(|x| + e_in) + mean(e_in);  e_d = e_in + e_mu + u (|d| + e_in + e_mu);
  e_var = mean(2 |d| e_d + e_d^2) + g(ns + 3) mean((|d| + e_d)^2);  t = var + eps, e_t = e_var + u (t + e_var);
  e_rs = (t - e_t)^-1/2 - t^-1/2 + 2 u (rstd + ...) (rsqrtf: one ulp);  A = (|d| + e_d)(rstd + e_rs);  e_xhat = A - |d| rstd + g(2) A;
  e_LN = |gamma| e_xhat + 2 u (|gamma| A + |beta|).
  forward
    `xb[s][e] = (bf16)(...)`           mlp_fused16.hip:105, mlp_fused.hip:182, mlp_fused32p.hip:246     e_h = b (|h| + e_LN) + e_LN
    `p0 = mfma16(a0, xb[s], p0)`       the pre-activation, C products and the bias                      e_A = |W1| e_h + (C + 2) u ab_A
    `hf[r] = (bf16)gelu_f(p0[r] + bl)` mlp_fused16.hip:144, mlp_fused.hip:221, mlp_fused32p.hip:396     e_G = 1.13 e_A + delta_gelu + b |G|
                                       (1.13 > sup |GELU'| = 1.1290)
    `o[r] = xv[r] + rs * (acc2 + bb)`  mlp_fused16.hip:173, mlp_fused.hip:253, mlp_fused32p.hip:508     e_y = |rs| (|W2| e_G + (4C + 2) u ab) + 2 u |y|
    next norm (mlp_fused16.hip:180-192, mlp_fused.hip:262-297): the LayerNorm bound with e_in = e_y; xw leaves as bf16: + b |xw|
    training pass (mlp_fused32p.hip:419 a1 = (bf16)P, :437 a1g, :250 h, :234 mean / rstd): e_A + b |A|, e_G, e_h; e_mu, e_rs (fp32, not doubled)
  backward (mlp_fused16.hip:284-296 and mlp_fused_dw.hip:158-165 for LN(x), xhat and the scaled dy; :335-340 / :210-215 for GELU, GELU', dA)
    `dyb = (bf16)(sm * gv)`            e_dy = (u + b) |sm gy|
    `q0 = mfma16(t0, dyb[s], q0)`      e_Q = |W2|^T e_dy + (C + 2) u ab_Q
    `gelu_both(...)`                   e_dg = 0.8 e_A + delta_dgelu   (0.8 > sup |GELU''| = 2 phi(0) = 0.7979)
    `df[r] = (bf16)(q0[r] * dg)`       e_dA = |dg| e_Q + |Q| e_dg + e_Q e_dg + u |dA| + b |dA|
    `acc3 = mfma16(a, df, acc3)`       e_dH = |W1|^T e_dA + (4C + 2) u ab_dH
    `gd = acc3 * gm`, s1, s2           e_gd = |gamma| e_dH + u |gd|;  e_m1 = mean(e_gd) + g(ns + 3) ab_m1;
                                       e_m2 = mean(e_gd |xhat| + |gd| e_xhat + e_gd e_xhat) + g(ns + 6) ab_m2
    `o = gv + rstd * (gd - m1 - xh * m2)`   T = gd - m1 - xhat m2:  e_T = e_gd + e_m1 + |xhat| e_m2 + e_xhat (|m2| + e_m2) + 3 u ab_T
                                       e_gx = rstd e_T + e_rs (|T| + e_T) + 2 u ab_gx   (the rstd the kernel multiplies by: eps^-1/2 on a constant row)
    `gd = ro * o` -> bf16              e_gxa = |ro| e_gx + (u + b) |ro gx|;   xhat, a1g, da1 leave as bf16: e_xhat + b |xhat|, e_G, e_dA
  weight-gradient sums of the on-chip kernel (M rows in 64-row tiles, P = grid partials summed in index order, mlp_fused_dw.hip:317-335)
    dW2 = dyb^T Gb                     sum_rows (e_dy |G| + |dy| e_G + e_dy e_G) + (M + P) u ab       G, db1 = colsum(dAb), db2 = colsum(dyb) alike
  esvit_ln_fold_finish (mlp_fused.hip:333-362, fp32): dW = G gamma + db beta: g(3) ab;  dgamma / dbeta: a thread adds ceil(J / 32)
    products, 32 threads are folded: g(ceil(J / 32) + 33) ab (+ u |previous| + u |sum| with accumulate).
  delta_gelu / delta_dgelu: the three forms (common.h erf_fast / gelu_f, common.h gelu_both, mlp_fused32p.hip Gelu43 clamped at |a| = 4.5) are
  transcribed below, evaluated in fp32 on 2 400 001 points of [-12, 12], and compared with fp64 erf-GELU; the allowance is twice the
  largest deviation (the device's v_exp / v_rcp are one ulp off the CPU's) + 4 u (|A| + 1).  Measured (tests/test_mlp_fused_cpu.py
  holds these figures to the transcriptions):
      gelu_f 4.6e-07     gelu_both 4.6e-07 (value) / 3.0e-07 (derivative)     Gelu43 3.4e-05 (at |a| = 12, the tail beyond the clamp)
  all far below b |G|.  Every bound carries the floor 2^-100.
Second criterion (a wrong hidden unit among 4C hides under worst-case sums): for every output and every group of 16 consecutive rows
(weight-gradient sums: the whole tensor)   rms(device - fp64) <= 1.5 rms(emulation - fp64) + floor,   floor = the rms over the group
of 2 u |value|: the output's own last fp32 operations, which the device may contract into one rounding where the emulation makes two.
An output that is the direct result of a LayerNorm (h, xhat, mean, rstd of x; xw, mean_n, rstd_n of y) adds the fp32 bound of that one
LayerNorm on its exact input (e_in = 0): its row reduction runs in another order on the device, and on a constant row the emulation's
x - mean is exactly 0 where the device's is not.  Nothing that passes through a product is in the floor: a worst-case term propagated
through the sums (the accumulation terms, the LayerNorm error of h carried on to y, the GELU allowance) is of the size of the emulation's
whole error at C >= 192 and would bring back the looseness this criterion exists to get away from; the emulation carries the same kinds
of error (fp32 accumulation in another order, the transcribed GELU forms), inside rms(emulation - fp64) and under the factor 1.5.
The CPU test proves the
condition with no floor at all: the emulation in two other summation orders against 1.2 rms(emulation - fp64).

Case -> instantiation (w rows per wave, R rows per workgroup; `rows` labels: 1, w-1, w, w+1, R-1, R, R+1, big = 2R + 2w + 5):
  fwd  C = 96 / 128 / 256  fwd16_kernel<C, 8, LNN>   w 16  R 128        fwd  C = 192  mlp_fused_fwd_kernel<192, LNN>   w 32  R 128
  fwd / train  C = 384     mlp32p_fwd_kernel<384, SIDE>  w 32  R 128
  bwd  C = 96 / 128        bwd16_kernel<C, 6, 3>  w 16  R 96    C = 192  <192, 4, 2>  w 16  R 64    C = 256  <256, 8, 2>  w 16  R 128
  label -> (workgroups, live waves of the last workgroup):  1, w-1, w -> (1, 1);  w+1 -> (1, 2);  R-1, R -> (1, R / w);  R+1 -> (2, 1);  big -> (3, 3)
  dw   C = 96  mlp_dw_kernel, 64-row tiles, grid G = min(tiles, CUs):  rows -> (tiles, workgroups, most tiles of one workgroup)
       1, 63, 64 -> (1, 1, 1);  65 -> (2, 2, 1);  229 -> (4, 4, 1);  64 G + 1 -> (G + 1, G, 2);  128 G + 77 -> (2 G + 2, G, 3)
Families at the last row count: dense (x rows at 1, 1e-2, 1e2, gy rows at 1e-4 .. 1e2; rowscale / rowscale_mlp / rowscale_out drawn from
{0, 1 / 0.7, 1, 0.37} with a zero in the first row, the last row and on both sides of the first wave boundary -- a case of one row keeps
a factor, and the tracer family ends on a live row), tracer k = 0 .. 3 (selection
matrices: hidden unit j reads channel (5 j + j / C) mod C, output channel c reads hidden unit k C + c; on chip also at 65 and 229 rows,
whose last tiles end on a live row), for C = 384 also chunk
q in {0, 1, 22, 23, 46, 47} (channel c reads hidden unit 32 q + c mod 32), numerics (eps 1e-6 and 1e-5: rows with |mean| = 100 std,
constant rows, rows at 1e-4 and 1e4, pre-activations swept over [-12, 12] with +-4.5, its neighbours and +-0 hit exactly).
"""
import functools
import math

import torch

from tests import norm_ref as NR

U, BF, FLOOR, g, data = NR.U, NR.BF, NR.FLOOR, NR.g, NR.data
SENTINEL = NR.SENTINEL
BF16 = torch.bfloat16
HCH = 32
DW_T = 64
DW_PART = 2 * 96 * 384 + 384 + 96
EPS = 1e-6
GELU_SUP1, GELU_SUP2 = 1.13, 0.8
A_RANGE = 12.0


def _f32(v):
    return NR._f32(v)


def bf(t):
    return t.to(BF16).to(t.dtype)


# ---- the three GELU forms of the kernels, transcribed (fp32 torch) ------------------------------------------------------------------------
_AS = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
_SQ, _PDF = 0.70710678118654752, 0.39894228040143268


def _as_poly(t):
    return t * (_AS[0] + t * (_AS[1] + t * (_AS[2] + t * (_AS[3] + t * _AS[4]))))


def gelu_f(x):
    """common.h: gelu_f over erf_fast"""
    z = x * _SQ
    az = z.abs()
    t = 1.0 / (1.0 + 0.3275911 * az)
    r = 1.0 - _as_poly(t) * torch.exp(-az * az)
    return 0.5 * x * (1.0 + torch.copysign(r, z))


def gelu_both(v, density=True):
    """common.h: gelu_both -> (GELU, GELU')"""
    av = v.abs() * _SQ
    t = 1.0 / (1.0 + 0.3275911 * av)
    e = torch.exp(-0.5 * v * v)
    cdf = 0.5 * (1.0 + torch.copysign(1.0 - _as_poly(t) * e, v))
    return v * cdf, (cdf + v * _PDF * e) if density else cdf


_P43 = (3.989448530e-01, 2.708297554e-02, 3.837898957e-03, 3.371665041e-05)
_Q43 = (2.345878969e-01, 2.366735537e-02, 1.174744135e-03)


def gelu43(v, clamp=True):
    """mlp_fused32p.hip: Gelu43, stages 0 .. 11.  Not bit for bit: the source's __builtin_fmaf steps are a multiplication and an addition
    here (two roundings for one), and 1 / q stands for v_rcp_f32; both lie inside the doubled allowance"""
    u = v.clamp(-4.5, 4.5) if clamp else v
    s = u * u
    p = ((_P43[3] * s + _P43[2]) * s + _P43[1]) * s + _P43[0]
    q = ((_Q43[2] * s + _Q43[1]) * s + _Q43[0]) * s + 1.0
    return ((p * u) * (1.0 / q) + 0.5) * v


def gelu64(a):
    return 0.5 * a * torch.erfc(-a * math.sqrt(0.5))  # (erfc: the lower tail keeps its relative accuracy)


def dgelu64(a):
    return 0.5 * torch.erfc(-a * math.sqrt(0.5)) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)


@functools.lru_cache(maxsize=None)
def gelu_deviation():
    """largest |transcription in fp32 - fp64 erf-GELU| on the dense grid: {form: (value, derivative or None)}"""
    x = torch.linspace(-A_RANGE, A_RANGE, 2400001, dtype=torch.float64).float()
    x64 = x.double()
    want, dwant = gelu64(x64), dgelu64(x64)
    gb, dgb = gelu_both(x)
    return {"gelu_f": (float((gelu_f(x).double() - want).abs().max()), None),
            "gelu_both": (float((gb.double() - want).abs().max()), float((dgb.double() - dwant).abs().max())),
            "gelu43": (float((gelu43(x).double() - want).abs().max()), None)}


GELU_DOC = {"gelu_f": (4.6e-07, None), "gelu_both": (4.6e-07, 3.0e-07), "gelu43": (3.4e-05, None)}  # the docstring's figures


def delta_gelu(form, A, deriv=False):
    return 2.0 * gelu_deviation()[form][1 if deriv else 0] + 4.0 * U * (A.abs() + 1.0)


# ---- launch geometry, restated ---------------------------------------------------------------------------------------------------------
# (kind, C) -> (instantiation, rows per wave, rows per workgroup, GELU form)
INSTANCES = {
    ("fwd", 96): ("fwd16_kernel<96,8>", 16, 128, "gelu_f"), ("fwd", 128): ("fwd16_kernel<128,8>", 16, 128, "gelu_f"),
    ("fwd", 192): ("mlp_fused_fwd_kernel<192>", 32, 128, "gelu_f"), ("fwd", 256): ("fwd16_kernel<256,8>", 16, 128, "gelu_f"),
    ("fwd", 384): ("mlp32p_fwd_kernel<384,false>", 32, 128, "gelu43"), ("train", 384): ("mlp32p_fwd_kernel<384,true>", 32, 128, "gelu43"),
    ("bwd", 96): ("bwd16_kernel<96,6,3>", 16, 96, "gelu_both"), ("bwd", 128): ("bwd16_kernel<128,6,3>", 16, 96, "gelu_both"),
    ("bwd", 192): ("bwd16_kernel<192,4,2>", 16, 64, "gelu_both"), ("bwd", 256): ("bwd16_kernel<256,8,2>", 16, 128, "gelu_both"),
    ("dw", 96): ("mlp_dw_kernel", 16, 64, "gelu_both"),
}
ROW_LABELS = ("1", "w-1", "w", "w+1", "R-1", "R", "R+1", "big")
LABEL_GEOMETRY = {"1": (1, 1), "w-1": (1, 1), "w": (1, 1), "w+1": (1, 2), "R-1": (1, None), "R": (1, None), "R+1": (2, 1), "big": (3, 3)}
DW_CUS = 256  # the library's answer without a device; the GPU test asks the device


def row_counts(w, R):
    return dict(zip(ROW_LABELS, (1, w - 1, w, w + 1, R - 1, R, R + 1, 2 * R + 2 * w + 5)))


def dw_row_counts(G):
    return [1, 63, 64, 65, 64 * 3 + 37, 64 * G + 1, 64 * 2 * G + 77]


def dw_geometry_table(G):
    return {1: (1, 1, 1), 63: (1, 1, 1), 64: (1, 1, 1), 65: (2, 2, 1), 229: (4, 4, 1), 64 * G + 1: (G + 1, G, 2), 128 * G + 77: (2 * G + 2, G, 3)}


def geometry(case, G=DW_CUS):
    """from the launch formulas (ceil_div(M, 16 NW) / ceil_div(M, 128) / dw_grid): instantiation, workgroups, live waves of the last
    workgroup, most tiles of one workgroup"""
    inst, w, R, _ = INSTANCES[(case["kind"], case["C"])]
    M = case["M"]
    if case["kind"] == "dw":
        tiles = -(-M // DW_T)
        grid = min(tiles, G)
        return dict(inst=inst, tiles=tiles, wgs=grid, per_wg=-(-tiles // grid))
    wgs = -(-M // R)
    return dict(inst=inst, wgs=wgs, live=-(-(M - (wgs - 1) * R) // w), per_wg=1)


def ln_depth(kind, C):
    return C // 2 + 1 if INSTANCES[(kind, C)][1] == 32 else C // 4 + 2


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
CHUNKS_384 = (0, 1, 22, 23, 46, 47)


def _case(kind, C, M, label, family, nn=False, k=0, chunk=None, eps=EPS):
    name = "%s_c%d%s_%s_%s" % (kind, C, "_nn" if nn else "", "r" + label.replace("-", "m").replace("+", "p"), family)
    if family == "tracer":
        name += "_q%d" % chunk if chunk is not None else "_k%d" % k
    if family == "numerics":
        name += "_e%d" % round(-math.log10(eps))
    return dict(name=name, kind=kind, C=C, M=M, label=label, family=family, nn=nn, k=k, chunk=chunk, eps=eps)


def build_cases(G=DW_CUS):
    cs = []
    for (kind, C), (_, w, R, _) in INSTANCES.items():
        if kind == "dw":
            rows = [(str(m), m) for m in dw_row_counts(G)]
        else:
            rows = list(row_counts(w, R).items())
        for nn in ((False, True) if (kind == "fwd" and C != 384) else (False,)):
            for label, M in rows:
                cs.append(_case(kind, C, M, label, "dense", nn))
            if kind == "dw":  # ragged last tiles that end on a live row (the tracer family's last row keeps a factor)
                cs += [_case(kind, C, M, label, "tracer", nn, k=0) for label, M in rows[3:5]]
            label, M = rows[-1]
            for k in range(4):
                cs.append(_case(kind, C, M, label, "tracer", nn, k=k))
            if C == 384:
                for q in CHUNKS_384:
                    cs.append(_case(kind, C, M, label, "tracer", nn, chunk=q))
            for eps in (1e-6, 1e-5):
                cs.append(_case(kind, C, M, label, "numerics", nn, eps=eps))
    return cs


CASES = build_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
ROWSCALES = (0.0, 1.0 / 0.7, 1.0, 0.37)
FOLD_SHAPES = ((384, 96), (70, 45), (1, 1))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _rowscale(key, M, w, zeros=True):
    """factors drawn from ROWSCALES; zeros: a zero in the first row, the last row and on both sides of the first wave boundary.  A case of
    one row keeps a factor (its only row would otherwise show nothing of the branch), and the tracer family ends on a live row (a clamped
    row past M that is counted in the on-chip sums repeats the last row: it shows only where that row's factor is not zero)"""
    idx = torch.randint(0, 4, (M,), generator=NR._gen(*key))
    rs = torch.tensor(ROWSCALES, dtype=torch.float32)[idx]
    if M == 1:
        rs[0] = ROWSCALES[1]
    elif zeros:
        for r in (0, M - 1, w - 1, w):
            if 0 <= r < M:
                rs[r] = 0.0
    else:
        rs[0], rs[M - 1] = ROWSCALES[2], ROWSCALES[3]
    if M > 2:
        rs[1] = ROWSCALES[1]
    return rs


@functools.lru_cache(maxsize=4)
def _inputs(name, G):
    c = BY_NAME.get(name) or {x["name"]: x for x in build_cases(G)}[name]
    kind, C, M, fam = c["kind"], c["C"], c["M"], c["family"]
    H4, w = 4 * C, INSTANCES[(kind, C)][1]
    wide = C == 384
    r = torch.arange(M)
    z = data((name, "x"), (M, C))
    if fam == "numerics":
        t = (r % 6).view(M, 1)
        const = data((name, "xc"), (M, 1), scale=3.0).expand(M, C)
        x = torch.where(t == 0, z + 100.0, torch.where(t == 1, const, torch.where(t == 2, z * 1e-4, torch.where(t == 3, z * 1e4, torch.where(t == 4, z * 1.5 + 0.3, 0.01 * z - 1.0)))))
    else:
        x = (z * 1.5 + 0.3) * torch.tensor([1.0, 1e-2, 1e2])[r % 3].view(M, 1)
    gy = data((name, "gy"), (M, C), scale=0.5) * (10.0 ** ((r % 7).float() - 4.0)).view(M, 1)
    gamma, beta = 1.0 + data((name, "g"), (C,), scale=0.2), data((name, "b"), (C,), scale=0.1)
    b2 = data((name, "b2"), (C,), scale=0.1)
    j = torch.arange(H4)
    if fam == "tracer":
        W1 = torch.zeros(H4, C)
        W1[j, (5 * j + j // C) % C] = 0.5 + (j % 7).float() / 8.0
        b1 = -1.0 + 2.0 * j.float() / H4
        W2 = torch.zeros(C, H4)
        ch = torch.arange(C)
        W2[ch, (32 * c["chunk"] + ch % 32) if c["chunk"] is not None else (c["k"] * C + ch)] = 0.75 + (ch % 5).float() / 16.0
    elif fam == "numerics":
        W1 = data((name, "W1"), (H4, C), scale=0.004)
        b1 = torch.linspace(-11.5, 11.5, H4)
        special = [4.5, -4.5, 0.0, -0.0] + [float(torch.nextafter(torch.tensor(s * 4.5), torch.tensor(s * d))) for s in (1.0, -1.0) for d in (0.0, 9.0)]
        for i, v in enumerate(special):  # hidden units that read no channel: the pre-activation is the bias, exactly
            W1[37 * i + 5] = 0.0
            b1[37 * i + 5] = v
        W2 = data((name, "W2"), (C, H4), scale=0.04 if wide else 0.05)
    else:
        W1 = data((name, "W1"), (H4, C), scale=0.06 if wide else 0.08)
        b1 = data((name, "b1"), (H4,), scale=0.1)
        W2 = data((name, "W2"), (C, H4), scale=0.04 if wide else 0.05)
    return dict(x=x.contiguous(), gy=gy, gamma=gamma, beta=beta, W1=W1, b1=b1.float(), W2=W2, b2=b2, gamma_n=1.0 + data((name, "gn"), (C,), scale=0.2),
                beta_n=data((name, "bn"), (C,), scale=0.1), rs=_rowscale((name, "rs"), M, w, fam != "tracer"), rs_out=_rowscale((name, "ro"), M, w, fam != "tracer"))


def inputs(case, G=DW_CUS):
    """the case's fp32 tensors on the CPU (W1 / W2: the fp32 masters; rs: rowscale / rowscale_mlp; rs_out)"""
    return _inputs(case["name"], G)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def ln_stmt(x, gamma, beta, eps, ns, e_in=None):
    """LayerNorm of fp64 rows x (carrying the error e_in) -> dict of mean, rstd, xhat, y and their errors e_* (the bound of norm_ref's
    ln_forward at reduction depth ns)"""
    e_in = torch.zeros_like(x) if e_in is None else e_in
    ga, be = gamma.abs(), beta.abs()
    mu = x.mean(1, keepdim=True)
    e_mu = g(ns + 2) * (x.abs() + e_in).mean(1, keepdim=True) + e_in.mean(1, keepdim=True)
    d = x - mu
    e_d = e_in + e_mu + U * (d.abs() + e_in + e_mu)
    var = (d * d).mean(1, keepdim=True)
    e_var = (2 * d.abs() * e_d + e_d ** 2).mean(1, keepdim=True) + g(ns + 3) * ((d.abs() + e_d) ** 2).mean(1, keepdim=True)
    t = var + eps
    e_t = e_var + U * (t + e_var)
    rstd = t ** -0.5
    e_rs = torch.where(e_t < t, (t - e_t).clamp(min=1e-300) ** -0.5 - rstd, torch.full_like(t, float("inf")))
    e_rs = e_rs + 2 * U * (rstd + e_rs)
    A = (d.abs() + e_d) * (rstd + e_rs)
    xh = d * rstd
    e_xh = (A - d.abs() * rstd) + g(2) * A
    y = xh * gamma + beta
    e_y = ga * e_xh + 2 * U * (ga * A + be)
    return dict(mean=mu, e_mean=e_mu, rstd=rstd, e_rstd=e_rs, xhat=xh, e_xhat=e_xh, y=y, e_y=e_y)


def _weights(inp):
    return bf(inp["W1"]).double(), bf(inp["W2"]).double()


def _out(res, k, v, e, ab=None, double=True):
    res[k], res["bd_" + k] = v, (2.0 if double else 1.0) * e + FLOOR
    if ab is not None:
        res["ab_" + k] = ab


def _hidden(inp, case, b, form, x, ln, SU=U):
    """LN(x) rounded, the pre-activation, GELU: values and errors (SU: the u of the accumulation terms)"""
    C = case["C"]
    W1, W2 = _weights(inp)
    h = ln["y"]
    e_h = b * (h.abs() + ln["e_y"]) + ln["e_y"]
    b1 = inp["b1"].double()
    A = h @ W1.t() + b1
    ab_A = h.abs() @ W1.abs().t() + b1.abs()
    e_A = e_h @ W1.abs().t() + (C + 2) * SU * ab_A
    Gv = gelu64(A)
    e_G0 = GELU_SUP1 * e_A + delta_gelu(form, A)
    e_G = e_G0 + b * (Gv.abs() + e_G0)
    return dict(W1=W1, W2=W2, h=h, e_h=e_h, A=A, ab_A=ab_A, e_A=e_A, G=Gv, e_G=e_G)


def statement(case, G=DW_CUS, b=BF):
    """-> dict of fp64 outputs with bd_* (and ab_* where a sum forms them)"""
    SU, gs = U, g  # (the u of the accumulation terms, named apart from the single roundings)
    inp = inputs(case, G)
    kind, C, M = case["kind"], case["C"], case["M"]
    form = INSTANCES[(kind, C)][3]
    ns = ln_depth(kind, C)
    eps = _f32(case["eps"])
    x, gamma, beta = inp["x"].double(), inp["gamma"].double(), inp["beta"].double()
    ln = ln_stmt(x, gamma, beta, eps, ns)
    hd = _hidden(inp, case, b, form, x, ln, SU)
    W1, W2, Gv, e_G, A, e_A = hd["W1"], hd["W2"], hd["G"], hd["e_G"], hd["A"], hd["e_A"]
    rs = inp["rs"].double().view(M, 1)
    res = {}
    if kind in ("fwd", "train"):
        b2 = inp["b2"].double()
        br = Gv @ W2.t() + b2
        ab_br = Gv.abs() @ W2.abs().t() + b2.abs()
        y = x + rs * br
        e_y = rs.abs() * (e_G @ W2.abs().t() + (4 * C + 2) * SU * ab_br) + 2 * U * y.abs()
        _out(res, "y", y, e_y, x.abs() + rs.abs() * ab_br)
        if case["nn"]:
            nx = ln_stmt(y, inp["gamma_n"].double(), inp["beta_n"].double(), eps, ns, e_in=e_y)
            _out(res, "xw", nx["y"], nx["e_y"] + b * (nx["y"].abs() + nx["e_y"]))
            _out(res, "mean_n", nx["mean"][:, 0], nx["e_mean"][:, 0])
            _out(res, "rstd_n", nx["rstd"][:, 0], nx["e_rstd"][:, 0])
        if kind == "train":
            _out(res, "a1", A, e_A + b * (A.abs() + e_A), hd["ab_A"])
            _out(res, "a1g", Gv, e_G)
            _out(res, "h", hd["h"], hd["e_h"])
            _out(res, "mean", ln["mean"][:, 0], ln["e_mean"][:, 0], double=False)
            _out(res, "rstd", ln["rstd"][:, 0], ln["e_rstd"][:, 0], double=False)
        return res
    gy, ro = inp["gy"].double(), inp["rs_out"].double().view(M, 1)
    xh, e_xh, rstd, e_rs = ln["xhat"], ln["e_xhat"], ln["rstd"], ln["e_rstd"]
    dy = rs * gy
    e_dy = (U + b) * dy.abs()
    Q = dy @ W2
    ab_Q = dy.abs() @ W2.abs()
    e_Q = e_dy @ W2.abs() + (C + 2) * SU * ab_Q
    dg = dgelu64(A)
    e_dg = GELU_SUP2 * e_A + delta_gelu(form, A, deriv=True)
    da = Q * dg
    e_da0 = dg.abs() * e_Q + Q.abs() * e_dg + e_Q * e_dg + U * da.abs()
    e_da = e_da0 + b * (da.abs() + e_da0)
    dH = da @ W1
    ab_dH = da.abs() @ W1.abs()
    e_dH = e_da @ W1.abs() + (4 * C + 2) * SU * ab_dH
    gd = dH * gamma
    e_gd = gamma.abs() * e_dH + U * (gd.abs() + gamma.abs() * e_dH)
    mean = lambda t: t.mean(1, keepdim=True)  # noqa: E731
    m1, ab_m1 = mean(gd), mean(gd.abs() + e_gd)
    e_m1 = mean(e_gd) + gs(ns + 3) * ab_m1
    m2, ab_m2 = mean(gd * xh), mean((gd.abs() + e_gd) * (xh.abs() + e_xh))
    e_m2 = mean(e_gd * xh.abs() + gd.abs() * e_xh + e_gd * e_xh) + gs(ns + 6) * ab_m2
    T = gd - m1 - xh * m2
    ab_T = gd.abs() + ab_m1 + xh.abs() * ab_m2
    e_T = e_gd + e_m1 + xh.abs() * e_m2 + e_xh * (m2.abs() + e_m2) + 3 * U * ab_T
    gx = gy + rstd * T
    ab_gx = gy.abs() + rstd * ab_T
    e_gx = rstd * e_T + e_rs * (T.abs() + e_T) + 2 * U * ab_gx
    _out(res, "gx", gx, e_gx, ab_gx)
    gxa = ro * gx
    _out(res, "gx_act", gxa, ro.abs() * e_gx + (U + b) * gxa.abs())
    e_xhb = e_xh + b * (xh.abs() + e_xh)
    if kind == "bwd":
        _out(res, "xhat", xh, e_xhb)
        _out(res, "a1g", Gv, e_G)
        _out(res, "da1", da, e_da)
        return res
    n = (M + min(-(-M // DW_T), G)) * SU
    ab = dy.abs().t() @ Gv.abs()
    _out(res, "dW2", dy.t() @ Gv, e_dy.t() @ Gv.abs() + dy.abs().t() @ e_G + e_dy.t() @ e_G + n * ab, ab)
    ab = da.abs().t() @ xh.abs()
    _out(res, "G", da.t() @ xh, e_da.t() @ xh.abs() + da.abs().t() @ e_xhb + e_da.t() @ e_xhb + n * ab, ab)
    _out(res, "db1", da.sum(0), e_da.sum(0) + n * da.abs().sum(0), da.abs().sum(0))
    _out(res, "db2", dy.sum(0), e_dy.sum(0) + n * dy.abs().sum(0), dy.abs().sum(0))
    return res


def fold_stmt(Gm, db, W, gamma, beta, prev=None):
    """esvit_ln_fold_finish in fp64: dW, dgamma, dbeta (+ prev = (dgamma, dbeta) with accumulate) and their bounds"""
    J = Gm.shape[0]
    n = -(-J // 32) + 33
    res = {}
    ab = Gm.abs() * gamma.abs() + db.abs().view(-1, 1) * beta.abs()
    _out(res, "dW", Gm * gamma + db.view(-1, 1) * beta, g(3) * ab, ab, double=False)
    for k, v, a in (("dgamma", (W * Gm).sum(0), (W * Gm).abs().sum(0)), ("dbeta", (db.view(-1, 1) * W).sum(0), (db.view(-1, 1) * W).abs().sum(0))):
        e = g(n) * a
        if prev is not None:
            p = prev[0 if k == "dgamma" else 1]
            e = e + U * (p.abs() + a)
            v, a = v + p, a + p.abs()
        _out(res, k, v, e, a, double=False)
    return res


def fold_inputs(J, C):
    key = ("fold", J, C)
    return dict(G=data(key + ("G",), (J, C)), db=data(key + ("db",), (J,)), W=data(key + ("W",), (J, C), scale=0.08), gamma=1.0 + data(key + ("g",), (C,), scale=0.2),
                beta=data(key + ("b",), (C,), scale=0.1), prev=(data(key + ("pg",), (C,), scale=3.0), data(key + ("pb",), (C,), scale=3.0)))


def perm32(n):
    """esvit_hip.h: position 8g + e of an aligned 32-block holds column 4g + e (e < 4) / 16 + 4g + (e - 4)"""
    p = torch.arange(n)
    gg, e = (p >> 3) & 3, p & 7
    return 32 * (p >> 5) + torch.where(e < 4, 4 * gg + e, 16 + 4 * gg + (e - 4))


def cast_weight_stmt(src, transpose, perm):
    out = (src.t() if transpose else src).to(BF16)
    return out[:, perm32(out.shape[1])].contiguous() if perm else out.contiguous()


# ---- references, metrics -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _reference(name, G):
    case = BY_NAME.get(name) or {x["name"]: x for x in build_cases(G)}[name]
    ref = statement(case, G)
    own = _ln_direct(case, ref, G)
    for k in outputs(ref):  # the floor of the second criterion (module docstring)
        ref["fl_" + k] = 2.0 * U * ref[k].abs() + own.get(k, 0.0) + FLOOR
    ref["emu_rms"] = {k: group_rms(v - ref[k], case, k) for k, v in emulate(case, G).items() if torch.is_tensor(v)}
    return ref


def reference(case, G=DW_CUS):
    """the statement, its bounds, the floors and the emulation's rms error per group"""
    return _reference(case["name"], G)


def outputs(ref):
    return [k for k in ref if "bd_" + k in ref]


def _ln_direct(case, ref, G):
    """the fp32 error of the LayerNorm whose direct result an output is, taken of that LayerNorm's exact input (x; the statement's y for the
    next norm): {output: error}.  It passes through no product"""
    inp = inputs(case, G)
    ns, eps = ln_depth(case["kind"], case["C"]), _f32(case["eps"])
    ln = ln_stmt(inp["x"].double(), inp["gamma"].double(), inp["beta"].double(), eps, ns)
    own = dict(h=ln["e_y"], xhat=ln["e_xhat"], mean=ln["e_mean"][:, 0], rstd=ln["e_rstd"][:, 0])
    if "xw" in ref:
        nx = ln_stmt(ref["y"], inp["gamma_n"].double(), inp["beta_n"].double(), eps, ns)
        own.update(xw=nx["e_y"], mean_n=nx["e_mean"][:, 0], rstd_n=nx["e_rstd"][:, 0])
    return own


ROW_OUTPUTS = ("y", "xw", "mean_n", "rstd_n", "a1", "a1g", "h", "mean", "rstd", "gx", "gx_act", "xhat", "da1")


def group_rms(err, case, key):
    """rms over groups of 16 consecutive rows (a wave's tokens) of a row-indexed tensor -> [groups]; over all of a weight-gradient sum -> [1]"""
    e2 = err.double() ** 2
    if key not in ROW_OUTPUTS:
        return e2.mean().sqrt().view(1)
    e2 = e2.reshape(case["M"], -1).mean(1)
    n = -(-case["M"] // 16)
    pad = torch.zeros(n * 16, dtype=torch.float64)
    cnt = torch.zeros(n * 16, dtype=torch.float64)
    pad[:case["M"]], cnt[:case["M"]] = e2, 1.0
    return (pad.view(n, 16).sum(1) / cnt.view(n, 16).sum(1)).sqrt()


def ratio(got, want, bound):
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs() / bound).max()) if got.numel() else 0.0


def metrics(case, got, ref, factor=1.5, floor=True):
    """ratio_*: max err / bound per output;  rms_*: max over the groups of rms(got - fp64) / (factor rms(emulation - fp64) + floor);
    floor = False: against the emulation alone (2^-100 keeps 0 / 0 out)"""
    m = {}
    for k in outputs(ref):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        m["ratio_" + k] = ratio(got[k], ref[k], ref["bd_" + k])
        if m["ratio_" + k] == float("inf"):
            m["rms_" + k] = float("inf")
            continue
        allow = factor * ref["emu_rms"][k] + (group_rms(ref["fl_" + k], case, k) if floor else FLOOR)
        m["rms_" + k] = float((group_rms(got[k] - ref[k], case, k) / allow).max())
    m.update({k: v for k, v in got.items() if k.startswith(("equal_", "ratio_"))})
    return m


def colsum_ratio(s, rows, n_partials):
    """a column sum of the on-chip kernel against the fp64 sum of the rounded rows it adds: only the fp32 additions lie between them,
    (rows + partials) u sum |terms|"""
    r = rows.double()
    bound = (r.shape[0] + n_partials) * U * r.abs().sum(0) + FLOOR
    return ratio(s.double(), r.sum(0), bound)


def failures(m):
    return ["%s = %.4g" % (k, v) for k, v in m.items() if (k.startswith("equal") and v != 1.0) or (k.startswith(("ratio", "rms")) and not v <= 1.0)]


def check(entry, case, m, record=None, where="cpu"):
    """print (and record) every figure, then assert"""
    tag = dict(test="mlp_fused", entry=entry, case=case["name"], where=where)
    if record is not None:
        record(**tag, **m)
    print("OBSERVED", tag, m)
    bad = failures(m)
    assert not bad, (entry, case["name"], bad)


# ---- fp32 emulation with the kernels' rounding points and 32-hidden chunking, and its mutants ------------------------------------------
MUTANTS = ("perm_swap", "stale_bias", "drop_last_chunk", "first_chunk_twice", "wave_shift", "rowscale_on_x", "b2_unscaled", "eps_dropped",
           "dgelu_no_density", "cdf_unclamped", "gxa_rowscale_mlp", "ln_as_xhat", "next_norm_of_x", "dw_clamped_row", "dw_last_partial", "dw_db1_unrounded", "one_hidden_unit")
MUTANT_CASES = {
    "one_hidden_unit": ("fwd_c384_rbig_dense", "fwd_c384_rbig_numerics_e6", "train_c384_rbig_dense", "fwd_c256_nn_rbig_dense", "bwd_c256_rbig_dense",
                        "dw_c96_r229_dense"),
    "perm_swap": ("fwd_c96_rbig_tracer_k0", "bwd_c128_rbig_tracer_k2", "fwd_c256_nn_rbig_dense"),
    "stale_bias": ("fwd_c96_rbig_tracer_k1", "fwd_c384_rbig_tracer_q1", "bwd_c192_rbig_tracer_k0", "train_c384_rbig_tracer_q23"),
    "drop_last_chunk": ("fwd_c192_rbig_tracer_k3", "fwd_c384_rbig_tracer_q47", "bwd_c256_rbig_tracer_k3", "dw_c96_r229_dense", "fwd_c128_r1_dense"),
    "first_chunk_twice": ("fwd_c128_nn_rbig_tracer_k0", "fwd_c384_rbig_tracer_q0", "bwd_c96_rbig_tracer_k0", "train_c384_r1_dense"),
    "wave_shift": ("fwd_c96_rbig_dense", "bwd_c192_rRp1_dense", "train_c384_rbig_dense", "dw_c96_r65_dense"),
    "rowscale_on_x": ("fwd_c96_rbig_dense", "fwd_c192_nn_rw_dense", "train_c384_rRm1_dense"),
    "b2_unscaled": ("fwd_c128_rbig_dense", "fwd_c384_rR_dense", "fwd_c256_rbig_tracer_k1"),
    "eps_dropped": ("fwd_c96_rbig_numerics_e6", "bwd_c256_rbig_numerics_e5", "train_c384_rbig_numerics_e5", "dw_c96_r%d_numerics_e6" % (128 * DW_CUS + 77)),
    "dgelu_no_density": ("bwd_c96_rbig_dense", "bwd_c128_rbig_numerics_e6", "dw_c96_r64_dense"),
    "cdf_unclamped": ("fwd_c384_rbig_numerics_e6", "train_c384_rbig_numerics_e5"),
    "gxa_rowscale_mlp": ("bwd_c96_rbig_dense", "bwd_c256_rRp1_dense", "dw_c96_r63_dense"),
    "ln_as_xhat": ("bwd_c192_rbig_dense", "train_c384_rbig_dense", "bwd_c128_rwm1_dense"),
    "next_norm_of_x": ("fwd_c96_nn_rbig_dense", "fwd_c192_nn_rbig_tracer_k2", "fwd_c256_nn_r1_dense"),
    "dw_clamped_row": ("dw_c96_r1_dense", "dw_c96_r65_tracer_k0", "dw_c96_r229_tracer_k0"),
    "dw_last_partial": ("dw_c96_r229_dense", "dw_c96_r%d_dense" % (128 * DW_CUS + 77), "dw_c96_r%d_tracer_k0" % (128 * DW_CUS + 77)),
    "dw_db1_unrounded": ("dw_c96_r64_dense", "dw_c96_r65_dense", "dw_c96_r229_dense"),
}
# the mutants tried, in this order, when the CPU test shows that every case catches one
CATCH_ALL = ("drop_last_chunk", "first_chunk_twice", "stale_bias")


def _ln32(x, gamma, beta, eps, drop_eps=False):
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = torch.rsqrt(var if drop_eps else var + torch.tensor(eps, dtype=torch.float32))
    xh = d * rstd
    return mean, rstd, xh, xh * gamma + beta


def emulate(case, G=DW_CUS, mutant=None, order="chunk"):
    """the case through the fp32 emulation -> dict of fp64 tensors (the statement's keys).  order: "chunk" (the kernels': hidden chunks of
    32 in ascending order), "matmul" (one product over all hidden units), "reversed" (chunks, and the on-chip partials, in descending order)"""
    assert mutant is None or mutant in MUTANTS
    inp = inputs(case, G)
    kind, C, M = case["kind"], case["C"], case["M"]
    H4, NCH = 4 * C, 4 * C // HCH
    _, w, R, form = INSTANCES[(kind, C)]
    eps = _f32(case["eps"])
    x, gy, gamma, beta, b1, b2 = (inp[k] for k in ("x", "gy", "gamma", "beta", "b1", "b2"))
    W1, W2 = bf(inp["W1"]), bf(inp["W2"])
    rs, ro = inp["rs"].view(M, 1), inp["rs_out"].view(M, 1)
    if mutant == "perm_swap":  # positions 9 and 10 of the second 32-block of the permuted fc1 copy hold each other's channel
        p = perm32(C).tolist()
        a, c_ = p[32 + 9], p[32 + 10]
        W1 = W1.clone()
        W1[:, [a, c_]] = W1[:, [c_, a]]
    mean, rstd, xh, h = _ln32(x, gamma, beta, eps, drop_eps=mutant == "eps_dropped")
    hb = bf(h)
    back = kind in ("bwd", "dw")
    dyb = bf(rs * gy) if back else None
    clamped = None
    if kind == "dw" and mutant == "dw_clamped_row" and M % DW_T:  # the rows past M of the last tile: row M - 1 again, its dy not zeroed
        clamped = DW_T - M % DW_T

    def act(P):
        if form == "gelu43":
            return gelu43(P, clamp=mutant != "cdf_unclamped"), None
        if form == "gelu_f":
            return gelu_f(P), None
        return gelu_both(P, density=mutant != "dgelu_no_density")

    chunks = [list(range(HCH * q, HCH * q + HCH)) for q in range(NCH)]
    if order == "matmul":
        chunks = [list(range(H4))]
    if order == "reversed":
        chunks = chunks[::-1]
    acc = torch.zeros(M, C)
    A_all, G_all, dA_all, dA_raw = (torch.zeros(M, H4) for _ in range(4))
    for idx in chunks:
        q = idx[0] // HCH
        bq = b1[idx]
        if mutant == "stale_bias" and order != "matmul" and q >= 1:  # a chunk reads the bias piece of the chunk before it
            bq = b1[[i - HCH for i in idx]]
        P = hb @ W1[idx].t() + bq
        gl, dg = act(P)
        Gb = bf(gl)
        lost = 4 * C - 41  # one hidden unit of the 4C contributes nothing to y / gx
        if mutant == "one_hidden_unit" and lost in idx:
            Gb = Gb.clone()
            Gb[:, idx.index(lost)] = 0.0
        A_all[:, idx], G_all[:, idx] = P, bf(gl)
        reps = 0 if (mutant == "drop_last_chunk" and q == NCH - 1) else (2 if (mutant == "first_chunk_twice" and q == 0) else 1)
        if back:
            raw = (dyb @ W2[:, idx]) * dg
            dab = bf(raw)
            dA_all[:, idx], dA_raw[:, idx] = dab, raw
            if mutant == "one_hidden_unit" and lost in idx:
                dab = dab.clone()
                dab[:, idx.index(lost)] = 0.0
            for _ in range(reps):
                acc = acc + dab @ W1[idx]
        else:
            for _ in range(reps):
                acc = acc + Gb @ W2[:, idx].t()
    out = {}
    if not back:
        if mutant == "rowscale_on_x":
            y = rs * x + rs * (acc + b2)
        elif mutant == "b2_unscaled":
            y = x + rs * acc + b2
        else:
            y = x + rs * (acc + b2)
        out["y"] = y
        if case["nn"]:
            src, gn = (x, gamma) if mutant == "next_norm_of_x" else (y, inp["gamma_n"])
            mn, rn, _, xw = _ln32(src, gn, inp["beta_n"], eps)
            out.update(xw=bf(xw), mean_n=mn[:, 0], rstd_n=rn[:, 0])
        if kind == "train":
            out.update(a1=bf(A_all), a1g=G_all, h=bf(xh) if mutant == "ln_as_xhat" else hb, mean=mean[:, 0], rstd=rstd[:, 0])
    else:
        gd = acc * gamma
        m1, m2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
        o = gy + rstd * (gd - m1 - xh * m2)
        out["gx"] = o
        out["gx_act"] = bf((ro * rs if mutant == "gxa_rowscale_mlp" else ro) * o)
        if kind == "bwd":
            out.update(xhat=hb if mutant == "ln_as_xhat" else bf(xh), a1g=G_all, da1=dA_all)
        else:
            xhb = bf(xh)
            dyu, Gu, dAu, xhu, dAr = dyb, G_all, dA_all, xhb, dA_raw
            if clamped:
                last = lambda t, v=None: torch.cat([t, (t[-1:] if v is None else v).expand(clamped, -1)])  # noqa: E731
                dyu, Gu, dAu, xhu, dAr = last(dyb, bf(rs[-1:] * gy[-1:])), last(G_all), last(dA_all), last(xhb), last(dA_raw)
            src1 = dAr if mutant == "dw_db1_unrounded" else dAu
            if order == "matmul":
                out.update(dW2=dyu.t() @ Gu, G=dAu.t() @ xhu, db1=src1.sum(0), db2=dyu.sum(0))
            else:
                rows = dyu.shape[0]
                nt = -(-rows // DW_T)
                grid = min(nt, G)

                def tiles(t):
                    p = torch.zeros(nt * DW_T, t.shape[1])
                    p[:rows] = t
                    return p.view(nt, DW_T, -1)
                dyt, Gt, dAt, xht, s1t = tiles(dyu), tiles(Gu), tiles(dAu), tiles(xhu), tiles(src1)
                per = dict(dW2=dyt.transpose(1, 2) @ Gt, G=dAt.transpose(1, 2) @ xht, db1=s1t.sum(1), db2=dyt.sum(1))
                blocks = list(range(grid))
                if mutant == "dw_last_partial" and grid > 1:
                    blocks = blocks[:-1]
                if order == "reversed":
                    blocks = blocks[::-1]
                for k, t in per.items():
                    tot = torch.zeros(t.shape[1:])
                    for blk in blocks:
                        part = torch.zeros(t.shape[1:])
                        for i in range(blk, nt, grid):
                            part = part + t[i]
                        tot = tot + part
                    out[k] = tot
    if mutant == "wave_shift":  # the second wave (the first where there is one wave only) stores the rows one below its own
        lo = w if M > w else 0
        hi = min(lo + w, M)
        src = torch.arange(lo, hi).add(1).clamp(max=M - 1)
        for k in out:
            if k in ROW_OUTPUTS:
                out[k] = out[k].clone()
                out[k][lo:hi] = out[k][src].clone()
    res = {k: v.double() for k, v in out.items()}
    if kind == "dw":  # db1 / db2 against the rounded dA / dy of the same run
        P = min(-(-M // DW_T), G)
        res["ratio_db1_sum"], res["ratio_db2_sum"] = colsum_ratio(out["db1"], dA_all, P), colsum_ratio(out["db2"], dyb, P)
    return res


def fold_emulate(Gm, db, W, gamma, beta, prev=None):
    """ln_fold_finish_kernel in fp32: thread ty adds rows ty, ty + 32, ..; 32 partial sums are folded in order"""
    J, C = Gm.shape
    dW = Gm * gamma + db.view(-1, 1) * beta
    pad = -(-J // 32) * 32
    pg, pb = torch.zeros(pad, C), torch.zeros(pad, C)
    pg[:J], pb[:J] = W * Gm, db.view(-1, 1) * W
    ag, ab = torch.zeros(32, C), torch.zeros(32, C)
    for i in range(pad // 32):
        ag, ab = ag + pg[32 * i:32 * i + 32], ab + pb[32 * i:32 * i + 32]
    a, b_ = torch.zeros(C), torch.zeros(C)
    for i in range(32):
        a, b_ = a + ag[i], b_ + ab[i]
    if prev is not None:
        a, b_ = prev[0] + a, prev[1] + b_
    return dict(dW=dW.double(), dgamma=a.double(), dbeta=b_.double())
