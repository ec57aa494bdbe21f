"""fp64 statement of the convolution and BatchNorm kernels (esvit_amd/csrc/conv.hip) that tests/test_conv_{cpu,gpu}.py compare against,
the case table both share, and the bounds.  Every function here is plain index arithmetic (a table of source positions per tap, a
gather or a scatter-add); nothing goes through F.unfold, F.fold or conv2d as oracle/ops_ref.py does.  Inputs are made in the case's
dtype and promoted, so bf16 inputs are exact in the reference.  Each function also returns `abs_sum`, the sum of |terms| per output
element, which is what a rounding bound scales with.

Bounds (u = 2^-24; none is tuned, none is read from a file):
  pure copies (im2col on all four paths, pad, crop)  torch.equal, zero tail included; fp32 NCHW -> bf16 columns: torch's RNE cast
  dwconv forward      |got - ref| <= 10 u abs_sum (nine products and eight additions, fused or not)      bf16: + 2^-8 |ref|
  col2im              T u abs_sum, T = ceil(k / stride)^2 terms at most per element; fp32 output in both modes
  affine act 0, 3     4 u (|a1 x1| + |a2 x2| + |a3|)                                                     bf16: + 2^-8 |ref|
  affine act 4        == x2 or 0 exactly where the fp64 pre-activation has |v| > 4 u (|a1 x1| + |a3|); inside the band either; an
                      element whose terms are all zero is computed exactly and must give 0
  affine act 1, 2     max(3 x the error of fp32 torch (oracle/ops_ref.col_affine2) on the same inputs, 16 u max|ref|): the device's
                      erf / exp cannot be derived here                                                   bf16: + 2^-8 |ref|
  reductions          (L + 1) u abs_sum, L = the longest chain of additions of the launch (reduce_chain below): a worst-case bound
  BN coefficients     rstd: 8 u cond relative, cond = 1 + (s2/n + mean^2) / (var + eps); the rest by propagation (bn_fwd_bounds)
  BN end to end       rstd relative error <= 8 (1 + r^2) u at mean / std = r

Case -> kernel (dispatch conditions of conv.hip; `off` = a contiguous view 4 elements into its buffer: 8 bytes in bf16, so every
16-byte test fails while the fallback's own 8-byte loads are still aligned; 16 bytes in fp32, where it changes nothing):
  entry point     kernel                          reached by (bf16 unless said)                        grid-stride loop taken twice by
  conv_im2col     im2col_nhwc_vec_kernel<bf16>    NHWC, Cin % 8 == 0, aligned: vil_k2, cvt_*_c64, c192  big_nhwc_vec (> 8192 * 256 vectors)
                  im2col_nchw_vec_kernel          NCHW (fp32 image -> bf16 columns): stem*, vil_k4      big_nchw_vec
                  im2col_kernel<bf16>             NHWC, Cin in (3, 12), or off at Cin = 64              big_elem/bf16 (> 8192 * 256 elements)
                  im2col_kernel<float>            every fp32 case, NCHW and NHWC                        big_elem/fp32
  conv_col2im     col2im_vec_kernel               Cin % 8 == 0, aligned                                 big_vec
                  col2im_kernel<bf16>             Cin in (3, 12), or off                                big_elem/bf16
                  col2im_kernel<float>            every fp32 case                                       big_elem/fp32
  dwconv3x3       dwconv3x3_strip_kernel          C % 8 == 0, aligned (C up to 2048)                    big_strip (strips > 2048 * PY)
                  dwconv3x3_kernel<bf16>          C in (4, 12, 20), or off                              big_pos/bf16 (off; positions > 4096 * PY)
                  dwconv3x3_kernel<float>         every fp32 case (C <= 1024)                           big_pos/fp32
  dwconv3x3_wgrad dwconv3x3_wgrad_strip_kernel    C % 8 == 0, aligned                                   loop_c2048 (strips > 512 * PY)
                  dwconv3x3_wgrad_kernel<bf16>    C in (4, 12, 20), or off                              loop_c1024_off (positions > 512 * PY)
                  dwconv3x3_wgrad_kernel<float>   every fp32 case                                       loop_c192, loop_c1024_off
  col_sums2       col_sums2_kernel<bf16|float>    C <= 1024                                             r2697_c192, r529_c1024 (rows > 512 * PY)
                  col_sums2_wide_kernel<..>       C in (2048, 4096)                                     r600_c2048 (rows > 512)
  col_affine2     col_affine2_kernel<T, 0..4>     act 0 (with and without x2), 1, 2, 3, 4               big (> 8192 * 256 elements), every act
  pad_crop_tokens pad_crop_kernel<bf16|float>     pad, crop, both at once                               big
  bn_*            the four coefficient kernels    C = 40 and 300 (a second workgroup)                   (no loop)
PY = position lanes of a workgroup: max(256 // (C / 4), 1) in the per-channel kernels, max(256 // (C / 8), 1) in the strip kernels.
"""
import math
import zlib

import torch

U = 2.0 ** -24
BF = 2.0 ** -8
DTYPES = (torch.float32, torch.bfloat16)
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
OFF = 4  # elements


def dt_name(dt):
    return {torch.float32: "fp32", torch.bfloat16: "bf16"}[dt]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()) % (2 ** 31))


def data(key, shape, dt, scale=1.0, shift=0.0):
    """seeded values stored as dt (on the CPU)"""
    return (torch.randn(*shape, generator=_gen(*key)) * scale + shift).to(dt)


def place(t, dev, off=0):
    """t on `dev` as a contiguous tensor whose first element lies `off` elements into a fresh (>= 16-byte aligned) buffer"""
    if t is None:
        return None
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def kpad(k, Cin):
    return -(-(k * k * Cin) // 8) * 8


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _taps(nB, H, W, k, stride, pad, mutant=None):
    """-> (pos, live), both [nB, Ho, Wo, k, k]: the source position b H W + iy W + ix of tap (ky, kx) of output (b, oy, ox) and
    whether it lies inside the grid.  Mutants: hw_swap (row stride H), border_kept (the row above the grid reads row 0),
    border_dropped (the last column is not read through the last tap of a row)."""
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    ar = torch.arange
    b = ar(nB).view(nB, 1, 1, 1, 1)
    iy = ar(Ho).view(1, Ho, 1, 1, 1) * stride - pad + ar(k).view(1, 1, 1, k, 1)
    ix = ar(Wo).view(1, 1, Wo, 1, 1) * stride - pad + ar(k).view(1, 1, 1, 1, k)
    inx = (ix >= 0) & (ix < W)
    live = (iy >= 0) & (iy < H) & inx
    if mutant == "border_kept":
        live = live | ((iy == -1) & inx)
    if mutant == "border_dropped":
        live = live & ~((ix == W - 1) & (ar(k).view(1, 1, 1, 1, k) == k - 1))
    rs = H if mutant == "hw_swap" else W
    pos = (b * (H * W) + iy.clamp(0, H - 1) * rs + ix.clamp(0, W - 1)).clamp(0, nB * H * W - 1)
    pos, live = torch.broadcast_tensors(pos, live)
    return pos.contiguous(), live.contiguous()


def im2col_ref(src, nchw, nB, H, W, Cin, k, stride, pad, out_dt, mutant=None):
    """-> cols [nB Ho Wo, Kpad] in out_dt, columns (ky, kx, c), zero tail: a copy (fp32 NCHW -> bf16: torch's round-to-nearest-even)"""
    pos, live = _taps(nB, H, W, k, stride, pad, mutant)
    src2d = src.view(nB, Cin, H * W).transpose(1, 2).reshape(nB * H * W, Cin) if nchw else src.view(nB * H * W, Cin)
    vals = src2d[pos.reshape(-1)]
    vals = torch.where(live.reshape(-1, 1), vals, torch.zeros_like(vals))
    rows, KK = pos.shape[0] * pos.shape[1] * pos.shape[2], k * k * Cin
    cols = torch.zeros((rows, kpad(k, Cin)), dtype=out_dt)
    cols[:, :KK] = vals.reshape(rows, KK).to(out_dt)
    if mutant == "tail_nonzero":
        cols[:, KK:] = 1
    return cols


def col2im_ref(dcols, nB, H, W, Cin, k, stride, pad, mutant=None):
    """-> (dsrc fp64 [nB H W, Cin], abs_sum): every column of a live tap is added to the source position it was read from"""
    pos, live = _taps(nB, H, W, k, stride, pad, mutant)
    v = dcols[:, :k * k * Cin].double().reshape(-1, Cin) * live.reshape(-1, 1)
    z = torch.zeros((nB * H * W, Cin), dtype=torch.float64)
    return z.clone().index_add_(0, pos.reshape(-1), v), z.clone().index_add_(0, pos.reshape(-1), v.abs())


def col2im_terms(k, stride):
    return math.ceil(k / stride) ** 2


def dwconv3x3_ref(x, w, nB, H, W, flip=False, mutant=None):
    """-> (y fp64 [nB H W, C], abs_sum).  Mutants: the three of _taps, noflip, strip_dropped (the last W % 4 columns are not written)"""
    C = x.shape[1]
    x64, w64 = x.double(), w.double().view(C, 9)
    pos, live = _taps(nB, H, W, 3, 1, 1, mutant)
    pos, live = pos.reshape(-1, 9), live.reshape(-1, 9)
    y = torch.zeros((nB * H * W, C), dtype=torch.float64)
    ab = torch.zeros_like(y)
    for t in range(9):
        ts = 8 - t if (flip and mutant != "noflip") else t
        term = x64[pos[:, t]] * w64[:, ts] * live[:, t, None]
        y += term
        ab += term.abs()
    if mutant == "strip_dropped" and W % 4:
        y.view(nB, H, W, C)[:, :, W - W % 4:] = 0
    return y, ab


def dwconv3x3_wgrad_ref(x, dy, nB, H, W, mutant=None, lanes=1):
    """-> (dw fp64 [C, 9], abs_sum).  Mutants: those of _taps, strip_dropped, lane_dropped (the positions of the last of `lanes`
    position lanes are left out)"""
    C = x.shape[1]
    x64, g64 = x.double(), dy.double().clone()
    if mutant == "strip_dropped" and W % 4:
        g64.view(nB, H, W, C)[:, :, W - W % 4:] = 0
    if mutant == "lane_dropped" and lanes > 1:
        g64[lanes - 1::lanes] = 0
    pos, live = _taps(nB, H, W, 3, 1, 1, mutant)
    pos, live = pos.reshape(-1, 9), live.reshape(-1, 9)
    dw = torch.zeros((C, 9), dtype=torch.float64)
    ab = torch.zeros_like(dw)
    for t in range(9):
        term = g64 * x64[pos[:, t]] * live[:, t, None]
        dw[:, t] = term.sum(0)
        ab[:, t] = term.abs().sum(0)
    return dw, ab


def col_sums2_ref(a, b, mutant=None, lanes=1):
    """-> (fp64 [2, C]: sum a, sum a b;  abs_sum [2, C])"""
    a64, b64 = a.double().clone(), b.double()
    if mutant == "lane_dropped" and lanes > 1:
        a64[lanes - 1::lanes] = 0
    p = a64 * b64
    return torch.stack([a64.sum(0), p.sum(0)]), torch.stack([a64.abs().sum(0), p.abs().sum(0)])


def col_affine2_ref(x1, a1, a3, x2=None, a2=None, act=0, mutant=None):
    """-> (y fp64, v = the fp64 pre-activation a1 x1 + a3, mag = |a1 x1| + |a3| (+ |a2 x2| for act 0))"""
    p1 = a1.double() * x1.double()
    v = p1 + a3.double()
    mag = p1.abs() + a3.double().abs()
    if act == 0:
        if x2 is not None:
            p2 = a2.double() * x2.double()
            v, mag = v + p2, mag + p2.abs()
        return v, v, mag
    if act == 1:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0))), v, mag
    if act == 2:
        cdf, pdf = 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))), torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
        return x2.double() * (cdf + v * pdf), v, mag
    if act == 3:
        return v.clamp_min(0.0), v, mag
    gate = (v >= 0) if mutant == "gate_ge" else (v > 0)
    return torch.where(gate, x2.double(), torch.zeros_like(v)), v, mag


def _f32(v):
    """a Python float as the kernel receives it"""
    return float(torch.tensor(v, dtype=torch.float32))


def bn_fwd_coeffs_ref(sums, n, gamma, beta, eps, momentum, rm=None, rv=None, mutant=None):
    """fp64 from the fp32 sums the kernel is fed -> dict(coef [4, C] = (a, shift, mean, rstd), cond, rm, rv, rm_terms)"""
    s, g, bt, n, eps, m = sums.double(), gamma.double(), beta.double(), float(n), _f32(eps), _f32(momentum)
    mean, ex2 = s[0] / n, s[1] / n
    var = (ex2 - mean * mean).clamp_min(0.0)
    rstd = (var + eps) ** -0.5
    a = g * rstd
    out = dict(coef=torch.stack([a, bt - mean * a, mean, rstd]), cond=1.0 + (ex2 + mean * mean) / (var + eps))
    if rm is not None:
        unbias = 1.0 if mutant == "biased_var" else n / (n - 1.0)
        out["rm"] = (1.0 - m) * rm.double() + m * mean
        out["rm_terms"] = ((1.0 - m) * rm.double()).abs() + (m * mean).abs()
        out["rv"] = (1.0 - m) * rv.double() + m * var * unbias
    return out


def bn_fwd_bounds(ref, gamma, beta):
    """[4, C] absolute bounds on (a, shift, mean, rstd): rstd has the relative error E = 8 u cond (division, square, subtraction
    of s2/n and mean^2, the addition of eps, rsqrt to one ulp); a = gamma rstd adds one rounding; mean = s1 / n is one rounding;
    shift = beta - mean a: the product carries E plus three roundings, the subtraction one more on each side"""
    a, shift, mean, rstd = ref["coef"]
    E = 8 * U * ref["cond"]
    ma = (mean * a).abs()
    return torch.stack([(E + 2 * U) * a.abs(), (E + 4 * U) * ma + 2 * U * (beta.double().abs() + ma), 2 * U * mean.abs(), E * rstd])


def bn_eval_coeffs_ref(rm, rv, gamma, beta, eps):
    rstd = (rv.double() + _f32(eps)) ** -0.5
    a = gamma.double() * rstd
    return torch.stack([a, beta.double() - rm.double() * a, rm.double(), rstd])


def bn_eval_bounds(ref, beta):
    a, shift, mean, rstd = ref
    ma = (mean * a).abs()
    return torch.stack([10 * U * a.abs(), 12 * U * ma + 2 * U * (beta.double().abs() + ma), 0 * mean, 8 * U * rstd])


def bn_bwd_local_ref(sums, coef):
    """-> (red fp64 [2, C], bound): red[0] = sums[0] exactly; red[1] = rstd (s1 - mean s0): 4 u rstd (|s1| + |mean s0|)"""
    s, c = sums.double(), coef.double()
    red = torch.stack([s[0], c[3] * (s[1] - c[2] * s[0])])
    return red, torch.stack([0 * s[0], 4 * U * c[3].abs() * (s[1].abs() + (c[2] * s[0]).abs())])


def bn_bwd_coeffs_ref(red, n, gamma, coef):
    """-> (abc fp64 [3, C], bound): A = g rstd (2 u); B = -g rstd^2 m2 (four operations: 6 u);
    C = -g rstd m1 - B mean: 8 u (|g rstd m1| + |B mean|).  red = None: B = C = 0 exactly"""
    c, g = coef.double(), gamma.double()
    mean, rstd = c[2], c[3]
    m1 = red.double()[0] / float(n) if red is not None else torch.zeros_like(mean)
    m2 = red.double()[1] / float(n) if red is not None else torch.zeros_like(mean)
    A, B = g * rstd, -g * rstd * rstd * m2
    t1 = g * rstd * m1
    return torch.stack([A, B, -t1 - B * mean]), torch.stack([2 * U * A.abs(), 6 * U * B.abs(), 8 * U * (t1.abs() + (B * mean).abs())])


def pad_crop_ref(src, nB, Hs, Ws, Hd, Wd, mutant=None):
    """a copy in the source dtype.  Mutants: hw_swap, border_kept (the first padding row repeats the last source row)"""
    ar = torch.arange
    y, x = ar(Hd).view(1, Hd, 1), ar(Wd).view(1, 1, Wd)
    live = ((y <= Hs) if mutant == "border_kept" else (y < Hs)) & (x < Ws)
    rs = Hs if mutant == "hw_swap" else Ws
    pos = (ar(nB).view(nB, 1, 1) * (Hs * Ws) + y.clamp(max=Hs - 1) * rs + x.clamp(max=Ws - 1)).clamp(max=nB * Hs * Ws - 1)
    pos, live = torch.broadcast_tensors(pos, live)
    vals = src[pos.reshape(-1)]
    return torch.where(live.reshape(-1, 1), vals, torch.zeros_like(vals))


# ---- launch rules restated (conv.hip: chan_block, the strip block, reduce_blocks through esvit_query) --------------------------------
def uses_strip(dt, C, off):
    return dt == torch.bfloat16 and C % 8 == 0 and C // 8 <= 256 and off == 0


def chan_lanes(C):
    return 1 if C // 4 > 256 else max(256 // (C // 4), 1)


def strip_lanes(C):
    return max(256 // (C // 8), 1)


def reduce_chain(kind, dt, C, nblk, rows=None, geo=None, off=0):
    """-> (L, PY): the longest chain of additions behind one output of a reduction launched on nblk workgroups -- the terms a
    thread adds in its loop, then the PY position lanes folded in LDS, then the nblk partial blocks; any summation order of
    esvit_partial_reduce is at most that long"""
    if kind == "wgrad":
        nB, H, W = geo
        if uses_strip(dt, C, off):
            PY = strip_lanes(C)
            return 4 * math.ceil(nB * H * math.ceil(W / 4) / (nblk * PY)) + PY + nblk, PY
        rows = nB * H * W
    PY = chan_lanes(C)
    return math.ceil(rows / (nblk * PY)) + PY + nblk, PY


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 counts as 0, x / 0 as inf): <= 1 passes"""
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), "non-finite output"
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def elem_bound(dt, fp32_bound, ref):
    return fp32_bound + (BF * ref.abs() if dt == torch.bfloat16 else 0.0)


def gate_check(got, ref_v, mag, x2):
    """act 4 -> (number of decided elements that are wrong, share of elements inside the band).  An element with mag == 0 is
    computed without rounding and belongs to the decided ones."""
    decided = (ref_v.abs() > 4 * U * mag) | (mag == 0)
    want = torch.where(ref_v > 0, x2.double(), torch.zeros_like(ref_v))
    g = got.detach().cpu().double()
    wrong = int((decided & (g != want)).sum())
    either = (~decided) & (g != 0) & (g != x2.double())
    return wrong + int(either.sum()), float((~decided).double().mean())


# ---- the case table ----------------------------------------------------------------------------------------------------------------
def _c(name, serves, **kw):
    kw.setdefault("off", 0)
    kw.setdefault("dts", DTYPES)
    kw.setdefault("big", False)     # crosses a launch cap, so some workgroup takes its grid-stride loop twice
    kw.setdefault("huge", False)    # 17M elements: on the device only
    return dict(name=name, serves=serves, **kw)


BF_ONLY, F32_ONLY = (torch.bfloat16,), (torch.float32,)

# geo = (nB, H, W, Cin, k, stride, pad); NHWC unless nchw
IM2COL = [
    _c("stem_13x22", "NCHW stem k7 s4 p2 (K = 147 -> 152): nchw_vec / im2col_kernel<float>; non-square", nchw=True, geo=(3, 13, 22, 3, 7, 4, 2)),
    _c("stem_22x13", "the same, H > W", nchw=True, geo=(3, 22, 13, 3, 7, 4, 2)),
    _c("vil_k4_9x14", "Vision Longformer stem k4 s4 p0, a grid no multiple of 4", nchw=True, geo=(3, 9, 14, 3, 4, 4, 0)),
    _c("vil_k2_5x9", "ViL merge k2 s2 p0, odd H and W: nhwc_vec", nchw=False, geo=(3, 5, 9, 48, 2, 2, 0)),
    _c("vil_k2_6x4", "k2 s2, even H and W", nchw=False, geo=(2, 6, 4, 8, 2, 2, 0)),
    _c("cvt_5x9_c64", "CvT k3 s2 p1, odd grid, W > H: nhwc_vec", nchw=False, geo=(3, 5, 9, 64, 3, 2, 1)),
    _c("cvt_9x5_c64", "H > W", nchw=False, geo=(3, 9, 5, 64, 3, 2, 1)),
    _c("cvt_6x8_c64", "even H and W at stride 2", nchw=False, geo=(3, 6, 8, 64, 3, 2, 1)),
    _c("cvt_9x5_c3", "Cin = 3 (K = 27 -> 32): im2col_kernel<bf16>, zero tail", nchw=False, geo=(3, 9, 5, 3, 3, 2, 1)),
    _c("cvt_5x9_c12", "Cin = 12 (K = 108 -> 112): im2col_kernel<bf16>, zero tail", nchw=False, geo=(3, 5, 9, 12, 3, 2, 1)),
    _c("cvt_7x6_c192", "24 vectors per tap", nchw=False, geo=(2, 7, 6, 192, 3, 2, 1)),
    _c("cvt_5x9_c64_off", "Cin % 8 == 0 but the source 8 bytes off: im2col_kernel<bf16>", nchw=False, geo=(3, 5, 9, 64, 3, 2, 1), off=OFF),
    _c("cvt_2x1_c8", "a grid smaller than the kernel after padding", nchw=False, geo=(2, 2, 1, 8, 3, 2, 1)),
    _c("cvt_1x2_c8", "H = 1", nchw=False, geo=(2, 1, 2, 8, 3, 2, 1)),
    _c("big_nhwc_vec", "3 * 101 * 99 * 576 / 8 = 2.16M vectors > 8192 * 256", nchw=False, geo=(3, 201, 197, 64, 3, 2, 1), dts=BF_ONLY, big=True, huge=True),
    _c("big_nchw_vec", "3 * 195 * 191 * 152 / 8 = 2.12M vectors > 8192 * 256", nchw=True, geo=(3, 780, 764, 3, 7, 4, 2), dts=BF_ONLY, big=True, huge=True),
    _c("big_elem", "3 * 81 * 79 * 112 = 2.15M elements > 8192 * 256: im2col_kernel<bf16|float>", nchw=False, geo=(3, 161, 157, 12, 3, 2, 1), big=True),
]

COL2IM = [
    _c("vil_k2_5x9", "k2 s2 p0 (one term per element), odd grid: the last row and column get nothing", geo=(3, 5, 9, 48, 2, 2, 0)),
    _c("vil_k2_6x4", "k2 s2, even grid", geo=(2, 6, 4, 8, 2, 2, 0)),
    _c("vil_k4_9x14", "k4 s4 p0", geo=(2, 9, 14, 8, 4, 4, 0)),
    _c("cvt_5x9_c64", "k3 s2 p1 (up to four terms), W > H: col2im_vec", geo=(3, 5, 9, 64, 3, 2, 1)),
    _c("cvt_9x5_c64", "H > W", geo=(3, 9, 5, 64, 3, 2, 1)),
    _c("cvt_6x8_c64", "even H and W", geo=(3, 6, 8, 64, 3, 2, 1)),
    _c("cvt_9x5_c3", "Cin = 3, zero tail ignored: col2im_kernel<bf16>", geo=(3, 9, 5, 3, 3, 2, 1)),
    _c("cvt_5x9_c12", "Cin = 12", geo=(3, 5, 9, 12, 3, 2, 1)),
    _c("cvt_7x6_c192", "24 vectors per position", geo=(2, 7, 6, 192, 3, 2, 1)),
    _c("cvt_5x9_c64_off", "columns 8 bytes off: col2im_kernel<bf16>", geo=(3, 5, 9, 64, 3, 2, 1), off=OFF),
    _c("cvt_2x1_c8", "a grid smaller than the kernel", geo=(2, 2, 1, 8, 3, 2, 1)),
    _c("k3_s1_4x7", "k3 s1 p1: nine terms per element", geo=(2, 4, 7, 8, 3, 1, 1)),
    _c("big_vec", "3 * 301 * 293 * 64 / 8 = 2.12M vectors > 8192 * 256", geo=(3, 301, 293, 64, 2, 2, 0), dts=BF_ONLY, big=True, huge=True),
    _c("big_elem", "3 * 245 * 239 * 12 = 2.11M elements > 8192 * 256: col2im_kernel<bf16|float>", geo=(3, 245, 239, 12, 3, 2, 1), big=True),
]

# geo = (nB, H, W, C)
DWCONV = [
    _c("5x9_c64", "non-square, nB = 3; strip: 8 lanes x 32; W % 4 = 1", geo=(3, 5, 9, 64)),
    _c("9x5_c64", "H > W", geo=(3, 9, 5, 64)),
    _c("5x9_c12", "C % 8 != 0: dwconv3x3_kernel<bf16>", geo=(3, 5, 9, 12)),
    _c("9x5_c4", "one channel lane", geo=(3, 9, 5, 4)),
    _c("3x7_c20", "C = 20; W % 4 = 3", geo=(2, 3, 7, 20)),
    _c("1x8_c8", "H = 1, W = 8", geo=(3, 1, 8, 8)),
    _c("4x1_c8", "W = 1", geo=(2, 4, 1, 8)),
    _c("1x1_c8", "H = W = 1: only the centre tap", geo=(2, 1, 1, 8)),
    _c("3x2_c40", "W = 2; C = 40: 5 strip lanes (PY 51) / 10 channel lanes (PY 25)", geo=(2, 3, 2, 40)),
    _c("2x3_c192", "W = 3; C = 192: 24 strip lanes (PY 10) / 48 channel lanes (PY 5)", geo=(2, 2, 3, 192)),
    _c("3x4_c16", "W = 4: exactly one strip", geo=(2, 3, 4, 16)),
    _c("2x5_c1024", "W = 5; C / 4 = 256: one position lane; strip 128 x 2", geo=(1, 2, 5, 1024)),
    _c("3x7_c2048", "C / 8 = 256: the widest strip launch, one position lane", geo=(1, 3, 7, 2048), dts=BF_ONLY),
    _c("1x3_c12", "W = 3, H = 1 in the per-channel kernel", geo=(2, 1, 3, 12)),
    _c("5x9_c64_off", "x 8 bytes off: dwconv3x3_kernel<bf16> at C % 8 == 0", geo=(3, 5, 9, 64), off=OFF),
    _c("big_strip", "33 * 63 = 2079 strips > 2048 * 1", geo=(1, 33, 250, 2048), dts=BF_ONLY, big=True, huge=True),
    _c("big_pos", "65 * 64 = 4160 positions > 4096 * 1 (bf16: off, so the per-channel kernel)", geo=(1, 65, 64, 1024), off=OFF, big=True),
]

WGRAD = [c for c in DWCONV if not c["big"]] + [
    _c("loop_c192", "3 * 31 * 29 = 2697 positions > 512 * 5 (fp32); bf16: strip, 744 strips", geo=(3, 31, 29, 192)),
    _c("loop_c1024_off", "23 * 23 = 529 positions > 512 * 1: dwconv3x3_wgrad_kernel<bf16|float>", geo=(1, 23, 23, 1024), off=OFF),
    _c("loop_c2048", "3 * 29 * 7 = 609 strips > 512 * 1: dwconv3x3_wgrad_strip_kernel", geo=(3, 29, 25, 2048), dts=BF_ONLY),
]

# (rows, C, same): same = b is a (BatchNorm statistics), else two tensors (its backward)
COL_SUMS = [
    _c("r7_c4", "one channel lane, 64 position lanes, fewer rows than lanes", rows=7, C=4, same=True),
    _c("r45_c12", "C = 12", rows=45, C=12, same=False),
    _c("r135_c64", "3 * 5 * 9 rows", rows=135, C=64, same=True),
    _c("r40_c40", "10 channel lanes: 256 % 10 != 0", rows=40, C=40, same=False),
    _c("r135_c64_off", "both operands 4 elements off", rows=135, C=64, same=False, off=OFF),
    _c("r2697_c192", "rows > 512 * 5: the loop is taken twice", rows=2697, C=192, same=False),
    _c("r529_c1024", "C / 4 = 256, rows > 512", rows=529, C=1024, same=True),
    _c("r40_c2048", "the DINO head's hidden width: col_sums2_wide, two channel tiles", rows=40, C=2048, same=True),
    _c("r600_c2048", "wide, rows > 512: the loop is taken twice", rows=600, C=2048, same=False),
    _c("r40_c4096", "four channel tiles", rows=40, C=4096, same=False),
    _c("r33_c1028", "wide with a partial last tile (257 lanes)", rows=33, C=1028, same=False),
]

AFFINE_SHAPES = [
    _c("r45_c12", "C = 12", rows=45, C=12),
    _c("r77_c40", "C = 40", rows=77, C=40),
    _c("r135_c64_off", "x1 and x2 4 elements off", rows=135, C=64, off=OFF),
    _c("big", "2740 * 768 = 2.10M elements > 8192 * 256", rows=2740, C=768, big=True),
]
AFFINE_ACTS = ("0", "0x2", "1", "2", "3", "4")   # 0: without x2; 0x2: with x2 and a2

# (nB, Hs, Ws, Hd, Wd, C)
PAD_CROP = [
    _c("pad_5x9_to_7x10", "pad both ways, non-square", geo=(3, 5, 9, 7, 10, 8)),
    _c("crop_9x5_to_7x4", "crop both ways", geo=(3, 9, 5, 7, 4, 40)),
    _c("pad_h_crop_w", "pad H, crop W", geo=(2, 3, 7, 5, 4, 16)),
    _c("same", "a plain copy", geo=(2, 4, 3, 4, 3, 8)),
    _c("one_to_3x2", "a 1 x 1 grid padded", geo=(2, 1, 1, 3, 2, 8)),
    _c("big", "3 * 300 * 295 positions: 2.1M (bf16) / 4.2M (fp32) vectors > 8192 * 256", geo=(3, 280, 290, 300, 295, 64), big=True, huge=True),
]

BN_COEF = [
    _c("n392_c40", "392 rows", n=392, C=40),
    _c("n2_c40", "the smallest batch: n / (n - 1) = 2", n=2, C=40),
    _c("n64_c300", "a second workgroup of channels", n=64, C=300),
]
BN_CHAIN = [(r, rows) for r in (0, 4, 16) for rows in (392, 6272)]
BN_CHAIN_C = 64


def cases(table, dt):
    return [c for c in table if dt in c["dts"]]


def ids(table):
    return [c["name"] for c in table]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def im2col_input(case, dt):
    nB, H, W, Cin = case["geo"][:4]
    if case["nchw"]:
        return data(("im2col", case["name"]), (nB, Cin, H, W), torch.float32)
    return data(("im2col", case["name"]), (nB * H * W, Cin), dt)


def col2im_input(case, dt):
    nB, H, W, Cin, k, s, p = case["geo"]
    return data(("col2im", case["name"]), (nB * out_size(H, k, s, p) * out_size(W, k, s, p), kpad(k, Cin)), dt)


def dwconv_input(case, dt):
    """-> (x, w fp32 [C, 9], dy)"""
    nB, H, W, C = case["geo"]
    return (data(("dw_x", case["name"]), (nB * H * W, C), dt), data(("dw_w", case["name"]), (C, 9), torch.float32, 0.3),
            data(("dw_g", case["name"]), (nB * H * W, C), dt))


def col_sums_input(case, dt):
    a = data(("cs_a", case["name"]), (case["rows"], case["C"]), dt, 1.0, 0.25)
    return a, (a if case["same"] else data(("cs_b", case["name"]), (case["rows"], case["C"]), dt))


def affine_input(case, dt):
    """-> (x1, x2, a1, a2, a3).  Channel 0 has a3 = 0 and one x1 in eight is 0 there: a pre-activation that is exactly zero, which
    `> 0` gates to 0 and `>= 0` would let through"""
    rows, C = case["rows"], case["C"]
    x1 = data(("af_x1", case["name"]), (rows, C), dt)
    x1[::8, 0] = 0
    x2 = data(("af_x2", case["name"]), (rows, C), dt)
    a1 = data(("af_a1", case["name"]), (C,), torch.float32, 0.2, 1.0)
    a2 = data(("af_a2", case["name"]), (C,), torch.float32, 0.5)
    a3 = data(("af_a3", case["name"]), (C,), torch.float32, 0.5)
    a3[0] = 0
    return x1, x2, a1, a2, a3


def pad_crop_input(case, dt):
    nB, Hs, Ws, _, _, C = case["geo"]
    return data(("pc", case["name"]), (nB * Hs * Ws, C), dt)


def bn_coef_input(case):
    """fp32 sums of a well-conditioned batch (|mean| <= std, so the 4 u of the running statistics is not spent on the cancellation
    the rstd bound is about), with channel 0 constant (var = 0 exactly) and channel 1 with s2 / n clearly below mean^2 (var clamps)
    -> dict(sums, n, gamma, beta, rm, rv, plus sums_dy for the backward coefficients)"""
    n, C = case["n"], case["C"]
    g = _gen("bn_coef", case["name"])
    if n == 2:
        c, d = 0.25 * torch.randn(C, generator=g), 1.0 + torch.rand(C, generator=g)
        x = torch.stack([c + d, c - d]).double()
    else:
        x = (torch.randn(n, C, generator=g) + 0.5 * torch.randn(C, generator=g)).double()
    x[:, 0] = 0.5
    dy = torch.randn(n, C, generator=g).double()
    sums = torch.stack([x.sum(0), (x * x).sum(0)])
    sums[1, 1] = n * (sums[0, 1] / n) ** 2 * (1 - 1e-3)
    return dict(sums=sums.float().contiguous(), n=n, gamma=(1 + 0.1 * torch.randn(C, generator=g)).float(), beta=(0.1 * torch.randn(C, generator=g)).float(),
                rm=(0.2 * torch.randn(C, generator=g)).float(), rv=(0.5 + torch.rand(C, generator=g)).float(),
                sums_dy=torch.stack([dy.sum(0), (dy * x).sum(0)]).float().contiguous())


def bn_offset_sums(C=40, n=392):
    """fp32 sums of channels whose mean / std runs from 0 to 16: the cancellation the rstd bound allows for (no running statistics)"""
    g = _gen("bn_offset", C, n)
    r = torch.linspace(0, 16, C).double()
    z = torch.randn(n, C, generator=g).double()
    x = (z - z.mean(0)) / z.std(0, unbiased=False) + r
    return torch.stack([x.sum(0), (x * x).sum(0)]).float().contiguous(), r


def bn_chain_input(r, rows, dt, C=BN_CHAIN_C):
    """rows x C with sample mean r and sample std 1 per channel before it is stored as dt"""
    z = torch.randn(rows, C, generator=_gen("bn_chain", r, rows)).double()
    z = (z - z.mean(0)) / z.std(0, unbiased=False)
    return (z + r).to(dt)


def bn_chain_ref(x, gamma, beta, eps=BN_EPS):
    """fp64 batch norm of the input as stored -> (y, mean, rstd)"""
    x64 = x.double()
    mean, var = x64.mean(0), x64.var(0, unbiased=False)
    rstd = (var + _f32(eps)) ** -0.5
    return (x64 - mean) * rstd * gamma.double() + beta.double(), mean, rstd


def bn_chain_y_bound(x, gamma, beta, r, mean, rstd, dt):
    """y = a x + shift with a = gamma rstd (1 + E'), E' = 8 (1 + r^2) u + 2 u: both products carry E' and the roundings of the
    shift (bn_fwd_bounds) and of the affine pass (4 u); the mean inside the shift carries the error of the column sum it came
    from, (L + 1) u mean|x| with L the chain of that launch"""
    E = 8 * (1 + r * r) * U + 8 * U
    a = (gamma.double() * rstd).abs()
    rows, C = x.shape
    L, _ = reduce_chain("col_sums2", dt, C, _reduce_blocks(rows), rows=rows)
    dmean = (L + 1) * U * x.double().abs().mean(0)
    ref = bn_chain_ref(x, gamma, beta)[0]
    return elem_bound(dt, E * a * (x.double().abs() + mean.abs()) + a * dmean + 4 * U * beta.double().abs(), ref)


def fp32_formula_rstd(x, eps=BN_EPS):
    """the kernels' formula (sum, sum of squares, E[x^2] - mean^2) in fp32 torch on the CPU"""
    xf = x.float()
    n = float(xf.shape[0])
    mean = xf.sum(0) / n
    var = ((xf * xf).sum(0) / n - mean * mean).clamp_min(0.0)
    return torch.rsqrt(var + eps)


def torch_bn_rstd(x, eps=BN_EPS):
    """save_invstd of torch's own fp32 batch norm on the CPU"""
    xf = x.float()
    C = xf.shape[1]
    return torch.native_batch_norm(xf, torch.ones(C), torch.zeros(C), None, None, True, BN_MOMENTUM, eps)[2]


def gelu_allowance(x1, a1, a3, x2, act, ref):
    """acts 1, 2: max(3 x the worst error of fp32 torch on the same (exactly representable) inputs, 16 u max|ref|)"""
    from oracle import ops_ref
    got = ops_ref.col_affine2(x1.float(), a1, a3, None if x2 is None else x2.float(), None, act=act)
    return max(3.0 * float((got.double() - ref).abs().max()), 16 * U * float(ref.abs().max()))


# ---- DINOHead(use_bn=True) at the reference's default width ------------------------------------------------------------------------
HEAD = dict(in_dim=48, hidden_dim=2048, bottleneck_dim=32, out_dim=96, rows=40)


def head_case():
    """-> (state dict of esvit_amd.DINOHead(48, 96, use_bn=True, bottleneck_dim=32) at hidden 2048, x [40, 48], probe [40, 96])"""
    import esvit_amd
    torch.manual_seed(2048)
    head = esvit_amd.DINOHead(HEAD["in_dim"], HEAD["out_dim"], use_bn=True, hidden_dim=HEAD["hidden_dim"], bottleneck_dim=HEAD["bottleneck_dim"])
    g = _gen("head2048")
    sd = head.state_dict()
    for n in ("mlp.1", "mlp.4"):   # BatchNorm away from its (1, 0) initialisation
        sd[n + ".weight"].copy_(1 + 0.1 * torch.randn(HEAD["hidden_dim"], generator=g))
        sd[n + ".bias"].copy_(0.1 * torch.randn(HEAD["hidden_dim"], generator=g))
    return {k: v.clone() for k, v in sd.items()}, torch.randn(HEAD["rows"], HEAD["in_dim"], generator=g), torch.randn(HEAD["rows"], HEAD["out_dim"], generator=g)


def head_ref(sd, x, probe):
    """fp64 autograd of the torch modules the head is made of -> dict(logits, dx, grads {name: tensor}, buffers {name: tensor})"""
    import copy
    import esvit_amd
    F = torch.nn.functional
    head = esvit_amd.DINOHead(HEAD["in_dim"], HEAD["out_dim"], use_bn=True, hidden_dim=HEAD["hidden_dim"], bottleneck_dim=HEAD["bottleneck_dim"])
    head.load_state_dict(copy.deepcopy(sd))
    head = head.double().train()
    x64 = x.double().requires_grad_(True)
    z = F.normalize(head.mlp(x64), dim=-1, p=2)
    v, g = head.last_layer.weight_v, head.last_layer.weight_g
    logits = z @ (g * v / v.norm(dim=1, keepdim=True)).t()
    (logits * probe.double()).sum().backward()
    return dict(logits=logits.detach(), dx=x64.grad, grads={n: p.grad for n, p in head.named_parameters() if p.grad is not None},
                buffers={n: b.detach().clone() for n, b in head.named_buffers()})


# ---- drivers shared by the CPU run (oracle/ops_ref.py, fp32 / bf16 torch) and the GPU run (esvit_amd.ops, the kernels) -----------------
# Each returns {metric: value}; check() asserts them: "equal*" == 1, "ratio*" <= 1 (err / bound), "wrong*" == 0,
# "band_share" <= 1e-3, "info_*" is recorded only.
def _reduce_blocks(rows):
    from esvit_amd import ops
    return ops.query(ops.Q_COL_REDUCE_BLOCKS, rows)


def run_im2col(o, dev, case, dt):
    nB, H, W, Cin, k, s, p = case["geo"]
    src = im2col_input(case, dt)
    got = o.conv_im2col(place(src, dev, case["off"]), case["nchw"], nB, H, W, Cin, k, s, p, dtype=dt)
    return dict(equal=float(torch.equal(got.cpu(), im2col_ref(src, case["nchw"], nB, H, W, Cin, k, s, p, dt))))


def run_col2im(o, dev, case, dt):
    nB, H, W, Cin, k, s, p = case["geo"]
    dcols = col2im_input(case, dt)
    got = o.conv_col2im(place(dcols, dev, case["off"]), nB, H, W, Cin, k, s, p)
    ref, ab = col2im_ref(dcols, nB, H, W, Cin, k, s, p)
    return dict(ratio=ratio(got, ref, col2im_terms(k, s) * U * ab), equal_fp32_out=float(got.dtype == torch.float32))


def run_dwconv(o, dev, case, dt, flip):
    nB, H, W, C = case["geo"]
    x, w, _ = dwconv_input(case, dt)
    got = o.dwconv3x3(place(x, dev, case["off"]), w.to(dev), nB, H, W, flip=flip)
    ref, ab = dwconv3x3_ref(x, w, nB, H, W, flip=flip)
    return dict(ratio=ratio(got, ref, elem_bound(dt, 10 * U * ab, ref)), equal_dtype=float(got.dtype == dt))


def run_wgrad(o, dev, case, dt):
    nB, H, W, C = case["geo"]
    x, _, dy = dwconv_input(case, dt)
    xd, gd = place(x, dev, case["off"]), place(dy, dev, case["off"])
    got = o.dwconv3x3_wgrad(xd, gd, nB, H, W).clone()
    again = o.dwconv3x3_wgrad(xd, gd, nB, H, W)
    ref, ab = dwconv3x3_wgrad_ref(x, dy, nB, H, W)
    L, _ = reduce_chain("wgrad", dt, C, _reduce_blocks(nB * H * W), geo=(nB, H, W), off=case["off"])
    return dict(ratio=ratio(got, ref, (L + 1) * U * ab), equal_repeat=float(torch.equal(got, again)), info_L=float(L))


def run_col_sums(o, dev, case, dt):
    a, b = col_sums_input(case, dt)
    ad = place(a, dev, case["off"])
    bd = ad if case["same"] else place(b, dev, case["off"])
    got = o.col_sums2(ad, bd).clone()
    again = o.col_sums2(ad, bd)
    ref, ab = col_sums2_ref(a, b)
    L, _ = reduce_chain("col_sums2", dt, case["C"], _reduce_blocks(case["rows"]), rows=case["rows"])
    return dict(ratio=ratio(got, ref, (L + 1) * U * ab), equal_repeat=float(torch.equal(got, again)), info_L=float(L))


def run_affine(o, dev, case, dt, act):
    x1, x2, a1, a2, a3 = affine_input(case, dt)
    code = int(act[0])
    use_x2 = act in ("0x2", "2", "4")
    x1d, x2d = place(x1, dev, case["off"]), (place(x2, dev, case["off"]) if use_x2 else None)
    got = o.col_affine2(x1d, a1.to(dev), a3.to(dev), x2d, a2.to(dev) if act == "0x2" else None, act=code)
    ref, v, mag = col_affine2_ref(x1, a1, a3, x2 if use_x2 else None, a2 if act == "0x2" else None, act=code)
    if code == 4:
        wrong, share = gate_check(got, v, mag, x2)
        return dict(wrong=float(wrong), band_share=share)
    if code in (1, 2):
        allow = gelu_allowance(x1, a1, a3, x2 if use_x2 else None, code, ref)
        return dict(ratio=ratio(got, ref, elem_bound(dt, allow, ref)), info_allowance=allow)
    return dict(ratio=ratio(got, ref, elem_bound(dt, 4 * U * mag, ref)))


def run_bn_coef(o, dev, case):
    """the four coefficient kernels on fp32 sums: forward with the running statistics, eval, backward local, backward (red and None)"""
    c = bn_coef_input(case)
    d = lambda t: t.to(dev)  # noqa: E731
    rm, rv = d(c["rm"].clone()), d(c["rv"].clone())
    coef = o.bn_fwd_coeffs(d(c["sums"]), c["n"], d(c["gamma"]), d(c["beta"]), BN_EPS, BN_MOMENTUM, rm, rv)
    ref = bn_fwd_coeffs_ref(c["sums"], c["n"], c["gamma"], c["beta"], BN_EPS, BN_MOMENTUM, c["rm"], c["rv"])
    bd = bn_fwd_bounds(ref, c["gamma"], c["beta"])
    m = {"ratio_" + n: ratio(coef[i], ref["coef"][i], bd[i]) for i, n in enumerate(("a", "shift", "mean", "rstd"))}
    m["ratio_running_mean"] = ratio(rm, ref["rm"], 4 * U * ref["rm_terms"])
    m["ratio_running_var"] = ratio(rv, ref["rv"], 4 * U * ref["rv"].abs())
    m["ratio_const_rstd"] = ratio(coef[3, :2], torch.full((2,), _f32(BN_EPS) ** -0.5, dtype=torch.float64), 4 * U * _f32(BN_EPS) ** -0.5)
    ev = o.bn_eval_coeffs(d(c["rm"]), d(c["rv"]), d(c["gamma"]), d(c["beta"]), BN_EPS)
    evr = bn_eval_coeffs_ref(c["rm"], c["rv"], c["gamma"], c["beta"], BN_EPS)
    evb = bn_eval_bounds(evr, c["beta"])
    m["ratio_eval"] = max(ratio(ev[i], evr[i], evb[i]) for i in range(4))
    coef_cpu = coef.cpu()
    red = o.bn_bwd_local(d(c["sums_dy"]), coef)
    redr, redb = bn_bwd_local_ref(c["sums_dy"], coef_cpu)
    m["ratio_bwd_local"] = max(ratio(red[i], redr[i], redb[i]) for i in range(2))
    red_cpu = red.cpu()
    abc = o.bn_bwd_coeffs(red, c["n"], d(c["gamma"]), coef)
    abcr, abcb = bn_bwd_coeffs_ref(red_cpu, c["n"], c["gamma"], coef_cpu)
    m["ratio_bwd_coeffs"] = max(ratio(abc[i], abcr[i], abcb[i]) for i in range(3))
    fixed = o.bn_bwd_coeffs(None, c["n"], d(c["gamma"]), coef).cpu()
    fr, fb = bn_bwd_coeffs_ref(None, c["n"], c["gamma"], coef_cpu)
    m["ratio_bwd_fixed_A"] = ratio(fixed[0], fr[0], fb[0])
    m["equal_bwd_fixed_BC_zero"] = float(bool((fixed[1:] == 0).all()))
    return m


def run_bn_offset(o, dev):
    """mean / std from 0 to 16 per channel, no running statistics: the rstd bound with its conditioning term"""
    sums, r = bn_offset_sums()
    C = sums.shape[1]
    gamma, beta = data(("bn_off_g",), (C,), torch.float32, 0.1, 1.0), data(("bn_off_b",), (C,), torch.float32, 0.1)
    coef = o.bn_fwd_coeffs(sums.to(dev), 392, gamma.to(dev), beta.to(dev), BN_EPS, BN_MOMENTUM)
    ref = bn_fwd_coeffs_ref(sums, 392, gamma, beta, BN_EPS, BN_MOMENTUM)
    bd = bn_fwd_bounds(ref, gamma, beta)
    return {"ratio_" + n: ratio(coef[i], ref["coef"][i], bd[i]) for i, n in enumerate(("a", "shift", "mean", "rstd"))}


def run_bn_chain(o, dev, r, rows, dt):
    """col_sums2 -> bn_fwd_coeffs -> col_affine2 against the fp64 batch norm of the input"""
    x = bn_chain_input(r, rows, dt)
    C = x.shape[1]
    gamma, beta = data(("bn_chain_g",), (C,), torch.float32, 0.1, 1.0), data(("bn_chain_b",), (C,), torch.float32, 0.1)
    xd = x.to(dev)
    coef = o.bn_fwd_coeffs(o.col_sums2(xd, xd), rows, gamma.to(dev), beta.to(dev), BN_EPS, BN_MOMENTUM)
    y = o.col_affine2(xd, coef[0].contiguous(), coef[1].contiguous())
    yr, mean, rstd = bn_chain_ref(x, gamma, beta)
    rel = lambda g: float(((g.detach().cpu().double() - rstd).abs() / rstd).max())  # noqa: E731
    lim = 8 * (1 + r * r) * U
    return dict(ratio_rstd=rel(coef[3]) / lim, ratio_y=ratio(y, yr, bn_chain_y_bound(x, gamma, beta, r, mean, rstd, dt)),
                info_rstd_rel=rel(coef[3]), info_torch_bn_rstd_rel=rel(torch_bn_rstd(x)), info_fp32_formula_rstd_rel=rel(fp32_formula_rstd(x)))


def run_pad_crop(o, dev, case, dt):
    nB, Hs, Ws, Hd, Wd, C = case["geo"]
    src = pad_crop_input(case, dt)
    got = o.pad_crop_tokens(src.to(dev), nB, Hs, Ws, Hd, Wd)
    return dict(equal=float(torch.equal(got.cpu(), pad_crop_ref(src, nB, Hs, Ws, Hd, Wd))))


def failures(metrics):
    bad = []
    for k, v in metrics.items():
        ok = (v == 1.0 if k.startswith("equal") else v <= 1.0 if k.startswith("ratio") else v == 0.0 if k.startswith("wrong")
              else v <= 1e-3 if k == "band_share" else True)
        if not ok:
            bad.append("%s = %.4g" % (k, v))
    return bad


def check(entry, case, dt, metrics, record=None, where="cpu"):
    """print (and record) every figure, then assert"""
    tag = dict(test="conv", entry=entry, case=case, dtype=dt_name(dt) if dt is not None else "fp32", where=where)
    if record is not None:
        record(**tag, **metrics)
    print("OBSERVED", tag, metrics)
    bad = failures(metrics)
    assert not bad, (entry, case, tag["dtype"], bad)
