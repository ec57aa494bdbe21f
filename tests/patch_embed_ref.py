"""fp64 statement of the fused patch embedding (esvit_amd/csrc/patch_embed.hip behind ops.patch_embed_fwd / patch_embed_bwd /
patch_embed_reduce) that tests/test_patch_embed_{cpu,gpu}.py compare against.  Plain index arithmetic in float64; nothing of
oracle/ops_ref.py or of the library is called.

  forward    cols[r, c*16 + ph*4 + pw] = bf16(img[b, c, 4 ty + ph, 4 tx + pw]),  r = row0(crop) + (b * H/4 + ty) * W/4 + tx
             y = cols W^T + bias;  mean = sum_e y / E;  rstd = (sum_e (y - mean)^2 / E + eps)^-1/2;  x = (y - mean) rstd gamma + beta
  backward   (mean, rstd given, as the kernel takes them)  xh = (y - mean) rstd;  gd = gx gamma;  s1 = sum_e gd / E;  s2 = sum_e gd xh / E
             dya = bf16((gd - s1 - xh s2) rstd);  dW = dya^T cols;  dbp = sum_r dya;  dgamma = sum_r gx xh;  dbeta = sum_r gx
The two bf16 rounding points are the pixels and dya.  `dtype=torch.float32` runs the same lines in fp32 (the restatement whose error sets
the bounds, below); the mutants are what the CPU test must see caught.

Bound of every output, the rule of tests/gemm_ref.py for activation epilogues (the device's rsqrtf and division are not correctly rounded
and their error cannot be derived here, so it is measured on the restatement, never on the kernel):
    |got - ref| <= max(3 x the worst error of the fp32 restatement of the same formula against fp64 over the output, 16 u max|ref|)
On inexact inputs dW and dbp also get dya_flip_allowance (a bf16 rounding of dya that falls the other way).  The floor is 2^-100.
"""
import torch

K = 48
FLOOR = 2.0 ** -100
U = 2.0 ** -24


def bf16_round(t):
    """round to nearest even bf16, kept in t's dtype (the inputs are fp32 values, so the fp32 step in between is exact)"""
    return t.float().bfloat16().to(t.dtype)


def rows_of(imgs):
    return [im.shape[0] * (im.shape[2] // 4) * (im.shape[3] // 4) for im in imgs]


def cols_of(imgs, dtype=torch.float64, order="cphpw"):
    """[sum rows, 48] columns of all crops; order: the column order ("cphpw" is the kernel's; "phpwc" the mutant)"""
    out = []
    for im in imgs:
        nB, ch, H, W = im.shape
        assert ch == 3 and H % 4 == 0 and W % 4 == 0
        v = im.to(dtype).reshape(nB, 3, H // 4, 4, W // 4, 4)  # b c ty ph tx pw
        v = v.permute(0, 2, 4, 1, 3, 5) if order == "cphpw" else v.permute(0, 2, 4, 3, 5, 1)  # b ty tx (c ph pw | ph pw c)
        out.append(v.reshape(nB * (H // 4) * (W // 4), K))
    return bf16_round(torch.cat(out))


def forward(imgs, W, bias, gamma, beta, eps, dtype=torch.float64, order="cphpw", drop_bias=False):
    """-> (x, mean, rstd, y).  W: the bf16 weight [E, 48] (any dtype holding bf16 values)"""
    cols = cols_of(imgs, dtype, order)
    y = cols @ W.to(dtype).t()
    if not drop_bias:
        y = y + bias.to(dtype)
    E = y.shape[1]
    mean = y.sum(1) / E
    d = y - mean[:, None]
    rstd = ((d * d).sum(1) / E + eps) ** -0.5
    x = d * rstd[:, None] * gamma.to(dtype) + beta.to(dtype)
    return x, mean, rstd, y


def backward(imgs, W, bias, gamma, gx, mean, rstd, dtype=torch.float64, round_dya=True, skip_rows=None):
    """-> (dW [E, 48], dbp, dgamma, dbeta, dL/dy before its rounding).  skip_rows: (r0, r1) rows left out of every sum (the "tile skipped" mutant)"""
    cols = cols_of(imgs, dtype)
    y = cols @ W.to(dtype).t() + bias.to(dtype)
    E = y.shape[1]
    gx = gx.to(dtype)
    xh = (y - mean.to(dtype)[:, None]) * rstd.to(dtype)[:, None]
    gd = gx * gamma.to(dtype)
    s1 = gd.sum(1, keepdim=True) / E
    s2 = (gd * xh).sum(1, keepdim=True) / E
    dy = (gd - s1 - xh * s2) * rstd.to(dtype)[:, None]
    dya = bf16_round(dy) if round_dya else dy
    keep = torch.ones(y.shape[0], dtype=dtype)
    if skip_rows is not None:
        keep[skip_rows[0]:skip_rows[1]] = 0
    k = keep[:, None]
    return (dya * k).t() @ cols, (dya * k).sum(0), (gx * xh * k).sum(0), (gx * k).sum(0), dy


def bound(ref64, restated32):
    """scalar bound of an output: max(3 x the worst error of the fp32 restatement in it, 16 u max|ref|), u = 2^-24"""
    return max(3.0 * float((restated32.double() - ref64).abs().max()), 16 * U * float(ref64.abs().max()), FLOOR)


def dya_flip_allowance(dy64, dy32, cols):
    """What the bf16 rounding of dya adds to the bounds of dW and dbp on inexact inputs: an element of dL/dy that lies within its own fp32
    error e = bound(dL/dy) of a rounding boundary (the midpoint of two neighbouring bf16 values) may round the other way than the statement's, which moves
    dya by one bf16 spacing.  -> (allowance of dW [E, 48], of dbp [E])"""
    e = bound(dy64, dy32)
    _, ex = torch.frexp(dy64.abs().clamp_min(2.0 ** -120))
    ulp = torch.ldexp(torch.ones_like(dy64), ex - 8)  # bf16 spacing at |dy|: 8 significant bits
    frac = (dy64.abs() / ulp) % 1.0
    near = ((frac - 0.5).abs() * ulp <= e).to(dy64.dtype) * ulp
    return near.t() @ cols.abs(), near.sum(0)


def ratio(got, ref64, bound):
    """largest |got - ref| / bound; an assertion holds when it is <= 1"""
    return float(((got.double().cpu() - ref64).abs() / bound).max())


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def exact_inputs(shapes, E, seed=0, paired=False):
    """pixels i / 4, |i| <= 3; weights j / 2, |j| <= 2; bias in eighths: y is a sum of at most 49 multiples of 1/8 below 37 -- exact in
    fp32 in any order.  paired: channels 2 i and 2 i + 1 share their weight row and bias (y[:, 2i] == y[:, 2i+1]: test_dw_exact)"""
    g = torch.Generator().manual_seed(seed)
    imgs = [torch.randint(-3, 4, s, generator=g).float() / 4 for s in shapes]
    W = torch.randint(-2, 3, (E, K), generator=g).float() / 2
    bias = torch.randint(-8, 9, (E,), generator=g).float() / 8
    if paired:
        W[1::2] = W[0::2]
        bias[1::2] = bias[0::2]
    gamma = 1 + torch.randint(-4, 5, (E,), generator=g).float() / 8
    beta = torch.randint(-8, 9, (E,), generator=g).float() / 8
    return imgs, W, bias, gamma, beta


def gaussian_inputs(shapes, E, seed=0):
    g = torch.Generator().manual_seed(seed)
    imgs = [torch.randn(s, generator=g) for s in shapes]
    W = bf16_round(torch.randn(E, K, generator=g) * 0.1)
    bias = torch.randn(E, generator=g) * 0.1
    gamma = 1 + 0.1 * torch.randn(E, generator=g)
    beta = 0.1 * torch.randn(E, generator=g)
    return imgs, W, bias, gamma, beta


# token counts every supported width is run at (tests/test_patch_embed_gpu.py); the forward's workgroup tile is 64 rows, the backward's 128
SHAPES = {
    "one_8x8": [(1, 3, 8, 8)],                                 # 4 tokens
    "three_20x12": [(3, 3, 20, 12)],                           # 45 tokens: a ragged tile
    "fwd_tile_m1": [(1, 3, 4, 252)], "fwd_tile": [(1, 3, 4, 256)], "fwd_tile_p1": [(1, 3, 4, 260)],     # 63, 64, 65
    "bwd_tile_m1": [(1, 3, 4, 508)], "bwd_tile": [(1, 3, 4, 512)], "bwd_tile_p1": [(1, 3, 4, 516)],     # 127, 128, 129
    "two_res_mid_tile": [(1, 3, 12, 20), (3, 3, 16, 16)],      # 15 + 48 tokens: the second crop tensor starts inside a subtile
    "rect_12x20": [(2, 3, 12, 20)],
    "route_ab": [(2, 3, 32, 32), (3, 3, 16, 16)],              # 128 + 48
    "seventeen_crops": [(1, 3, 8, 4 * (1 + i % 3)) for i in range(17)],  # more crop tensors than one launch takes
}
# the backward's persistent walk (one workgroup per CU, 256 on the MI355X): 768 tiles = 3 per workgroup; 384 tiles = 2 for the first 128
# workgroups and 1 for the rest
WALK_SHAPES = {"walk_3_tiles": [(6, 3, 512, 512)], "walk_uneven": [(3, 3, 512, 512)]}
