"""The fused update (esvit_amd/csrc/update.hip: clip -> AdamW / SGD / LARS -> teacher EMA -> bf16 weight copies) stated in float64, the
builder of the tables and arenas its kernels read, and the comparison that tests/test_update_cpu.py runs on an fp32 emulation and
tests/test_update_gpu.py on the kernels.

The statement is plain arithmetic on float64 tensors.  The kernels receive their scalars as `float`; with fp32_scalars=True (the
default) every one of them -- lr, wd, clip, the betas / momentum / eta, eps, ema_m, the two bias corrections, and the differences the
kernel forms from them in one fp32 operation (1 - b1, 1 - b2, 1 - ema_m, 1 - lr wd) -- enters rounded to fp32, so that what is compared
is the arithmetic on the tensors and not the representation of 0.9.  fp32_scalars=False leaves them as given: that is how the CPU
tests hold the statement against torch.optim and the oracle at 1e-12.

Element bounds (include/esvit_hip.h states them as the contract): |got - want| <= K 2^-24 (sum of the absolute values of the
relation's terms), want evaluated in fp64 from the launch's own fp32 inputs and the DEVICE's statistics.  K counts the fp32
roundings between the inputs and the term that collects most of them, each at most 2^-24 relative (u), to first order, without
counting on any contraction into FMAs (a contraction removes a rounding, never adds one):

  clip factor c = clip / (sqrt(s) + 1e-6)                     sqrt, add, divide                                   3   (0 when c = 1)
  AdamW  m' = m + (1 - b1)(c g - m)                           c 3, c g 1, the difference 1, the product 1, the sum 1           K = 7
         v' = b2 v + (1 - b2)(c g)(c g)                       (c g) 4, twice; two products, the sum                            K = 12
         p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)   from the device's m', v':
                                                              lr / bc1 1, 1 / sqrt(bc2) 2, sqrt(v') 1, their product 1, + eps 1,
                                                              m' / denom 1, the product with lr / bc1 1: 8 on the step term, and
                                                              the final difference.  That difference and the product before it
                                                              are one FMA under the contraction hipcc applies by default, as are
                                                              the product and sum of denom: 7 remain.  Uncontracted, nine worst-
                                                              case roundings of one sign on the step term would exceed this K  K = 8
  SGD    mu' = momentum mu + (c g + wd p)                     c 3, c g 1, inner sum 1, outer sum 1                             K = 6
  LARS   mu' = momentum mu + q (c g + wd p)                   q = eta sqrt(s1) / sqrt(c c s0 + 2 c wd s2 + wd wd s1): sqrt(s1) 1,
                                                              eta 1, the divide 1, the radicand (c c) s0 carries 2 x 3 + 2 and two
                                                              sums: 10 cs, halved by the root, + 1 for the root itself: q costs
                                                              4 + 5 cs where cs = (c c s0 + 2 c wd |s2| + wd wd s1) / radicand is
                                                              1 when g.p is small against |g||p| (cs <= the cond of the q bound);
                                                              then c g 4, inner sum 1, q 9 and its product 1, outer sum 1      K = 16
                                                              (the three roundings of c are counted in q and again in c g, where
                                                              they enter with opposite signs and cancel to the extent that
                                                              c c s0 carries the radicand: at least as much room as cs <= CS_MAX
                                                              = 1.5 takes, which test_update_cpu.py asserts of the test tensors)
  SGD / LARS  p' = p - lr mu'    from the device's mu':       the product and the difference                                   K = 2
  EMA    t' = ema_m t + (1 - ema_m) p'   from the device's p': a product per term and the sum                                   K = 2

Statistic bound (level 1): (32 + chunks_t) u sum|terms|, the sequential bound of the header; the atomic form adds the same chunk
partials in an arbitrary order, which the sequential bound covers.  Factor bounds (level 2): c within ((32 + chunks_t) / 2 + 1) u
relative (half the statistic's, the root), q within ((32 + chunks_t)(1 + cond) / 2 + 8) u relative with
cond = (c^2 sum g^2 + 2 c wd sum|g p| + wd^2 sum p^2) / |c g + wd p|^2: LARS takes |c g + wd p| from three statistics, which cancels
when c g ~ -wd p, where the reference takes the norm of the tensor."""
import math
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
CHUNK = 4096
TFIELDS = 12
MOAT = 32  # sentinel elements in front of, between and behind the regions of an arena (a multiple of 8: 16 bytes in both arenas)
SENTINEL = -3.0e33  # finite, and nothing an update produces; compared by bits
ADAMW, SGD, LARS = 0, 1, 2
RULE_NAMES = {ADAMW: "adamw", SGD: "sgd", LARS: "lars"}
K = {ADAMW: {"m": 7, "v": 12, "p": 8}, SGD: {"mu": 6, "p": 2}, LARS: {"mu": 16, "p": 2}}
K_EMA = 2
COND_MAX = 8.0


# ---- scalars -------------------------------------------------------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


def bits(x):
    return int(np.float32(x).view(np.uint32))


def _r(x, fp32_scalars):
    return f32(x) if fp32_scalars else float(x)


def _one_minus(x, fp32_scalars):
    """1 - x as the kernel forms it: one fp32 subtraction of the fp32 value"""
    return float(np.float32(1.0) - np.float32(x)) if fp32_scalars else 1.0 - float(x)


def _decay(lr, wd, group, fp32_scalars):
    if group != 0:
        return 1.0
    if fp32_scalars:
        return float(np.float32(1.0) - np.float32(np.float32(lr) * np.float32(wd)))
    return 1.0 - float(lr) * float(wd)


def pack_bc(b1, b2, t):
    """slot 8 of the table as esvit_amd.update builds it: bits(1 - b1^t) | bits(1 - b2^t) << 32, as a signed 64-bit value"""
    v = bits(1.0 - b1 ** t) | (bits(1.0 - b2 ** t) << 32)
    return v - (1 << 64) if v >= 1 << 63 else v


def unpack_bc(packed):
    packed = int(packed) & ((1 << 64) - 1)
    lo, hi = np.uint32(packed & 0xffffffff), np.uint32(packed >> 32)
    return float(lo.view(np.float32)), float(hi.view(np.float32))


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def statistics(g, p=None):
    """-> [(sum g^2, sum |g^2|)] and, with p, also (sum p^2, .), (sum g p, sum |g p|): float64 sums of float64 products"""
    g = g.double()
    out = [(float((g * g).sum()), float((g * g).sum()))]
    if p is not None:
        p = p.double()
        out.append((float((p * p).sum()), float((p * p).sum())))
        out.append((float((g * p).sum()), float((g * p).abs().sum())))
    return out


def clip_coef(sum_gg, clip, fp32_scalars=True):
    """utils.clip_gradients for one tensor: min(1, clip / (|g| + 1e-6)); clip == 0 switches clipping off"""
    clip = _r(clip, fp32_scalars)
    if not clip > 0.0:
        return 1.0
    coef = clip / (math.sqrt(float(sum_gg)) + _r(1e-6, fp32_scalars))
    return coef if coef < 1.0 else 1.0


def adamw_moments(g, m, v, c, b1, b2, fp32_scalars=True):
    gc = c * g
    m1 = m + _one_minus(b1, fp32_scalars) * (gc - m)
    v1 = _r(b2, fp32_scalars) * v + _one_minus(b2, fp32_scalars) * gc * gc
    return m1, v1


def adamw_param(p, m1, v1, lr, wd, group, eps, bc1, bc2, fp32_scalars=True):
    lr, eps, bc1, bc2 = (_r(x, fp32_scalars) for x in (lr, eps, bc1, bc2))
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    return p * _decay(lr, wd, group, fp32_scalars) - (lr / bc1) * (m1 / denom)


def adamw(p, g, m, v, c, lr, wd, group, b1, b2, eps, bc1, bc2, fp32_scalars=True):
    """torch.optim.AdamW on the clipped gradient c g -> (p', m', v')"""
    m1, v1 = adamw_moments(g, m, v, c, b1, b2, fp32_scalars)
    return adamw_param(p, m1, v1, lr, wd, group, eps, bc1, bc2, fp32_scalars), m1, v1


def momentum_buffer(p, g, mu, c, q, wd, group, momentum, fp32_scalars=True):
    wdp = _r(wd, fp32_scalars) if group == 0 else 0.0
    return _r(momentum, fp32_scalars) * mu + q * (c * g + wdp * p)


def momentum_param(p, mu1, lr, fp32_scalars=True):
    return p - _r(lr, fp32_scalars) * mu1


def sgd(p, g, mu, c, lr, wd, group, momentum, fp32_scalars=True):
    """torch.optim.SGD(momentum, dampening 0, no nesterov) on c g, weight decay for group 0 -> (p', mu')"""
    mu1 = momentum_buffer(p, g, mu, c, 1.0, wd, group, momentum, fp32_scalars)
    return momentum_param(p, mu1, lr, fp32_scalars), mu1


def lars(p, g, mu, c, q, lr, wd, group, momentum, fp32_scalars=True):
    """utils.LARS.step on c g: dp = q (c g + wd p) for group 0 (ndim != 1), c g otherwise (pass q = 1) -> (p', mu')"""
    mu1 = momentum_buffer(p, g, mu, c, q if group == 0 else 1.0, wd, group, momentum, fp32_scalars)
    return momentum_param(p, mu1, lr, fp32_scalars), mu1


def lars_q(sum_gg, sum_pp, sum_gp, c, wd, eta, group, fp32_scalars=True):
    """the trust ratio eta |p| / |c g + wd p| from the three statistics; 1 for group 1 and where either norm is 0"""
    if group != 0:
        return 1.0
    wd, eta = _r(wd, fp32_scalars), _r(eta, fp32_scalars)
    pn = math.sqrt(float(sum_pp))
    un = math.sqrt(max(c * c * float(sum_gg) + 2.0 * c * wd * float(sum_gp) + wd * wd * float(sum_pp), 0.0))
    return eta * pn / un if (pn > 0.0 and un > 0.0) else 1.0


def lars_cs(sum_gg, sum_pp, sum_gp, c, wd, fp32_scalars=True):
    """the same ratio for the radicand as the kernel forms it from the statistics: |sum g p| in the numerator; 1 where the radicand is 0"""
    wd = _r(wd, fp32_scalars)
    rad = c * c * sum_gg + 2.0 * c * wd * sum_gp + wd * wd * sum_pp
    return (c * c * sum_gg + 2.0 * c * wd * abs(sum_gp) + wd * wd * sum_pp) / rad if rad > 0.0 else 1.0


def lars_cond(sum_gg, sum_pp, sum_abs_gp, c, wd, g, p, fp32_scalars=True):
    """(c^2 sum g^2 + 2 c wd sum|g p| + wd^2 sum p^2) / |c g + wd p|^2 with the norm taken from the tensors; 1 where that norm is 0"""
    wd = _r(wd, fp32_scalars)
    un2 = float(((c * g.double() + wd * p.double()) ** 2).sum())
    if un2 == 0.0:
        return 1.0
    return (c * c * sum_gg + 2.0 * c * wd * sum_abs_gp + wd * wd * sum_pp) / un2


def ema(tp, p_new, ema_m, fp32_scalars=True):
    return tp * _r(ema_m, fp32_scalars) + p_new * _one_minus(ema_m, fp32_scalars)


# ---- tables and arenas -----------------------------------------------------------------------------------------------------------------
Spec = namedtuple("Spec", "numel group has_grad teacher student_copy teacher_copy")
F32_NAMES = ("p", "g", "m", "v", "t")  # table slots 0 - 4
BF16_NAMES = ("pb", "tb")              # table slots 10, 11
SLOT = {"p": 0, "g": 1, "m": 2, "v": 3, "t": 4, "pb": 10, "tb": 11}


def _roundup(n, k):
    return -(-n // k) * k


class Layout:
    """Where every buffer of every tensor lives: one fp32 arena (p, g, m, v, teacher of each tensor in turn) and one bf16 arena (the two
    copies).  Every buffer has a region whether or not the table points at it -- an absent one keeps the sentinel --, every region
    starts on a 16-byte boundary (4 floats, 8 bf16) and is preceded and followed by at least MOAT sentinel elements; the part of the
    last 16 bytes of a region that the tensor does not use belongs to the moat."""

    def __init__(self, specs, chunk=CHUNK, moat=MOAT):
        self.specs = [Spec(*s) for s in specs]
        assert all(s.numel > 0 and (s.teacher or not s.teacher_copy) for s in self.specs)
        self.chunk, self.moat = chunk, moat
        self.off = {k: [] for k in F32_NAMES + BF16_NAMES}
        o32 = o16 = moat
        for s in self.specs:
            for k in F32_NAMES:
                self.off[k].append(o32)
                o32 += _roundup(s.numel, 4) + moat
            for k in BF16_NAMES:
                self.off[k].append(o16)
                o16 += _roundup(s.numel, 8) + moat
        self.size32, self.size16 = o32, o16
        self.chunks = np.array([(t, c) for t, s in enumerate(self.specs) for c in range(-(-s.numel // chunk))], dtype=np.int32).reshape(-1, 2)
        self.nchunks = len(self.chunks)

    def __len__(self):
        return len(self.specs)

    def nchunks_of(self, i):
        return -(-self.specs[i].numel // self.chunk)

    def present(self, name, i, rule):
        """does the table row of tensor i point at this buffer?  A tensor without the has-gradient bit gets g = exp_avg = exp_avg_sq = 0,
        as FusedClipAdamWEMA builds the row of a frozen parameter; exp_avg_sq exists for AdamW only"""
        s = self.specs[i]
        return {"p": True, "g": bool(s.has_grad), "m": bool(s.has_grad), "v": bool(s.has_grad) and rule == ADAMW, "t": bool(s.teacher),
                "pb": bool(s.student_copy), "tb": bool(s.teacher_copy)}[name]

    def table(self, base32, base16, rule, bc=0):
        """int64 [n, 12] for arenas at the byte addresses base32 / base16"""
        tab = np.zeros((len(self.specs), TFIELDS), dtype=np.int64)
        for i, s in enumerate(self.specs):
            for k in F32_NAMES:
                if self.present(k, i, rule):
                    tab[i, SLOT[k]] = base32 + 4 * self.off[k][i]
            for k in BF16_NAMES:
                if self.present(k, i, rule):
                    tab[i, SLOT[k]] = base16 + 2 * self.off[k][i]
            tab[i, 5], tab[i, 6], tab[i, 7], tab[i, 8] = s.numel, s.group, int(bool(s.has_grad)), bc
        return tab

    def get(self, arena, name, i):
        o = self.off[name][i]
        return arena[o:o + self.specs[i].numel]

    def data_mask(self, names, rule):
        """bool [arena size]: True on the elements of present buffers; everything else (moats, paddings, regions of absent buffers)
        must keep the sentinel"""
        mask = np.zeros(self.size32 if names is F32_NAMES else self.size16, dtype=bool)
        for i, s in enumerate(self.specs):
            for k in names:
                if self.present(k, i, rule):
                    mask[self.off[k][i]:self.off[k][i] + s.numel] = True
        return torch.from_numpy(mask)

    def new_arenas(self):
        return torch.full((self.size32,), SENTINEL, dtype=torch.float32), torch.full((self.size16,), SENTINEL, dtype=torch.bfloat16)


# ---- the tensor set of the element tests ---------------------------------------------------------------------------------------------
#            numel      group grad teacher scopy tcopy
SPECS = [
    (1,                 1, 1, 1, 1, 1),  # 0
    (3,                 0, 1, 0, 0, 0),  # 1
    (4,                 0, 1, 1, 1, 0),  # 2  whole float4
    (5,                 1, 0, 1, 0, 1),  # 3  no gradient
    (4095,              0, 1, 1, 1, 1),  # 4  small gradient: coef >= 1
    (4096,              1, 0, 0, 1, 0),  # 5  whole, no gradient, no teacher
    (4097,              1, 1, 0, 1, 0),  # 6  two chunks, the second a single scalar
    (2 * 4096 + 2,      0, 0, 1, 0, 1),  # 7  three chunks, no gradient
    (257 * 4096 + 5,    0, 1, 1, 1, 1),  # 8  more than 256 chunks; a block of exact zeros in g
    (2 * 4096,          0, 1, 1, 0, 1),  # 9  whole, two chunks, small gradient: coef >= 1
    (4096 + 4,          0, 1, 1, 1, 1),  # 10 p == 0 everywhere: LARS |p| == 0
    (4096 + 3,          0, 1, 1, 1, 0),  # 11 g == 0 everywhere: sqnorm == 0, and with wd == 0 LARS |u| == 0
]
ZERO_P, ZERO_G, SMALL_G, BIG, ZERO_BLOCK = 10, 11, (4, 9), 8, (1000, 3000)
ALIGNED = (1, 2)  # group-0 tensors of a few elements: g takes the signs of p, so that c g + wd p cannot cancel (cond = cs = 1)
CS_MAX = 1.5


def guard_layout():
    """300 tensors of 1 to 8 elements: the guard's loop over the statistics takes a second trip (and a fourth for LARS)"""
    return Layout([(1 + i % 8, i % 2, 1, i % 3 != 0, i % 4 != 0, (i % 3 != 0) and i % 5 != 0) for i in range(300)])


def _spread(n, gen):
    """randn * 10^(4 rand - 2); a magnitude below 1e-6 is lifted to it so that no product of the update is subnormal"""
    x = torch.randn(n, generator=gen) * 10.0 ** (4.0 * torch.rand(n, generator=gen) - 2.0)
    return torch.where(x.abs() < 1e-6, torch.full_like(x, 1e-6), x)


def make_inputs(layout, rule, seed=5, zero_moments=False, special=False):
    """-> (fp32 arena, bf16 arena) on the CPU: sentinels everywhere, data in the present buffers.  The copies start as garbage (a stale
    copy must be overwritten), the moments as a previous step would leave them (exp_avg_sq >= 0).  special: the layout is SPECS and gets
    its zero tensors, small gradients and zero block."""
    gen = torch.Generator().manual_seed(seed)
    a32, a16 = layout.new_arenas()
    for i, s in enumerate(layout.specs):
        n = s.numel
        p, g, m, v, t = _spread(n, gen), _spread(n, gen), 0.3 * _spread(n, gen), _spread(n, gen) ** 2, _spread(n, gen)
        if special:
            if i == ZERO_P:
                p.zero_()
            if i == ZERO_G:
                g.zero_()
            if i in SMALL_G:
                g *= 1e-3
            if i == BIG:
                g[ZERO_BLOCK[0]:ZERO_BLOCK[1]] = 0.0
            if i in ALIGNED:
                g = g.abs() * torch.sign(p)
        if zero_moments:
            m.zero_()
            v.zero_()
        for k, x in zip(F32_NAMES, (p, g, m, v, t)):
            if layout.present(k, i, rule):
                layout.get(a32, k, i).copy_(x)
        for k in BF16_NAMES:
            if layout.present(k, i, rule):
                layout.get(a16, k, i).copy_((torch.rand(n, generator=gen) + 500.0).to(torch.bfloat16))
    return a32, a16


# hyper-parameters of a launch: (clip, lr, wd, h1, h2, eps, ema_m) in the argument order of esvit_fused_clip_update_ema, and the step count t
BASE = {ADAMW: dict(clip=3.0, lr=1e-3, wd=0.05, h1=0.9, h2=0.999, eps=1e-8, ema_m=0.996, t=3),
        SGD: dict(clip=3.0, lr=0.1, wd=0.05, h1=0.9, h2=0.0, eps=1e-8, ema_m=0.996, t=3),
        LARS: dict(clip=3.0, lr=0.1, wd=0.05, h1=0.9, h2=0.001, eps=1e-8, ema_m=0.996, t=3)}
T_BC2_ONE = 20000  # 0.999^20000 = 2e-9 < 2^-25: 1 - b2^t rounds to exactly 1.0f
VARIANTS = {"main": {}, "noclip": dict(clip=0.0), "lr0": dict(lr=0.0), "ema1": dict(ema_m=1.0), "ema0": dict(ema_m=0.0), "wd0": dict(wd=0.0)}
ADAMW_STEPS = {"t1": dict(t=1, zero_moments=True), "t2": dict(t=2), "t1000": dict(t=1000), "tbig": dict(t=T_BC2_ONE)}


def variants(rule):
    out = dict(VARIANTS)
    if rule == ADAMW:
        out.update(ADAMW_STEPS)
    return out


def hyper(rule, **over):
    h = dict(BASE[rule])
    h.update(over)
    h["bc"] = pack_bc(h["h1"], h["h2"], h["t"]) if rule == ADAMW else 0
    return h


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------
def _ratio(err, room):
    """max err / room; 0 / 0 (a relation whose every term is zero must be reproduced exactly) counts as 0, x / 0 as inf"""
    r = torch.where(room > 0, err / room.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                       b.contiguous().view(torch.int32 if b.dtype == torch.float32 else torch.int16))


def check_statistics(layout, a32, got, stats):
    """level 1: `got` (fp32 [n * stats], the atomic esvit_grad_sqnorm) against fp64 within (32 + chunks_t) u sum|terms|; exactly 0 for a
    tensor without the has-gradient bit -> (worst err / bound, [what broke])"""
    worst, broken = 0.0, []
    got = got.double().view(len(layout), stats)
    for i, s in enumerate(layout.specs):
        if not s.has_grad:
            if bool((got[i] != 0).any()):
                broken.append("statistics of tensor %d (no gradient) are not 0" % i)
            continue
        ref = statistics(layout.get(a32, "g", i), layout.get(a32, "p", i) if stats == 3 else None)
        for k, (want, abs_sum) in enumerate(ref):
            lim = (32 + layout.nchunks_of(i)) * U * abs_sum
            err = abs(float(got[i, k]) - want)
            r = err / lim if lim > 0 else (0.0 if err == 0 else float("inf"))
            worst = max(worst, r)
            if not err <= lim:
                broken.append("statistic %d of tensor %d: err %.3e bound %.3e" % (k, i, err, lim))
    return worst, broken


def factors(layout, rule, h, a32, stats, i):
    """c and q of tensor i in fp64 from the statistics given (fp32 [n * S] of the device, or None: fp64 from the tensors)"""
    s = layout.specs[i]
    if not s.has_grad:
        return 1.0, 1.0
    S = 3 if rule == LARS else 1
    if stats is None:
        st = [x[0] for x in statistics(layout.get(a32, "g", i), layout.get(a32, "p", i) if S == 3 else None)]
    else:
        st = [float(x) for x in stats.double().view(len(layout), S)[i]]
    c = clip_coef(st[0], h["clip"])
    q = lars_q(st[0], st[1], st[2], c, h["wd"], h["h2"], s.group) if rule == LARS else 1.0
    return c, q


def check_factors(layout, rule, h, a32, stats):
    """level 2: c and q from the device's statistics against c and q from the fp64 tensors -> ({name: worst err / bound}, [broken])"""
    worst, broken = {"c": 0.0, "q": 0.0}, []
    for i, s in enumerate(layout.specs):
        if not s.has_grad:
            continue
        c_dev, q_dev = factors(layout, rule, h, a32, stats, i)
        c_ref, q_ref = factors(layout, rule, h, a32, None, i)
        B = 32 + layout.nchunks_of(i)
        lim = (B / 2.0 + 1.0) * U * c_ref
        if (c_ref == 1.0) != (c_dev == 1.0) or abs(c_dev - c_ref) > lim:
            broken.append("c of tensor %d: %r from the device's statistic, %r in fp64" % (i, c_dev, c_ref))
        worst["c"] = max(worst["c"], abs(c_dev - c_ref) / lim)
        if rule == LARS and s.group == 0:
            g, p = layout.get(a32, "g", i), layout.get(a32, "p", i)
            (gg, _), (pp, _), (_, agp) = statistics(g, p)
            cond = lars_cond(gg, pp, agp, c_ref, h["wd"], g, p)
            lim = (B * (1.0 + cond) / 2.0 + 8.0) * U * q_ref
            if cond > COND_MAX or abs(q_dev - q_ref) > lim:
                broken.append("q of tensor %d: %r from the device's statistics, %r in fp64, cond %.2f" % (i, q_dev, q_ref, cond))
            worst["q"] = max(worst["q"], abs(q_dev - q_ref) / lim)
        elif q_dev != 1.0 or q_ref != 1.0:
            broken.append("q of tensor %d is not 1" % i)
    return worst, broken


def check_update(layout, rule, h, in32, in16, out32, out16, stats):
    """level 3 and the exact properties, on CPU tensors: the arenas before and after one esvit_fused_clip_update_ema and the statistics it
    read -> ({relation: worst err / bound}, [what broke])"""
    worst, broken = {}, []

    def rel(name, got, want, room_terms, k):
        room = k * U * room_terms
        err = (got.double() - want).abs()
        worst[name] = max(worst.get(name, 0.0), _ratio(err, room))
        if not bool((err <= room).all()):
            j = int((err - room).argmax())
            broken.append("%s: err %.3e bound %.3e at element %d" % (name, float(err[j]), float(room[j]), j))

    lr, wd, ema_m = f32(h["lr"]), f32(h["wd"]), f32(h["ema_m"])
    for i, s in enumerate(layout.specs):
        tag = "tensor %d" % i
        p0, p1 = layout.get(in32, "p", i), layout.get(out32, "p", i)
        if s.has_grad:
            g = layout.get(in32, "g", i).double()
            c, q = factors(layout, rule, h, in32, stats, i)
            m0, m1 = layout.get(in32, "m", i).double(), layout.get(out32, "m", i)
            wdp = wd if s.group == 0 else 0.0
            if rule == ADAMW:
                b1, b2 = f32(h["h1"]), f32(h["h2"])
                bc1, bc2 = unpack_bc(h["bc"])
                v0, v1 = layout.get(in32, "v", i).double(), layout.get(out32, "v", i)
                want_m, want_v = adamw_moments(g, m0, v0, c, b1, b2)
                o1, o2 = _one_minus(b1, True), _one_minus(b2, True)
                rel("m", m1, want_m, m0.abs() + (o1 * c * g).abs() + (o1 * m0).abs(), K[ADAMW]["m"])
                rel("v", v1, want_v, (b2 * v0).abs() + o2 * (c * g) ** 2, K[ADAMW]["v"])
                want_p = adamw_param(p0.double(), m1.double(), v1.double(), lr, wd, s.group, h["eps"], bc1, bc2)
                t1 = p0.double() * _decay(lr, wd, s.group, True)
                rel("p", p1, want_p, t1.abs() + (want_p - t1).abs(), K[ADAMW]["p"])
                if bool((v1 < 0).any()):
                    broken.append(tag + ": exp_avg_sq went negative")
            else:
                mom = f32(h["h1"])
                want_mu = momentum_buffer(p0.double(), g, m0, c, q, wd, s.group, mom)
                rel("mu", m1, want_mu, (mom * m0).abs() + (q * c * g).abs() + (q * wdp * p0.double()).abs(), K[rule]["mu"])
                rel("p", p1, momentum_param(p0.double(), m1.double(), lr), p0.double().abs() + (lr * m1.double()).abs(), K[rule]["p"])
            if lr == 0.0 and not _same_bits(p1, p0):
                broken.append(tag + ": lr == 0 moved p")
            if lr == 0.0 and _same_bits(m1, layout.get(in32, "m", i)):
                broken.append(tag + ": lr == 0 froze the moments too")
            if not _same_bits(layout.get(out32, "g", i), layout.get(in32, "g", i)):
                broken.append(tag + ": g was written")
        elif not _same_bits(p1, p0):
            broken.append(tag + ": p of a tensor without gradient moved")
        if s.teacher:
            t0, t1_ = layout.get(in32, "t", i), layout.get(out32, "t", i)
            om = _one_minus(ema_m, True)
            rel("ema", t1_, ema(t0.double(), p1.double(), ema_m), (t0.double() * ema_m).abs() + (p1.double() * om).abs(), K_EMA)
            if ema_m == 1.0 and not _same_bits(t1_, t0):
                broken.append(tag + ": ema_m == 1 moved the teacher")
            if ema_m == 0.0 and not _same_bits(t1_, p1):
                broken.append(tag + ": ema_m == 0 did not make the teacher p'")
            if s.teacher_copy and not _same_bits(layout.get(out16, "tb", i), t1_.to(torch.bfloat16)):
                broken.append(tag + ": teacher copy != bf16(teacher')")
        if s.student_copy and not _same_bits(layout.get(out16, "pb", i), p1.to(torch.bfloat16)):
            broken.append(tag + ": student copy != bf16(p')")
    # whatever is not a present buffer keeps its sentinel: moats, the unused end of a region's last 16 bytes, regions of absent buffers
    for name, names, before, after in (("fp32", F32_NAMES, in32, out32), ("bf16", BF16_NAMES, in16, out16)):
        quiet = ~layout.data_mask(names, rule)
        if not _same_bits(after[quiet], before[quiet]):
            broken.append("the %s arena was written outside the present buffers" % name)
    return worst, broken


def unchanged(in32, in16, out32, out16):
    return _same_bits(in32, out32) and _same_bits(in16, out16)
