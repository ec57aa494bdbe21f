"""The wide LayerNorm rows of esvit_amd/csrc/norm.hip (ln_wide_fwd_kernel / ln_wide_bwd_kernel: 2048 < C <= 8192, C % 1024 == 0, behind
esvit_layernorm_fwd / esvit_layernorm_bwd / esvit_merge_ln_fwd / esvit_merge_ln_bwd): the case table tests/test_norm_wide_gpu.py and
tests/test_swin_large_cpu.py share, the restated block-count rule, the fp64 statement with its bounds, one runner shaped like the C ABI
(every output inside a sentinel moat, every input between NaN rows) that drives either the library on the device or an fp32 emulation
in the kernels' order on the CPU, and the mutants of that emulation.

The statement and the bound formulas are those of tests/norm_ref.py (imported, not edited: ln_forward, ln_backward, act_copy; its module
docstring derives them).  They read the reduction depths through norm_ref.ln_shape / ln_bwd_blocks / fold_depth, which know the twelve
narrow instantiations only; wide_rules() puts the wide kernels' depths there for the duration of a call and hands widths up to 2048 on
to the originals:
  row reductions   hsum4 (two additions deep), NV = C / 1024 sequential additions in the lane, six butterfly steps in the wave, four
                   sequential additions over the waves' partials in LDS (block_sum):  ns = 2 + NV + 6 + 4, stated to norm_ref as a
                   64-lane group with ITERS = NV + 4
  dgamma / dbeta   one row at a time per workgroup, so no fold over row groups: `trips` additions in the lane, then partial_reduce_kernel
                   as in norm_ref:  ng = trips + ceil(ceil(nblk / SLICES) / 4) + 2 + SLICES (+ 1 with accumulate)
  blocks           min(rows, 1024); the forward launches one workgroup per row
No bound is tuned and none takes the allowance norm_ref.reference() adds from the fp32 restatement: these are the derived bounds alone."""
import contextlib
import functools

import torch

from tests import norm_ref as NR

WIDTHS = (3072, 4096, 5120, 6144, 7168, 8192)
REFUSED = (98, 2052, 2560, 9216)
MAX_BLOCKS = 1024
THREADS = 256
DTYPES = NR.DTYPES
SENTINEL = NR.SENTINEL
MERGE_PAD_FLAG = 0x40000000  # ESVIT_MERGE_PAD (include/esvit_hip.h)


# ---- the host rules, restated -----------------------------------------------------------------------------------------------------------
def nv(C):
    """vectors per lane of the wide kernels, 0 where the width is not theirs"""
    return C // 1024 if (2048 < C <= 8192 and C % 1024 == 0) else 0


def blocks(rows, C):
    """ESVIT_Q_LN_BWD_BLOCKS at the wide widths; at the others the rule of norm_ref (0 where the library refuses)"""
    return max(1, min(MAX_BLOCKS, rows)) if nv(C) else NR.ln_bwd_blocks(rows, C)


def _ln_shape(C, _orig=NR.ln_shape):
    return (64, nv(C) + 4, 1) if nv(C) else _orig(C)


def _ln_bwd_blocks(rows, C, _orig=NR.ln_bwd_blocks):
    return blocks(rows, C) if nv(C) else _orig(rows, C)


def _fold_depth(rows, C, accumulate=False, _orig=NR.fold_depth):
    if not nv(C):
        return _orig(rows, C, accumulate)
    nblk = blocks(rows, C)
    trips = -(-rows // nblk)
    slices = 32 if nblk >= 256 else 8
    return trips + -(-(-(-nblk // slices)) // 4) + 2 + slices + (1 if accumulate else 0)


@contextlib.contextmanager
def wide_rules():
    saved = NR.ln_shape, NR.ln_bwd_blocks, NR.fold_depth
    NR.ln_shape, NR.ln_bwd_blocks, NR.fold_depth = _ln_shape, _ln_bwd_blocks, _fold_depth
    try:
        yield
    finally:
        NR.ln_shape, NR.ln_bwd_blocks, NR.fold_depth = saved


# ---- the case table --------------------------------------------------------------------------------------------------------------------
def _ln(name, C, rows, **kw):
    c = dict(kind="ln", name=name, C=C, rows=rows, eps=1e-6, fill="normal", want_f32=False, g_in=False, bwd="plain", rowscale=None,
             gb="adjacent", map=None)
    c.update(kw)
    return c


def _merge(nB, H, W, Cin, pad=False):
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if pad else (H // 2, W // 2)
    return dict(kind="merge", name="wmerge_%s%dx%dx%dx%d" % ("pad_" if pad else "", nB, H, W, Cin), nB=nB, H=H, W=W, Cin=Cin, C=4 * Cin,
                rows=nB * Ho * Wo, eps=1e-6, pad=pad)


SHAPE_WIDTHS = (3072, 5120, 8192)
SHAPE_ROWS = (1, 5, MAX_BLOCKS + 5)  # 1024 + 5: blocks 0 .. 4 take two trips through the backward loop, the others one
V = 3072  # every option once at this width


def _build():
    cs = [_ln("wln_w%d_r%d" % (C, r), C, r) for C in SHAPE_WIDTHS for r in SHAPE_ROWS]
    cs += [_ln("wln_var_f32", V, 5, want_f32=True),
           _ln("wln_var_gin", V, 5, g_in=True),
           _ln("wln_var_act", V, 5, g_in=True, bwd="cast"),
           _ln("wln_var_act_rs2", V, 5, g_in=True, bwd="cast", rowscale=2),  # samples of two rows (the last of one), a factor 0 among them
           _ln("wln_var_toact", V, 5, bwd="to_act"),
           _ln("wln_var_gb_separate", V, 5, gb="separate"),
           _ln("wln_map_h6_s3", V, 2 * 36, map=(6, 7, 3, 2))]  # 6 x 6 tokens in one shifted 7 x 7 window: 13 pad slots per sample
    for eps in (1e-6, 1e-5):
        for fill in ("mean100", "const"):
            cs.append(_ln("wln_num_%s_e%d" % (fill, 6 if eps == 1e-6 else 5), V, 5, eps=eps, fill=fill))
    cs += [_merge(1, 2, 2, 768), _merge(2, 4, 6, 768), _merge(1, 3, 5, 768, pad=True)]
    return cs


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def params(prefix=""):
    return [(c, dt) for c in CASES for dt in DTYPES if c["name"].startswith(prefix)]


def ids(ps):
    return ["%s-%s" % (c["name"], NR.dt_name(dt)) for c, dt in ps]


# ---- geometry --------------------------------------------------------------------------------------------------------------------------
def merge_src(nB, H, W, pad):
    """[merged rows, 4] token row of every quadrant in the order (0,0) (1,0) (0,1) (1,1); -1 where pad mode reads a token past the grid"""
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if pad else (H // 2, W // 2)
    r = torch.arange(nB * Ho * Wo)
    b, i, j = r // (Ho * Wo), (r % (Ho * Wo)) // Wo, r % Wo
    q = torch.arange(4)
    ti, tj = 2 * i[:, None] + (q & 1)[None, :], 2 * j[:, None] + (q >> 1)[None, :]
    src = (b[:, None] * H + ti) * W + tj
    return torch.where((ti < H) & (tj < W), src, torch.full_like(src, -1))


def _gather(xt, src, Cin):
    """token rows [T, Cin] -> merged rows [R, 4 Cin], zeros where src is -1"""
    g = xt[src.clamp(min=0)] * (src >= 0).to(xt.dtype)[:, :, None]
    return g.reshape(src.shape[0], 4 * Cin)


def _map_rows(case):
    if case.get("map") is None:
        return None, case["rows"], None, 0
    H, ws, shift, nB = case["map"]
    t2w, period = NR.row_map(H, ws, shift)
    r = torch.arange(case["rows"])
    return (r // (H * H)) * period + t2w[r % (H * H)], nB * period, t2w, period


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _inputs(name, dt):
    c = BY_NAME[name]
    C, rows, D = c["C"], c["rows"], NR.data
    if c["kind"] == "merge":
        T = c["nB"] * c["H"] * c["W"]
        x = D((name, "x"), (T, c["Cin"])) * 1.5 + 0.3
        xg = _gather(x, merge_src(c["nB"], c["H"], c["W"], c["pad"]), c["Cin"])
        rs = D((name, "rs"), (T,)).abs() + 0.5
        rs[1] = 0.0
        extra = dict(dy2=D((name, "dy2"), (rows, C), dt), rowscale=rs, gb_prev=D((name, "gbp"), (2, C)))
        drows = rows
    else:
        z = D((name, "x"), (rows, C))
        if c["fill"] == "normal":
            x = z * 1.5 + D((name, "xm"), (rows, 1), scale=0.5)
        elif c["fill"] == "mean100":  # |mean| = 100 std
            x = z + torch.where(torch.arange(rows) % 2 == 0, 100.0, -100.0).view(rows, 1)
        else:
            x = D((name, "xc"), (rows, 1), scale=3.0).expand(rows, C).contiguous()
        xg = x
        drows = _map_rows(c)[1]
        extra = dict(g_in=D((name, "gin"), (rows, C)), dy_f32=D((name, "dy32"), (rows, C)))
        if c["rowscale"]:
            rs = D((name, "rs"), (-(-rows // c["rowscale"]),)).abs() + 0.5
            rs[1] = 0.0
            extra["rowscale"] = rs
    x64 = xg.double()
    mean = x64.mean(1)
    rstd = (((x64 - mean[:, None]) ** 2).mean(1) + NR._f32(c["eps"])) ** -0.5
    return dict(x=x, gamma=1.0 + D((name, "gamma"), (C,), scale=0.2), beta=D((name, "beta"), (C,), scale=0.1), dy=D((name, "dy"), (drows, C), dt),
                mean=mean.float(), rstd=rstd.float(), **extra)


def inputs(case, dt):
    return _inputs(case["name"], dt)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def statement(case, dt):
    """-> fp64 tensors under the keys of run()'s outputs, each with ab_ (the expression in absolute values) and bd_ (its bound)"""
    with wide_rules():
        return _statement(case, dt)


def _statement(case, dt):
    x, res, f64 = inputs(case, dt), {}, (lambda t: t.double())
    C, rows, eps = case["C"], case["rows"], NR._f32(case["eps"])
    if case["kind"] == "ln":
        fw = NR.ln_forward(f64(x["x"]), f64(x["gamma"]), f64(x["beta"]), eps, C, dt)
        NR._put(res, fw, ("mean", "rstd"))
        ri, drows, _, _ = _map_rows(case)
        if ri is None:
            NR._put(res, fw, ("y",))
        else:  # the row-mapped store into a zero-initialised output: pad rows stay exactly 0
            for p, fill in (("", 0.0), ("ab_", 0.0), ("bd_", NR.FLOOR)):
                buf = torch.full((drows, C), fill, dtype=torch.float64)
                buf[ri] = fw[p + "y"]
                res[p + "y"] = buf
        if case["want_f32"]:
            res.update(y_f32=fw["y"], ab_y_f32=fw["ab_y"], bd_y_f32=fw["bd_y_f32"])
        d = f64(x["dy_f32"] if case["bwd"] == "to_act" else x["dy"])
        if ri is not None:
            d = d[ri]
        bw = NR.ln_backward(f64(x["x"]), d, f64(x["mean"]), f64(x["rstd"]), f64(x["gamma"]), C, g_in=f64(x["g_in"]) if case["g_in"] else None)
        NR._put(res, bw, ("dgamma", "dbeta"))
        if case["bwd"] != "to_act":
            NR._put(res, bw, ("dx",))
        if case["bwd"] in ("cast", "to_act"):
            sc = torch.ones(rows, 1, dtype=torch.float64)
            if case["rowscale"]:
                sc = f64(x["rowscale"])[torch.arange(rows) // case["rowscale"]].view(rows, 1)
            res["dx_act"], res["bd_dx_act"] = NR.act_copy(bw["dx"], bw["bd_dx"], sc, dt)
            res["ab_dx_act"] = sc.abs() * bw["ab_dx"]
        return res
    nB, H, W, Cin = case["nB"], case["H"], case["W"], case["Cin"]
    src = merge_src(nB, H, W, case["pad"])
    xg = _gather(f64(x["x"]), src, Cin)  # (a pad quadrant is a run of zeros that enters the statistics)
    fw = NR.ln_forward(xg, f64(x["gamma"]), f64(x["beta"]), eps, C, dt)
    NR._put(res, fw, ("mean", "rstd", "y"))
    st = (f64(x["mean"]), f64(x["rstd"]), f64(x["gamma"]), C)
    bw = NR.ln_backward(xg, f64(x["dy"]), *st)
    b2 = NR.ln_backward(xg, f64(x["dy2"]), *st, accumulate=True)
    NR._put(res, bw, ("dgamma", "dbeta"))
    live = (src >= 0).reshape(-1)
    for p in ("", "ab_", "bd_"):  # the scatter to the token rows: every token of the true grid is written once, a pad quadrant has no dx
        buf = torch.zeros(nB * H * W, Cin, dtype=torch.float64)
        buf[src.reshape(-1)[live]] = bw[p + "dx"].reshape(rows * 4, Cin)[live]
        res[p + "dx"] = buf
    one, rs = torch.ones(nB * H * W, 1, dtype=torch.float64), f64(x["rowscale"]).view(-1, 1)
    res["act"], res["bd_act"] = NR.act_copy(res["dx"], res["bd_dx"], one, dt)
    res["act_rs"], res["bd_act_rs"] = NR.act_copy(res["dx"], res["bd_dx"], rs, dt)
    res["ab_act"], res["ab_act_rs"] = res["ab_dx"], rs * res["ab_dx"]
    for k in ("dgamma", "dbeta"):  # the first call overwrites what the destination held, the second adds
        res["acc_" + k] = bw[k] + b2[k]
        res["ab_acc_" + k] = bw["ab_" + k] + b2["ab_" + k]
        res["bd_acc_" + k] = bw["bd_" + k] + b2["bd_" + k] + NR.U * (bw[k].abs() + b2[k].abs())
    return res


@functools.lru_cache(maxsize=2)
def _reference(name, dt):
    return statement(BY_NAME[name], dt)


def reference(case, dt):
    """the statement, computed once per (case, dtype) and shared"""
    return _reference(case["name"], dt)


# ---- buffers of the runner -------------------------------------------------------------------------------------------------------------
def _pad_of(t):
    return t.shape[-1] if t.dim() == 2 else 4  # one row, or 16 bytes of a vector: the 16-byte accesses of the kernels stay aligned


def guard(t, dev):
    """the tensor on the device between NaN rows (int maps: between rows of an index far outside)"""
    t = t.contiguous()
    n = _pad_of(t)
    flat = torch.full((t.numel() + 2 * n,), float("nan") if t.is_floating_point() else 2 ** 30, dtype=t.dtype, device=dev)
    flat[n:n + t.numel()] = t.reshape(-1).to(dev)
    return flat[n:n + t.numel()].view(t.shape)


class Out:
    """an output inside a moat of sentinels"""

    def __init__(self, shape, dt, dev, init=None):
        n = shape[-1] if len(shape) == 2 else 4
        size = 1
        for s in shape:
            size *= s
        self.n, self.size = n, size
        self.buf = torch.full((size + 2 * n,), SENTINEL, dtype=dt, device=dev)
        self.t = self.buf[n:n + size].view(shape)
        if init is not None:
            self.t.fill_(init)

    def moat(self):
        return bool((self.buf[:self.n] == SENTINEL).all()) and bool((self.buf[self.n + self.size:] == SENTINEL).all())


# ---- the two libraries behind the runner: C-ABI-shaped calls on preallocated tensors, 0 = done ---------------------------------------
class Device:
    """esvit_amd's shared library through ctypes; the workspace is exactly what ESVIT_Q_LN_BWD_BLOCKS answers, inside a moat"""

    def __init__(self):
        from esvit_amd import ops
        self.o, self.ws = ops, []

    def _ws(self, rows, C, dev):
        n = self.o.query(self.o.Q_LN_BWD_BLOCKS, rows, C)
        w = Out((max(n, 1), 2 * C), torch.float32, dev)
        self.ws.append(w)
        return w.t

    def fwd(self, dt, x, gamma, beta, eps, rows, C, y, y_f32, mean, rstd, rowmap, tokens, period_out):
        o = self.o
        return o.lib.esvit_layernorm_fwd(o._code(dt), o._p(x), o._p(gamma), o._p(beta), eps, rows, C, o._p(y), o._p(y_f32), o._p(mean), o._p(rstd),
                                         o._p(rowmap), tokens, period_out, o._stream())

    def bwd(self, dt, dy, x, mean, rstd, gamma, g_in, rows, C, dx, dgamma, dbeta, rowmap, tokens, period_in, dx_act, act_dt, rowscale, rps):
        o = self.o
        return o.lib.esvit_layernorm_bwd(o._code(dt), o._p(dy), o._p(x), o._p(mean), o._p(rstd), o._p(gamma), o._p(g_in), rows, C, o._p(dx), o._p(dgamma),
                                         o._p(dbeta), o._p(self._ws(rows, C, x.device)), o._p(rowmap), tokens, period_in, o._p(dx_act),
                                         o._code(act_dt) if dx_act is not None else 0, o._p(rowscale), rps, o._stream())

    def merge_fwd(self, dt, x, gamma, beta, eps, nB, H, W, Cin, pad, y, mean, rstd):
        o = self.o
        return o.lib.esvit_merge_ln_fwd(o._code(dt), o._p(x), o._p(gamma), o._p(beta), eps, nB, H | (MERGE_PAD_FLAG if pad else 0), W, Cin, o._p(y),
                                        o._p(mean), o._p(rstd), o._stream())

    def merge_bwd(self, dt, dy, x, mean, rstd, gamma, nB, H, W, Cin, pad, dx, dgamma, dbeta, dx_act, rowscale, rps, accumulate):
        o = self.o
        rows = mean.numel()
        return o.lib.esvit_merge_ln_bwd(o._code(dt), o._p(dy), o._p(x), o._p(mean), o._p(rstd), o._p(gamma), nB, H | (MERGE_PAD_FLAG if pad else 0), W, Cin,
                                        o._p(dx), o._p(dgamma), o._p(dbeta), o._p(self._ws(rows, 4 * Cin, x.device)), o._p(dx_act), o._p(rowscale), rps,
                                        int(accumulate), o._stream())

    def ws_moats(self):
        ok = all(w.moat() for w in self.ws)
        self.ws = []
        return ok


MUTANTS = ("wave_partial_left_out", "last_slice_skipped", "second_trip_overwrites", "pad_quadrant_dropped", "rowscale_ignored",
           "accumulate_overwrites")
# the cases that must catch each mutant (tests/test_swin_large_cpu.py asserts that each does, in both dtypes)
MUTANT_CASES = {
    "wave_partial_left_out": ("wln_w3072_r1", "wln_w8192_r5"),
    "last_slice_skipped": ("wln_w3072_r5", "wln_w5120_r1", "wmerge_1x2x2x768"),
    "second_trip_overwrites": ("wln_w3072_r1029", "wln_w5120_r1029"),
    "pad_quadrant_dropped": ("wmerge_pad_1x3x5x768",),
    "rowscale_ignored": ("wln_var_act_rs2", "wmerge_2x4x6x768"),
    "accumulate_overwrites": ("wmerge_1x2x2x768", "wmerge_pad_1x3x5x768"),
}


class Emulation:
    """the wide kernels in fp32 torch on the CPU, behind the same calls: the same reduction shapes (hsum4, NV additions in the lane, the
    butterfly of the wave, the four partials added in order; the row loop and partial_reduce_kernel for dgamma / dbeta) and the same
    rounding points up to the compiler's contractions"""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant

    def ws_moats(self):
        return True

    def _slices(self, C):
        live = torch.ones(C)
        if self.mutant == "last_slice_skipped":
            live[(nv(C) - 1) * 1024:] = 0.0
        return live

    def _rowsum(self, X):
        """X [R, C] fp32 -> [R]: lane t holds the vectors t + it 256"""
        R, C = X.shape
        Vv = X.view(R, nv(C), THREADS, 4)
        h = (Vv[..., 0] + Vv[..., 1]) + (Vv[..., 2] + Vv[..., 3])
        s = torch.zeros(R, THREADS)
        for i in range(nv(C)):
            s = s + h[:, i]
        s = s.view(R, THREADS // 64, 64)
        idx, o = torch.arange(64), 32
        while o:
            s = s + s[:, :, idx ^ o]
            o //= 2
        r = torch.zeros(R)
        for w in range(THREADS // 64 - (1 if self.mutant == "wave_partial_left_out" else 0)):
            r = r + s[:, w, 0]
        return r

    def _fwd(self, xg, gamma, beta, eps, stat_live=None):
        C = xg.shape[1]
        live = self._slices(C)
        xs = xg * live
        mu = (self._rowsum(xs) / C).view(-1, 1)
        d = (xs - mu) * live
        if stat_live is not None:
            d = d * stat_live
        rs = torch.rsqrt(self._rowsum(d * d) / C + torch.tensor(eps, dtype=torch.float32))
        return ((xg - mu) * rs.view(-1, 1) * gamma + beta) * live, mu[:, 0].clone(), rs

    def _bwd(self, xg, d, mean, rstd, gamma, stat_live=None, prev=None):
        """-> (dx before g_in [rows, C], dgamma, dbeta)"""
        rows, C = xg.shape
        live = self._slices(C) if stat_live is None else self._slices(C) * stat_live
        mu, rs = mean.view(-1, 1), rstd.view(-1, 1)
        xh = (xg - mu) * rs * live
        gd = d * gamma * live
        dl = d * live
        s1 = (self._rowsum(gd) / C).view(-1, 1)
        s2 = (self._rowsum(gd * xh) / C).view(-1, 1)
        o = (gd - s1 - xh * s2) * rs
        contrib = torch.cat([dl * xh, dl], 1)
        nblk = blocks(rows, C)
        trips = -(-rows // nblk)
        P = torch.zeros(trips * nblk, 2 * C)
        P[:rows] = contrib
        P = P.view(trips, nblk, 2 * C)
        acc = torch.zeros(nblk, 2 * C)
        for t in range(trips):
            if self.mutant == "second_trip_overwrites" and t >= 1:
                took = torch.arange(nblk) + t * nblk < rows
                acc = torch.where(took.view(-1, 1), P[t], acc)
            else:
                acc = acc + P[t]
        gb = NR.Emulation._partial_reduce(acc)
        if prev is not None and self.mutant != "accumulate_overwrites":
            gb = prev + gb
        return o, gb[:C].clone(), gb[C:].clone()

    def fwd(self, dt, x, gamma, beta, eps, rows, C, y, y_f32, mean, rstd, rowmap, tokens, period_out):
        if not nv(C):
            return -1
        o, mu, rs = self._fwd(x.reshape(rows, C), gamma, beta, eps)
        r = torch.arange(rows)
        ro = r if rowmap is None else (r // tokens) * period_out + rowmap.long()[r % tokens]
        y[ro] = o.to(dt)
        if y_f32 is not None:
            y_f32.copy_(o)
        mean.copy_(mu), rstd.copy_(rs)
        return 0

    def bwd(self, dt, dy, x, mean, rstd, gamma, g_in, rows, C, dx, dgamma, dbeta, rowmap, tokens, period_in, dx_act, act_dt, rowscale, rps):
        if not nv(C):
            return -1
        r = torch.arange(rows)
        d = dy.float()[r if rowmap is None else (r // tokens) * period_in + rowmap.long()[r % tokens]]
        o, dg, db = self._bwd(x.reshape(rows, C), d, mean, rstd, gamma)
        if g_in is not None:
            o = o + g_in
        if dx is not None:
            dx.copy_(o)
        if dx_act is not None:
            sc = torch.ones(rows) if (rowscale is None or self.mutant == "rowscale_ignored") else rowscale[r // rps]
            dx_act.copy_((o * sc.view(-1, 1)).to(act_dt))
        dgamma.copy_(dg), dbeta.copy_(db)
        return 0

    def _stat_live(self, src, Cin):
        if self.mutant != "pad_quadrant_dropped":
            return None
        return (src >= 0).float()[:, :, None].expand(-1, -1, Cin).reshape(src.shape[0], 4 * Cin)

    def merge_fwd(self, dt, x, gamma, beta, eps, nB, H, W, Cin, pad, y, mean, rstd):
        src = merge_src(nB, H, W, pad)
        o, mu, rs = self._fwd(_gather(x, src, Cin), gamma, beta, eps, self._stat_live(src, Cin))
        y.copy_(o.to(dt)), mean.copy_(mu), rstd.copy_(rs)
        return 0

    def merge_bwd(self, dt, dy, x, mean, rstd, gamma, nB, H, W, Cin, pad, dx, dgamma, dbeta, dx_act, rowscale, rps, accumulate):
        src = merge_src(nB, H, W, pad)
        prev = torch.cat([dgamma, dbeta]).clone() if accumulate else None
        o, dg, db = self._bwd(_gather(x, src, Cin), dy.float(), mean, rstd, gamma, self._stat_live(src, Cin), prev)
        live = (src >= 0).reshape(-1)
        tok = src.reshape(-1)[live]
        o = o.reshape(-1, Cin)[live]
        dx[tok] = o
        if dx_act is not None:
            sc = torch.ones(tok.numel()) if (rowscale is None or self.mutant == "rowscale_ignored") else rowscale[tok // rps]
            dx_act[tok] = (o * sc.view(-1, 1)).to(dx_act.dtype)
        dgamma.copy_(dg), dbeta.copy_(db)
        return 0


# ---- the runner ------------------------------------------------------------------------------------------------------------------------
def _run_ln(be, dev, case, dt):
    x = inputs(case, dt)
    C, rows = case["C"], case["rows"]
    ri, drows, t2w, period = _map_rows(case)
    G = lambda t: guard(t, dev)  # noqa: E731
    xd, gamma, beta = G(x["x"]), G(x["gamma"]), G(x["beta"])
    rowmap = None if t2w is None else G(t2w.to(torch.int32))
    tokens = 0 if t2w is None else t2w.numel()
    y = Out((drows, C), dt, dev, init=0.0 if ri is not None else None)  # (the row-mapped store goes into a zeroed output)
    yf = Out((rows, C), torch.float32, dev) if case["want_f32"] else None
    mean, rstd = Out((rows,), torch.float32, dev), Out((rows,), torch.float32, dev)
    outs = [y, mean, rstd] + ([yf] if yf else [])
    rc = be.fwd(dt, xd, gamma, beta, case["eps"], rows, C, y.t, yf.t if yf else None, mean.t, rstd.t, rowmap, tokens, period)
    assert rc == 0, rc
    raw = dict(y=y.t, mean=mean.t, rstd=rstd.t)
    flags = {}
    if ri is not None:
        padrows = torch.ones(drows, dtype=torch.bool)
        padrows[ri] = False
        flags["equal_pad_zero"] = float(bool((y.t[padrows.to(dev)] == 0).all()))
    if yf:
        raw["y_f32"] = yf.t
    to_act = case["bwd"] == "to_act"
    dy = G(x["dy_f32"] if to_act else x["dy"])
    gb = Out((5, C), torch.float32, dev)
    dg, db = gb.t[1], gb.t[2 if case["gb"] == "adjacent" else 3]
    dx = None if to_act else Out((rows, C), torch.float32, dev)
    dxa = Out((rows, C), dt, dev) if case["bwd"] != "plain" else None
    rsc = G(x["rowscale"]) if case["rowscale"] else None
    rc = be.bwd(torch.float32 if to_act else dt, dy, xd, G(x["mean"]), G(x["rstd"]), gamma, G(x["g_in"]) if case["g_in"] else None, rows, C,
                dx.t if dx else None, dg, db, rowmap, tokens, period, dxa.t if dxa else None, dt, rsc, case["rowscale"] or 0)
    assert rc == 0, rc
    raw.update(dgamma=dg, dbeta=db)
    if dx:
        raw["dx"] = dx.t
    if dxa:
        raw["dx_act"] = dxa.t
    outs += [gb] + ([dx] if dx else []) + ([dxa] if dxa else [])
    idle = (0, 4) + ((3,) if case["gb"] == "adjacent" else (2,))
    flags["equal_moat"] = float(all(o.moat() for o in outs) and all(bool((gb.t[r] == SENTINEL).all()) for r in idle) and be.ws_moats())
    return raw, flags


def _run_merge(be, dev, case, dt):
    x = inputs(case, dt)
    nB, H, W, Cin, C, rows, pad = case["nB"], case["H"], case["W"], case["Cin"], case["C"], case["rows"], case["pad"]
    T = nB * H * W
    G = lambda t: guard(t, dev)  # noqa: E731
    xd, gamma, beta = G(x["x"]), G(x["gamma"]), G(x["beta"])
    y, mean, rstd = Out((rows, C), dt, dev), Out((rows,), torch.float32, dev), Out((rows,), torch.float32, dev)  # (row slices of larger buffers)
    assert be.merge_fwd(dt, xd, gamma, beta, case["eps"], nB, H, W, Cin, pad, y.t, mean.t, rstd.t) == 0
    raw = dict(y=y.t, mean=mean.t, rstd=rstd.t)
    st = (G(x["mean"]), G(x["rstd"]), gamma, nB, H, W, Cin, pad)
    dy, dy2, rsc = G(x["dy"]), G(x["dy2"]), G(x["rowscale"])
    gb = Out((4, C), torch.float32, dev)
    gb.t[1:3] = x["gb_prev"].to(dev)
    dx = Out((T, Cin), torch.float32, dev)
    assert be.merge_bwd(dt, dy, xd, *st, dx.t, gb.t[1], gb.t[2], None, None, 1, 0) == 0  # (overwrites what the destination held)
    raw.update(dx=dx.t.clone(), dgamma=gb.t[1].clone(), dbeta=gb.t[2].clone())
    dx2, act = Out((T, Cin), torch.float32, dev), Out((T, Cin), dt, dev)
    assert be.merge_bwd(dt, dy, xd, *st, dx2.t, gb.t[1], gb.t[2], act.t, None, 1, 0) == 0
    raw["act"] = act.t.clone()
    flags = dict(equal_dx_out=float(torch.equal(dx2.t, dx.t)), equal_overwrite=float(torch.equal(gb.t[1], raw["dgamma"]) and torch.equal(gb.t[2], raw["dbeta"])))
    assert be.merge_bwd(dt, dy, xd, *st, dx2.t, gb.t[1], gb.t[2], act.t, rsc, 1, 0) == 0
    raw["act_rs"] = act.t.clone()
    assert be.merge_bwd(dt, dy2, xd, *st, dx2.t, gb.t[1], gb.t[2], None, None, 1, 1) == 0  # accumulate
    raw.update(acc_dgamma=gb.t[1].clone(), acc_dbeta=gb.t[2].clone())
    flags["equal_moat"] = float(all(o.moat() for o in (y, mean, rstd, gb, dx, dx2, act)) and bool((gb.t[0] == SENTINEL).all()) and bool((gb.t[3] == SENTINEL).all())
                                and be.ws_moats())
    return raw, flags


def run(be, dev, case, dt, repeat=False):
    """every entry of the case through `be` -> fp64 CPU tensors under the statement's keys and equal_* flags; repeat: a second launch of
    everything on the same inputs gave the same bits"""
    fn = _run_ln if case["kind"] == "ln" else _run_merge
    raw, flags = fn(be, dev, case, dt)
    if repeat:
        again, _ = fn(be, dev, case, dt)
        flags["equal_repeat"] = float(all(torch.equal(raw[k], again[k]) for k in raw))
    res = {k: v.detach().cpu().double() for k, v in raw.items()}
    res.update(flags)
    return res


def metrics(case, dt, got):
    """err / bound of every output over every element, and the run's equal_* flags"""
    ref = reference(case, dt)
    m = {}
    for k in NR.outputs(ref):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        m["ratio_" + k] = NR.ratio(got[k], ref[k], ref["bd_" + k])
    m.update({k: v for k, v in got.items() if k.startswith("equal_")})
    return m
