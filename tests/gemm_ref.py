"""The fp64 statement of one esvit_gemm call (include/esvit_hip.h, esvit_gemm_desc), inputs for which the GEMM is EXACT, the case
table of tests/test_gemm_gpu.py, the moats around every operand and the mutants tests/test_gemm_cpu.py proves the comparison catches.

Exact inputs.  A holds i * 2^-SA with |i| <= 3, B holds j * 2^-SB with |j| <= 2, bias / residual / an accumulated-into C hold
integers times 2^-(SA+SB), rowscale is in {0, 0.5, 1, 2}, alpha in {1, 0.5, -2}.  Every product and every partial sum is then a multiple of
2^-(SA+SB+2) (alpha = 0.5 and rowscale = 0.5 each cost one more bit) far below 2^24 such units (check_exact), so an fp32 accumulation gives the exact value in ANY order, fused or not, on both
MFMA types, split over K or not, reduced in any tree.  Before the activation function nothing has a tolerance: an fp32 output equals the
fp64 statement bit for bit, a bf16 output equals torch's round-to-nearest-even cast of it (the skewed integer distributions put most
values of the longer reductions between bf16 neighbours and many exactly half way: 257 must become 256).  +0 and -0 count as equal.

Activation epilogues (GELU, QuickGELU and their derivatives) take symmetric inputs scaled so the pre-activation spreads over about
[-6, 6] and the bound of tests/conv_ref.py (affine acts 1, 2):
    |got - ref| <= max(3 x the worst error of the fp32 restatement oracle/ops_ref on the same inputs against fp64, 16 u max|ref|)
                   (+ 2^-8 |ref| for a bf16 output),  u = 2^-24.
The device's erf_fast / __expf error cannot be derived here, so it is measured against the reference, never against the kernel.

Moats.  Every operand lives inside a larger buffer: lda / ldb / ldc / ldaux / ldr wider than dense, guard rows before and after, batch
items apart; input pads hold NaN (a kernel that reads a pad and multiplies by zero fails on NaN x 0), outputs -- C, aux, partial, colsum,
colsum_partial -- hold a NaN sentinel bit pattern that must survive everywhere the statement writes nothing (pad columns, guard rows,
rows no row map targets).  The `defeat` set of a case moves a pointer 8 bytes (bias: one float) or makes a pitch 4 mod 8 (ldr: 2 mod 4)
so that whole interior tiles leave the straight-line epilogues (gemm_epilogue_bf16, p8_epi_matches) for the general ones and their
per-item scalar fallbacks.
"""
import math
import zlib

import torch

U = 2.0 ** -24
BF = 2.0 ** -8
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)
AUTO, REGSTAGE, DMA4, DMA8, DMA4W, P8 = range(6)
KNAME = {AUTO: "auto", REGSTAGE: "regstage", DMA4: "dma4", DMA8: "dma8", DMA4W: "dma4w", P8: "p8"}
EPI_NONE, EPI_GELU, EPI_GELU_BWD, EPI_QGELU, EPI_QGELU_BWD = range(5)
SA, SB = 2, 1                      # A = i 2^-SA, B = j 2^-SB
SENT32, SENT16 = 0x7FC12345, 0x7FC5  # NaN bit patterns no kernel produces
GUARD = 2                          # guard rows before and after every plane


def dt_name(dt):
    return {F32: "fp32", BF16: "bf16"}[dt]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()) % (2 ** 31))


def ints(key, shape, lim, probs=None):
    """seeded integers in [-lim, lim] as fp64: uniform, or drawn with `probs` (2 lim + 1 weights)"""
    n = 1
    for s in shape:
        n *= s
    if probs is None:
        v = torch.randint(-lim, lim + 1, (n,), generator=_gen(*key))
    else:
        v = torch.multinomial(torch.tensor(probs, dtype=torch.float64), n, replacement=True, generator=_gen(*key)) - lim
    return v.double().view(*shape)


A_SKEW = (.03, .03, .04, .05, .1, .25, .5)  # mean 1.91: sums grow with K past the 8 bits of a bf16 mantissa (2.2 units per k: beyond 256
B_SKEW = (.04, .06, .1, .3, .5)             # mean 1.16  units from K = 128 on, beyond 512 from K = 256 on), signs still mix


# ---- the statement -------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def qgelu64(x):
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad64(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1.0 + 1.702 * x * (1.0 - s))


def _at(ptr, idx):
    buf, off = ptr
    return buf[off + idx]


def reference(p, mutant=None):
    """esvit_gemm on the descriptor `p` in fp64.  Pointer fields are (flat tensor, element offset) pairs or None: fp64 copies of the
    buffers as they lie in memory, NaN pads included (int64 for rowmap); C is its contents before the call.
    -> {"C" | "aux" | "colsum": (flat element index int64 [n], value fp64 [n], the activation's argument fp64 [n] or None, the linear
    part alpha acc + bias fp64 [n])}: every element the call writes, un-rounded; everything else must not be written."""
    g = lambda k, d=0: p.get(k, d) if p.get(k, d) is not None else d
    M, N, K = p["M"], p["N"], p["K"]
    aks, bks = g("a_kstrided"), g("b_kstrided")
    batch, splitk = max(1, g("batch", 1)), g("splitk")
    alpha, epi = float(g("alpha", 1.0)), g("epilogue")
    m = torch.arange(M).view(M, 1)
    n = torch.arange(N).view(1, N)
    k = torch.arange(K)
    idx_c, val_c, pre_c, lin_c, idx_x, val_x = [], [], [], [], [], []
    out = {}
    for z in range(batch):
        zb = 0 if mutant == "batch_b0" else z
        a = _at(p["A"], z * g("strideA") + (k.view(1, K) * p["lda"] + m if aks else m * p["lda"] + k.view(1, K)))        # op(A) [M, K]
        b = _at(p["B"], zb * g("strideB") + (k.view(K, 1) * p["ldb"] + n if bks else n.view(1, N) * p["ldb"] + k.view(K, 1)))  # op(B) [K, N]
        if mutant == "k_chunk":
            a = a.clone()
            a[:, K - 8:] = 0
        if mutant == "last_slice" and splitk > 1:   # the last non-empty slice of 64-deep k-tiles never reaches the reduction
            nkt = -(-K // 64)
            per = -(-nkt // splitk)
            a = a.clone()
            a[:, ((nkt - 1) // per) * per * 64:] = 0
        acc = a @ b
        v = acc * alpha
        if mutant == "alpha_twice" and splitk > 1:
            v = v * alpha
        if z == 0 and p.get("colsum") is not None:
            cs = acc.sum(1) if mutant == "colsum_n" else a.sum(1)
            out["colsum"] = (p["colsum"][1] + torch.arange(M), cs * alpha, None, None)
        bias = _at(p["bias"], n) if p.get("bias") is not None else None
        if bias is not None and mutant != "bias_after":
            v = v + (bias * alpha if mutant == "alpha_bias" else bias)
        pre, lin = None, v   # the activation's argument, and the linear part alpha acc + bias
        if epi in (EPI_GELU, EPI_QGELU):
            pre = v
            if p.get("aux") is not None:
                idx_x.append((p["aux"][1] + m * p["ldaux"] + n).reshape(-1))
                val_x.append(v.reshape(-1))
            v = gelu64(v) if epi == EPI_GELU else qgelu64(v)
        elif epi in (EPI_GELU_BWD, EPI_QGELU_BWD):
            x = _at(p["aux"], m * p["ldaux"] + n)
            pre = x
            v = v * (gelu_grad64(x) if epi == EPI_GELU_BWD else qgelu_grad64(x))
        if bias is not None and mutant == "bias_after":
            v = v + bias
        rows = torch.arange(M)
        drow = rows
        written = torch.ones(M, dtype=torch.bool)
        late = None
        if p.get("rowmap") is not None:
            period = g("rowmap_period") + (1 if mutant == "period" else 0)
            tk = _at(p["rowmap"], rows % period)
            drow = (rows // period) * g("rowmap_tokens") + tk
            written = tk >= 0
            if mutant == "dropped_written":   # a dropped row lands on the sample's first token row, after the row that belongs there
                late = ~written
                drow = torch.where(written, drow, (rows // period) * g("rowmap_tokens"))
                written = torch.ones(M, dtype=torch.bool)
        if p.get("rowscale") is not None:
            src = rows if mutant == "rowscale_src" else drow
            v = v * _at(p["rowscale"], torch.where(written, src, torch.zeros_like(src)) // g("rows_per_sample")).view(M, 1)
        if p.get("residual") is not None:
            src = rows % ((M // g("rowmap_period")) * g("rowmap_tokens")) if mutant == "res_src" else drow
            v = v + _at(p["residual"], torch.where(written, src, torch.zeros_like(src)).view(M, 1) * g("ldr") + n)
        ic = p["C"][1] + z * g("strideC") + drow.view(M, 1) * p["ldc"] + n
        if splitk > 1 and g("accumulate"):
            v = v + p["C"][0][ic.clamp(min=0)]
        order = torch.arange(M)
        if late is not None:
            order = torch.cat([order[~late], order[late]])
        order = order[written[order]]
        if late is not None:   # the late store wins
            last = {}
            for r in order.tolist():
                last[int(drow[r])] = r
            order = torch.tensor(sorted(last.values()))
        idx_c.append(ic[order].reshape(-1))
        val_c.append(v[order].reshape(-1))
        pre_c.append(None if pre is None else pre[order].reshape(-1))
        lin_c.append(lin[order].reshape(-1))
    out["C"] = (torch.cat(idx_c), torch.cat(val_c), None if pre_c[0] is None else torch.cat(pre_c), torch.cat(lin_c))
    if idx_x:
        out["aux"] = (torch.cat(idx_x), torch.cat(val_x), None, None)
    return after(p, out, mutant) if mutant in AFTER else out


# mutants that are a transform of the statement's own result (the others above change a step inside it; "trunc" lives in round_to)
AFTER = ("row_drop", "row_dup", "col_drop", "col_dup", "no_acc")


def after(p, out, mutant):
    """the statement's C with the last row / column of every batch item not written or holding its neighbour's values (rows: no row map),
    or without the contents C had before an accumulating call"""
    idx, val, pre, lin = out["C"]
    N = p["N"]
    if mutant == "no_acc":
        return dict(out, C=(idx, val - p["C"][0][idx], pre, lin))
    shape = (-1, N) if mutant.startswith("col") else (-1, p["M"], N)   # every written row is whole: N consecutive entries
    cut = (lambda t: t.view(shape)[:, :-1]) if mutant.startswith("col") else (lambda t: t.view(shape)[:, :-1, :])
    if mutant.endswith("drop"):
        f = lambda t: None if t is None else cut(t).reshape(-1)
        return dict(out, C=(f(idx), f(val), f(pre), f(lin)))

    def dup(t):
        if t is None:
            return None
        t = t.clone().view(shape)
        if mutant == "col_dup":
            t[:, -1] = t[:, -2]
        else:
            t[:, -1, :] = t[:, -2, :]
        return t.reshape(-1)
    return dict(out, C=(idx, dup(val), dup(pre), dup(lin)))


def round_to(v, dt, mutant=None):
    """fp64 -> the stored type as the device must do it: exact to fp32, then round-to-nearest-even to bf16"""
    f = v.float()
    if dt == F32:
        return f
    if mutant == "trunc":
        return (f.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    return f.bfloat16()


# ---- problems: buffers with moats and the descriptor that points into them ---------------------------------------------------------------
def _sentinel(numel, dt):
    if dt == F32:
        return torch.full((numel,), SENT32, dtype=torch.int32).view(torch.float32)
    return torch.full((numel,), SENT16, dtype=torch.int16).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def rowmap_of(kind):
    """-> (map int32 [period], tokens per sample).  "win": Swin's window -> token scatter of a 6 x 6 grid in one padded, shifted 7 x 7
    window (13 dropped slots); "hand": five rows per sample onto seven token rows, of which 1, 4 and 5 are never targeted"""
    if kind == "win":
        from oracle import ops_ref
        return torch.from_numpy(ops_ref.window_maps(6, 6, 7, 3)[0].copy()), 36
    return torch.tensor([3, -1, 0, 6, 2], dtype=torch.int32), 7


ROWSCALES = (1.0, 0.5, 0.0, 2.0)
DEFEATS = ("c_ptr", "ldc", "bias_ptr", "aux_ptr", "ldaux", "res_ptr", "ldr", "stridec", "partial_ptr")
ALL_OFF = frozenset(DEFEATS)


def build(case, dt):
    """-> problem: bufs {name: flat tensor as it is uploaded}, desc {field: scalar | (buffer name, element offset)}, and what
    verify() needs.  Seeded by the case's name."""
    c = case
    M, N, K, lay = c["M"], c["N"], c["K"], c["lay"]
    aks, bks = int(lay == "wg"), int(lay in ("dg", "wg"))
    batch, splitk = c.get("batch", 1), c.get("splitk", 0)
    epi, defeat = c.get("epi", EPI_NONE), frozenset(c.get("defeat", ()))
    act = epi != EPI_NONE
    out_dt = F32 if c.get("out_f32", 0) else dt
    es_c = 4 if out_dt == F32 else 2
    key = (c["name"],)
    bufs, desc, outs = {}, {}, {}
    sa, sb = SA, SB
    if act:  # symmetric integers; the pre-activation sqrt(8 K) 2^-(sa+sb) units wide -> about [-6, 6] at three sigma
        sa, sb = 1, max(0, round(math.log2(math.sqrt(8.0 * K) / 2.0)) - 1)
    unit_ab = 2.0 ** -(sa + sb)

    def plane(name, rows, cols, pad, t_dt, values, nb=1, off=0, sentinel=False, stride_mod=None):
        """[nb] planes of rows x cols at pitch cols + pad, GUARD rows around, `off` elements into the buffer; values [nb, rows, cols] or None"""
        ld = cols + pad
        stride = (rows + GUARD) * ld if nb > 1 else 0
        if stride_mod is not None:
            while stride % 8 != stride_mod:
                stride += 1
        total = off + GUARD * ld + (nb - 1) * stride + (rows + GUARD) * ld
        buf = _sentinel(total, t_dt) if sentinel else torch.full((total,), float("nan"), dtype=t_dt)
        base = off + GUARD * ld
        if values is not None:
            for z in range(nb):
                buf[base + z * stride: base + z * stride + rows * ld].view(rows, ld)[:, :cols] = values[z].to(t_dt)
        bufs[name] = buf
        return base, ld, stride

    def vec(name, n, values, off=0, sentinel=False):
        buf = _sentinel(off + n + 8, F32) if sentinel else torch.full((off + n + 8,), float("nan"), dtype=F32)
        if values is not None:
            buf[off + 4: off + 4 + n] = values.float()
        bufs[name] = buf
        return off + 4

    ldpad = 8 if dt == BF16 else 4  # lda / ldb stay multiples of the 16-byte vector (validate)
    ra, ca = (K, M) if aks else (M, K)
    rb, cb = (K, N) if bks else (N, K)
    av = ints(key + ("A",), (batch, ra, ca), 3, None if act else A_SKEW) * 2.0 ** -sa
    bv = ints(key + ("B",), (batch, rb, cb), 2, None if act else B_SKEW) * 2.0 ** -sb
    base, ld, st = plane("A", ra, ca, 2 * ldpad, dt, av, nb=batch)
    desc.update(A=("A", base), lda=ld, strideA=st)
    base, ld, st = plane("B", rb, cb, ldpad, dt, bv, nb=batch)
    desc.update(B=("B", base), ldb=ld, strideB=st)

    rm = c.get("rowmap")
    out_rows = M
    if rm:
        rmap, tokens = rowmap_of(rm)
        period = rmap.numel()
        assert M % period == 0
        out_rows = (M // period) * tokens
        bufs["rowmap"] = torch.cat([torch.full((4,), -7, dtype=torch.int32), rmap.int(), torch.full((4,), -7, dtype=torch.int32)])
        desc.update(rowmap=("rowmap", 4), rowmap_period=period, rowmap_tokens=tokens)
    if c.get("bias"):
        desc["bias"] = ("bias", vec("bias", N, ints(key + ("bias",), (N,), 6 if act else 40) * unit_ab, off=1 if "bias_ptr" in defeat else 0))
    if c.get("rowscale"):
        rps = tokens if rm else 24
        ns = -(-out_rows // rps)
        desc["rowscale"] = ("rowscale", vec("rowscale", ns, torch.tensor([ROWSCALES[(i + 1) % 4] for i in range(ns)])))
        desc["rows_per_sample"] = rps
    if epi in (EPI_GELU_BWD, EPI_QGELU_BWD) or c.get("aux"):
        xv = ints(key + ("aux",), (1, M, N), 48).mul(0.125) if epi in (EPI_GELU_BWD, EPI_QGELU_BWD) else None
        base, ld, _ = plane("aux", M, N, 4 if "ldaux" in defeat else 8, dt, xv, off=(8 // (2 if dt == BF16 else 4)) if "aux_ptr" in defeat else 0,
                            sentinel=xv is None)
        desc.update(aux=("aux", base), ldaux=ld)
        if xv is None:
            outs["aux"] = dt
    # C: its contents before the call matter when the call accumulates into it (split-K accumulate; residual = C)
    res_is_c = c.get("residual") == "C"
    cinit = ints(key + ("C",), (batch, out_rows, N), 50) * unit_ab if (c.get("accumulate") or res_is_c) else None
    cpad = (4 if "ldc" in defeat else 8) if splitk <= 1 else 0   # split-K wants a dense C
    base, ld, st = plane("C", out_rows, N, cpad, out_dt, cinit, nb=batch, off=(8 // es_c) if "c_ptr" in defeat else 0, sentinel=True,
                         stride_mod=(4 if "stridec" in defeat else 0) if batch > 1 else None)
    desc.update(C=("C", base), ldc=ld, strideC=st)
    outs["C"] = out_dt
    if res_is_c:
        desc.update(residual=("C", base), ldr=ld)
    elif c.get("residual"):
        base, ld, _ = plane("residual", out_rows, N, 2 if "ldr" in defeat else 4, F32, ints(key + ("res",), (1, out_rows, N), 60) * unit_ab,
                            off=2 if "res_ptr" in defeat else 0)
        desc.update(residual=("residual", base), ldr=ld)
    if splitk > 1:
        off = 1 if "partial_ptr" in defeat else 0
        bufs["partial"] = _sentinel(off + splitk * M * N + 16, F32)
        desc.update(partial=("partial", off + 8), splitk=splitk, accumulate=int(c.get("accumulate", 0)))
        outs["partial"] = F32
    if c.get("colsum"):
        desc["colsum"] = ("colsum", vec("colsum", M, None, sentinel=True))
        outs["colsum"] = F32
        if splitk > 1:
            bufs["colsum_partial"] = _sentinel(splitk * M + 16, F32)
            desc["colsum_partial"] = ("colsum_partial", 8)
            outs["colsum_partial"] = F32
    desc.update(M=M, N=N, K=K, a_kstrided=aks, b_kstrided=bks, batch=batch, epilogue=epi, out_f32=int(c.get("out_f32", 0)),
                alpha=c.get("alpha", 1.0), kernel=c["kern"] if dt == BF16 else AUTO)
    return dict(case=c, dt=dt, bufs=bufs, desc=desc, outs=outs, act=act, unit=unit_ab / 4)


def ref_view(prob):
    """the descriptor over fp64 copies of the buffers, for reference()"""
    p = {}
    for f, v in prob["desc"].items():
        if isinstance(v, tuple):
            b = prob["bufs"][v[0]]
            p[f] = (b.long() if b.dtype == torch.int32 else b.double(), v[1])
        else:
            p[f] = v
    return p


def expected(prob, mutant=None):
    """-> {output: (buffer as it must read after the call, written index, fp64 value, pre-activation)}"""
    ref = reference(ref_view(prob), mutant)
    exp = {}
    for name, (idx, val, pre, lin) in ref.items():
        buf = prob["bufs"][name].clone()
        buf[idx] = round_to(val, prob["outs"][name], mutant)
        exp[name] = (buf, idx, val, pre, lin)
    return exp


def check_exact(prob):
    """every value the accumulation can pass through is a whole number of units below 2^24 -- the condition under which fp32 is exact
    in any order.  -> the largest abs_sum in units"""
    p = ref_view(prob)
    lin = dict(p, epilogue=EPI_NONE, aux=None)   # the activation's argument alpha acc + bias (GELU') / everything (no activation)
    for name, (idx, val, _, _) in reference(lin).items():
        u = val / prob["unit"]
        assert bool(torch.isfinite(u).all()) and bool((u == u.round()).all()), (prob["case"]["name"], name)
    q = dict(lin, alpha=abs(p.get("alpha", 1.0)))
    for f in ("A", "B", "bias", "residual", "C"):
        if q.get(f) is not None:
            q[f] = (torch.nan_to_num(q[f][0].abs(), nan=0.0), q[f][1])
    if q.get("rowscale") is not None:
        q["rowscale"] = (torch.full_like(q["rowscale"][0], 2.0), q["rowscale"][1])
    worst = max(float(val.max()) for _, val, _, _ in reference(q).values()) / prob["unit"]
    assert worst < 2 ** 24, worst
    return worst


def act_bound(prob, val, pre, lin):
    """per-element bound of an activation epilogue's C: the fp32 restatement (oracle/ops_ref) on the same exact inputs, measured against fp64"""
    from oracle import ops_ref
    epi = prob["desc"]["epilogue"]
    x = pre.float()
    if epi == EPI_GELU:
        got = ops_ref._gelu(x)
    elif epi == EPI_QGELU:
        got = ops_ref._qgelu(x)
    else:
        got = lin.float() * (ops_ref._gelu_grad(x) if epi == EPI_GELU_BWD else ops_ref._qgelu_grad(x))
    base = max(3.0 * float((got.double() - val).abs().max()), 16 * U * float(val.abs().max()))
    return base + (BF * val.abs() if prob["outs"]["C"] == BF16 else 0.0)


def verify(prob, got, exp=None, record=None):
    """the comparison of the GPU test: `got` {output: flat tensor after the call}.  -> list of failures (empty = pass)"""
    exp = exp or expected(prob)
    bad = []
    name_ = prob["case"]["name"] + "-" + dt_name(prob["dt"])
    for name in prob["outs"]:
        g = got[name]
        if name in ("partial", "colsum_partial"):  # slabs of slices: guards intact, every plane written, the planes sum to the statement
            n = prob["desc"]["M"] * (prob["desc"]["N"] if name == "partial" else 1)
            off, sk = prob["desc"][name][1], prob["desc"]["splitk"]
            mask = torch.ones(g.numel(), dtype=torch.bool)
            mask[off: off + sk * n] = False
            if not torch.equal(_bits(g)[mask], _bits(prob["bufs"][name])[mask]):
                bad.append("%s %s: guard overwritten" % (name_, name))
            tot = g[off: off + sk * n].double().view(sk, n).sum(0)
            src = "C" if name == "partial" else "colsum"
            want = exp[src][2]
            if name == "partial" and prob["desc"].get("accumulate"):
                want = want - ref_view(prob)["C"][0][exp["C"][1]]
            if not (bool(torch.isfinite(tot).all()) and torch.equal(tot, want)):
                bad.append("%s %s: slices do not sum to the statement" % (name_, name))
            continue
        buf, idx, val, pre, lin = exp[name]
        same = (_bits(g) == _bits(buf)) | ((g == 0) & (buf == 0))
        if prob["act"] and name == "C":
            w = torch.zeros(g.numel(), dtype=torch.bool)
            w[idx] = True
            if not bool(same[~w].all()):
                bad.append("%s C: %d elements outside the written set changed" % (name_, int((~same[~w]).sum())))
            gv = g[idx].double()
            bound = act_bound(prob, val, pre, lin)
            err = (gv - val).abs()
            ratio = float((err / bound).max()) if bool(torch.isfinite(gv).all()) else float("inf")
            if record is not None:
                record(test="gemm", case=name_, kernel=KNAME[resolves_to(prob["case"], prob["dt"])[0]], out=dt_name(prob["outs"]["C"]), where="mi355x",
                       max_err=float(err.max()), ratio=ratio)
            if not ratio <= 1.0:
                bad.append("%s C: err / bound = %.3g" % (name_, ratio))
        elif not bool(same.all()):
            i = int((~same).nonzero()[0])
            bad.append("%s %s: %d of %d elements differ, first at %d: got %r, want %r" % (name_, name, int((~same).sum()), g.numel(), i, float(g[i]), float(buf[i])))
    return bad


def run(ops, dev, prob):
    """one launch through ops._gemm on fresh copies of the buffers -> ({output: flat tensor on the host}, resolved (kernel, tile_m, tile_n))"""
    d = {n: b.to(dev) for n, b in prob["bufs"].items()}
    assert all(t.data_ptr() % 16 == 0 for t in d.values())   # what addresses() assumed
    kw = {f: (d[v[0]][v[1]:] if isinstance(v, tuple) else v) for f, v in prob["desc"].items()}
    sel = ops.gemm_select(prob["dt"], **kw)[:3]
    ops._gemm(prob["dt"], **kw)
    torch.cuda.synchronize()
    return {n: d[n].cpu() for n in prob["outs"]}, sel


def run_and_verify(ops, dev, case, dt, record=None):
    """the GPU test of one case: resolved loop and tile, exact comparison + moats, and a second launch with the same bits"""
    prob = build(case, dt)
    got, sel = run(ops, dev, prob)
    bad = verify(prob, got, record=record)
    if sel != resolves_to(case, dt):
        bad.append("%s-%s: resolved to %r, the table says %r" % (case["name"], dt_name(dt), sel, resolves_to(case, dt)))
    again, _ = run(ops, dev, prob)
    for n in prob["outs"]:
        if not torch.equal(_bits(got[n]), _bits(again[n])):
            bad.append("%s-%s %s: a second launch gave other bits" % (case["name"], dt_name(dt), n))
    return bad


# ---- which loop and tile a case must resolve to (gemm.hip: choose, dma4_tile, dma4w_tile) -------------------------------------------------
def tile4(N):
    return 96 if (N % 96 == 0 and N % 128 != 0) else (64 if N <= 64 else 128)


def resolves_to(case, dt):
    if "want" in case and dt == BF16:
        return case["want"]
    N = case["N"]
    if dt == F32:
        return (REGSTAGE, 128, tile4(N))
    kern = case["kern"]
    if kern == DMA4:
        return (DMA4, 128, tile4(N))
    if kern == DMA4W:
        assert N % 96 == 0
        return (DMA4W, 128, 192 if N % 192 == 0 else 96)
    assert kern in (DMA8, P8), case
    return (kern, 256, 256)


def loops(lay, N, K, rowmap=False):
    """the bf16 main loops that take a problem when forced"""
    out = [DMA4]
    if N % 96 == 0:
        out.append(DMA4W)
    if lay != "wg":
        out.append(DMA8)
    if K % 64 == 0 and not rowmap:
        out.append(P8)
    return out


# forced loops the library refuses by contract (check_selector): listed, never silently replaced; tests/test_gemm_cpu.py pins each
REFUSED = [
    dict(why="eight-phase loop: K % 64 != 0", dt=BF16, lay="nt", M=296, N=328, K=200, kern=P8),
    dict(why="eight-phase loop: row map", dt=BF16, lay="nt", M=196, N=152, K=64, kern=P8, rowmap="win"),
    dict(why="8-wave tile: weight-gradient layout", dt=BF16, lay="wg", M=328, N=328, K=200, kern=DMA8),
    dict(why="register-staged loop in bf16", dt=BF16, lay="nt", M=168, N=152, K=72, kern=REGSTAGE),
    dict(why="LDS-DMA loop in fp32", dt=F32, lay="nt", M=168, N=152, K=72, kern=DMA4),
    dict(why="weight-gradient layout: M % 8 != 0 (the 300 x 300 multi-item walk runs as 304 x 296 there)", dt=BF16, lay="wg", M=300, N=300, K=128, kern=P8,
         validate=True),
]


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def _case(family, name, lay, M, N, K, kern, dts=DTYPES, **kw):
    c = dict(family=family, name="%s-%s-%s-%dx%dx%d-%s" % (family, name, lay, M, N, K, KNAME[kern]), lay=lay, M=M, N=N, K=K, kern=kern, dts=dts)
    c.update(kw)
    return c


def _with_fp32(kern):
    return DTYPES if kern == DMA4 else (BF16,)   # the fp32 loop runs once per shape, beside the default bf16 loop


def _shapes():
    out = []
    nt = [(40, 24, 8), (168, 152, 72), (168, 77, 72)] + [(168, n, 136) for n in (64, 96, 288, 192, 384, 200)]
    for M, N, K in nt:
        for kern in (DMA4, DMA4W):
            if kern in loops("nt", N, K):
                out.append(_case("shape", "plain", "nt", M, N, K, kern, _with_fp32(kern)))
    for K in (64, 128, 200):
        out.append(_case("shape", "plain", "nt", 296, 328, K, DMA8, (BF16,)))
    for K in (64, 128, 192, 256, 448):
        out.append(_case("shape", "plain", "nt", 296, 328, K, P8, (BF16,)))
    for N in (24, 152, 96, 192, 328):
        for M, K in ((40, 8), (168, 72), (168, 136)):
            for kern in (DMA4, DMA4W):
                if kern in loops("dg", N, K):
                    out.append(_case("shape", "plain", "dg", M, N, K, kern, _with_fp32(kern)))
        for K in (64, 128, 200):
            out.append(_case("shape", "plain", "dg", 296, N, K, DMA8, (BF16,)))
        for K in (64, 128, 192, 256, 448):
            out.append(_case("shape", "plain", "dg", 296, N, K, P8, (BF16,)))
    return out


def _wgrad():
    out = []
    mn = (40, 96, 152, 192, 328)
    for K in (8, 72, 200, 448):
        for i, M in enumerate(mn):
            for s in (0, 2):
                N = mn[(i + s) % 5]
                for kern in loops("wg", N, K):
                    out.append(_case("wgrad", "plain", "wg", M, N, K, kern, _with_fp32(kern), out_f32=1))
                    out.append(_case("wgrad", "colsum", "wg", M, N, K, kern, _with_fp32(kern), out_f32=1, colsum=1))
                    out.append(_case("wgrad", "resC", "wg", M, N, K, kern, _with_fp32(kern), out_f32=1, colsum=s // 2, residual="C"))
    return out


# (name, layout, fields); outputs have the activation dtype unless out_f32
EPILOGUES = [
    ("none", "nt", {}), ("bias", "nt", dict(bias=1)), ("bias-f32", "nt", dict(bias=1, out_f32=1)),
    ("gelu", "nt", dict(bias=1, epi=EPI_GELU)), ("gelu-aux", "nt", dict(bias=1, epi=EPI_GELU, aux=1)),
    ("qgelu", "nt", dict(bias=1, epi=EPI_QGELU)), ("qgelu-aux", "nt", dict(epi=EPI_QGELU, aux=1)),
    ("gelubwd", "dg", dict(epi=EPI_GELU_BWD)), ("gelubwd-f32", "dg", dict(epi=EPI_GELU_BWD, out_f32=1)),
    ("qgelubwd", "dg", dict(epi=EPI_QGELU_BWD)), ("qgelubwd-f32", "dg", dict(epi=EPI_QGELU_BWD, out_f32=1)),
    ("res-f32", "nt", dict(bias=1, residual=1, out_f32=1)), ("res", "nt", dict(residual=1)),
    ("res-rs-f32", "nt", dict(bias=1, residual=1, rowscale=1, out_f32=1)), ("res-rs", "nt", dict(bias=1, residual=1, rowscale=1)),
    ("res-f32", "wg", dict(residual=1, out_f32=1)),
    ("rs", "nt", dict(bias=1, rowscale=1)), ("rs-alone", "nt", dict(rowscale=1)),
    ("alpha.5-bias", "nt", dict(bias=1, alpha=0.5)), ("alpha-2-bias", "nt", dict(bias=1, alpha=-2.0)), ("alpha-2-bias-f32", "dg", dict(bias=1, alpha=-2.0, out_f32=1)),
]
ROWMAPS = [
    ("win-res-rs-f32", 196, dict(rowmap="win", bias=1, residual=1, rowscale=1, out_f32=1)),
    ("win-res", 196, dict(rowmap="win", residual=1)),
    ("win-plain", 196, dict(rowmap="win", bias=1)),
    ("hand-res-rs-f32", 170, dict(rowmap="hand", bias=1, residual=1, rowscale=1, out_f32=1)),
    ("hand-rs", 170, dict(rowmap="hand", rowscale=1)),
]
# the interior-plus-ragged shape of every tile: (kernel, M, N, K)
TILE_SHAPES = [(DMA4, 168, 152, 72), (DMA4, 168, 288, 72), (DMA4, 168, 64, 72), (DMA4W, 168, 384, 72), (DMA4W, 168, 288, 72),
               (DMA8, 296, 328, 72), (P8, 296, 328, 128)]


def _epilogues():
    out = []
    for kern, M, N, K in TILE_SHAPES:
        for name, lay, f in EPILOGUES:
            if kern not in loops(lay, N, K):
                continue
            for defeat in ((), ALL_OFF):
                out.append(_case("epi", name + ("-off" if defeat else "-dense"), lay, M, N, K, kern, _with_fp32(kern), defeat=defeat, **f))
    for kern in (DMA4, DMA4W, DMA8):
        for name, M, f in ROWMAPS:
            N = 288 if kern == DMA4W else 152
            for defeat in ((), ALL_OFF):
                out.append(_case("rowmap", name + ("-off" if defeat else "-dense"), "nt", M, N, 72, kern, _with_fp32(kern), defeat=defeat, **f))
    # one condition of the fast-path predicates at a time, on a shape with interior tiles
    full = dict(bias=1, residual=1, out_f32=1)
    for kern, M, N, K in ((DMA4, 168, 152, 72), (P8, 296, 328, 128)):
        for term in ("c_ptr", "ldc", "bias_ptr", "res_ptr", "ldr"):
            out.append(_case("single", term, "nt", M, N, K, kern, _with_fp32(kern), defeat=(term,), **full))
        for term in ("aux_ptr", "ldaux"):
            out.append(_case("single", term + "-gelu", "nt", M, N, K, kern, _with_fp32(kern), defeat=(term,), bias=1, epi=EPI_GELU, aux=1))
            out.append(_case("single", term + "-gelubwd", "dg", M, N, K, kern, _with_fp32(kern), defeat=(term,), epi=EPI_GELU_BWD))
    return out


def _splitk():
    out = []
    # (dg, 168 x 192 / 288: the two whole-width tiles 128 x 192 and 128 x 96 with a k-strided B; the default loop has its dg cases at N = 152)
    for lay, M, N in (("dg", 168, 152), ("dg", 168, 192), ("dg", 168, 288), ("wg", 152, 192), ("dg", 296, 328), ("wg", 328, 296)):
        big = M > 200
        for kern in loops(lay, N, 320):
            if big != (kern in (DMA8, P8)) or (lay == "dg" and N % 96 == 0 and kern != DMA4W):
                continue
            for sk in (2, 3, 7, 4):   # 5 k-tiles of 64: slices of 3+2, 2+2+1, 1 x 5 + 2 empty, 2+2+1 + 1 empty
                for of32, acc in ((1, 0), (1, 1), (0, 0), (0, 1)):
                    f = dict(splitk=sk, out_f32=of32, accumulate=acc, colsum=int(lay == "wg"))
                    if sk == 3:
                        f["alpha"] = 0.5
                    if sk == 7 and of32:
                        f["defeat"] = ("partial_ptr",)
                    # fp32 mode: 32-deep k-tiles, K = 160 gives the same five
                    out.append(_case("splitk", "s%d-%s%s" % (sk, "f32" if of32 else "act", "-acc" if acc else ""), lay, M, N, 320, kern, (BF16,), **f))
                    if kern == DMA4 and of32:
                        out.append(_case("splitk", "s%d-f32%s" % (sk, "-acc" if acc else ""), lay, M, N, 160, kern, (F32,), **f))
    # the forward shape with N = 77: partial rows at odd addresses, scalar partial stores; splitk 3 of two k-tiles leaves slice 2 empty
    # 165 x 77: M N % 4 == 1, the reduction's last quad is a single element
    for M in (168, 165):
        for sk in (2, 3):
            for of32 in (1, 0):
                out.append(_case("splitk", "n77-s%d-%s" % (sk, "f32" if of32 else "act"), "nt", M, 77, 72, DMA4, DTYPES if of32 else (BF16,), splitk=sk,
                                 out_f32=of32, alpha=0.5 if sk == 2 else 1.0))
    # N % 4 != 0 on whole interior tiles: the partial planes start off the 16-byte grid
    out.append(_case("splitk", "n150-s2-f32", "nt", 168, 150, 72, DMA4, DTYPES, splitk=2, out_f32=1))
    out.append(_case("splitk", "n330-s2-f32", "nt", 296, 330, 128, P8, (BF16,), splitk=2, out_f32=1))
    out.append(_case("splitk", "n330-s2-f32", "nt", 296, 330, 128, DMA8, (BF16,), splitk=2, out_f32=1))
    return out


def empty_slices(K, splitk, bk):
    nkt = -(-K // bk)
    per = -(-nkt // splitk)
    return (splitk - 1) * per >= nkt


def _batch():
    out = []
    for M, N, K in ((104, 104, 64), (104, 64, 104)):
        for lay in ("nt", "dg", "wg"):
            for defeat in ((), ("stridec",)):
                tag = "z3" + ("-stridec" if defeat else "")
                want = (DMA4, 128, tile4(N))   # AUTO: batched problems stay on the default loop
                out.append(_case("batch", tag, lay, M, N, K, AUTO, DTYPES, batch=3, defeat=defeat, want=want))
                for kern in loops(lay, N, K):
                    out.append(_case("batch", tag, lay, M, N, K, kern, (BF16,), batch=3, defeat=defeat))
    # the attention shapes are smaller than any tile: item 1 of a misaligned strideC on whole interior tiles as well
    for lay in ("nt", "dg", "wg"):
        for defeat in ((), ("stridec",)):
            tag = "z3-interior" + ("-stridec" if defeat else "")
            out.append(_case("batch", tag, lay, 168, 152, 64, DMA4, DTYPES, batch=3, defeat=defeat))
            for kern in loops(lay, 328, 64)[1:]:
                out.append(_case("batch", tag, lay, 296, 328, 64, kern, (BF16,), batch=3, defeat=defeat))
    return out


def _multi():
    """the eight-phase loop walking more than one item per workgroup (more than 256 items), and its empty split-K slices"""
    out = []
    for lay, M, N in (("nt", 300, 300), ("wg", 304, 296)):
        out.append(_case("multi", "z66", lay, M, N, 128, P8, (BF16,), batch=66, out_f32=int(lay == "wg")))
        out.append(_case("multi", "s66", lay, M, N, 4480, P8, (BF16,), splitk=66, out_f32=1, colsum=int(lay == "wg")))
    out.append(_case("multi", "z66-whole", "nt", 512, 512, 64, P8, (BF16,), batch=66, bias=1))
    return out


def p8_items(case):
    return (-(-case["M"] // 256)) * (-(-case["N"] // 256)) * max(case.get("batch", 1), case.get("splitk", 0))


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = _shapes() + _wgrad() + _epilogues() + _splitk() + _batch() + _multi()
        names = [c["name"] for c in _TABLE]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:5]
    return _TABLE


def select(family=None, kern=None, lay=None, pred=None):
    """[(case, dtype)] of the table, filtered"""
    out = []
    for c in table():
        if family is not None and c["family"] != family:
            continue
        if kern is not None and c["kern"] != kern:
            continue
        if lay is not None and c["lay"] != lay:
            continue
        if pred is not None and not pred(c):
            continue
        out.extend((c, dt) for dt in c["dts"])
    return out


# ---- the two fast-path predicates, transcribed ------------------------------------------------------------------------------------------
def addresses(prob):
    """byte addresses of the pointer fields when every buffer starts on a 16-byte boundary (torch's allocator gives 256)"""
    es = lambda name: prob["bufs"][name].element_size()
    return {f: 0x100000 + v[1] * es(v[0]) for f, v in prob["desc"].items() if isinstance(v, tuple)}


def fast_terms(prob, z=1):
    """the terms of gemm_epilogue_bf16's `fast` (gemm_kernels.h:599-613, split-K: :594) and p8_epi_matches (gemm_p8.hip:255-271) that
    speak about alignment -> {term: holds}; terms about absent operands are left out"""
    d, ad = prob["desc"], addresses(prob)
    al16 = lambda f: ad[f] % 16 == 0
    t = {}
    if d.get("splitk", 0) > 1:
        t["n4"] = d["N"] % 4 == 0
        t["partial_ptr"] = al16("partial")
        return t
    t["ldc"] = d["ldc"] % 8 == 0
    t["c_ptr"] = al16("C")
    if d["batch"] > 1:
        t["stridec"] = (d["strideC"] * z) % 8 == 0   # the eight-phase loop asks strideC % 8 == 0 outright
    if "bias" in d:
        t["bias_ptr"] = al16("bias")
    if "aux" in d:
        t["ldaux"] = d["ldaux"] % 8 == 0
        t["aux_ptr"] = al16("aux")
    if "residual" in d:
        t["ldr"] = d["ldr"] % 4 == 0
        t["res_ptr"] = al16("residual")
    return t


def has_interior_tile(case, dt):
    _, bm, bn = resolves_to(case, dt)
    return case["M"] >= bm and case["N"] >= bn


# ---- mutants of the statement: (name, which cases it must change) ------------------------------------------------------------------------
MUTANTS = [
    ("k_chunk", lambda c: True),
    ("row_drop", lambda c: not c.get("rowmap")),
    ("row_dup", lambda c: not c.get("rowmap")),
    ("col_drop", lambda c: True),
    ("col_dup", lambda c: True),
    ("trunc", lambda c: True),     # needs a bf16 output (checked by the test)
    ("bias_after", lambda c: c.get("bias") and c.get("epi", 0) in (EPI_GELU, EPI_QGELU)),
    ("alpha_bias", lambda c: c.get("bias") and c.get("alpha", 1.0) != 1.0),
    ("alpha_twice", lambda c: c.get("splitk", 0) > 1 and c.get("alpha", 1.0) != 1.0),
    ("rowscale_src", lambda c: c.get("rowscale") and c.get("rowmap")),
    ("res_src", lambda c: c.get("residual") and c.get("rowmap")),
    ("period", lambda c: c.get("rowmap")),
    ("dropped_written", lambda c: c.get("rowmap")),
    ("no_acc", lambda c: c.get("accumulate")),
    ("last_slice", lambda c: c.get("splitk", 0) > 1),
    ("batch_b0", lambda c: c.get("batch", 1) > 1),
    ("colsum_n", lambda c: c.get("colsum")),
]


def render(prob, mutant):
    """the output buffers a kernel with the mutant's mistake would leave"""
    exp = expected(prob, mutant)
    got = {n: exp[n][0] for n in exp}
    true = expected(prob)
    for n in ("partial", "colsum_partial"):  # a well-formed slab: all of the (mutated) statement in slice 0
        if n in prob["outs"]:
            src = "C" if n == "partial" else "colsum"
            buf = prob["bufs"][n].clone()
            off, sk = prob["desc"][n][1], prob["desc"]["splitk"]
            cnt = prob["desc"]["M"] * (prob["desc"]["N"] if n == "partial" else 1)
            buf[off: off + sk * cnt] = 0
            if exp[src][1].numel() == cnt:
                v = exp[src][2]
                if n == "partial" and prob["desc"].get("accumulate") and mutant != "no_acc":
                    v = v - ref_view(prob)["C"][0][true["C"][1]]
                buf[off: off + cnt] = v.float()
            got[n] = buf
    return got
