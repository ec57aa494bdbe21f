"""fp64 statement of the DINO loss kernels (esvit_amd/csrc/dino_loss.hip) that tests/test_dino_loss_{cpu,gpu}.py compare against,
the metrics they use, and the seeded inputs they share.  Everything here comes straight from the softmax / log_softmax formula of
the loss; nothing takes the (row_max, row_lse) hand-over or the `nterms * p_s - p_t` form of the kernel and of oracle/ops_ref.py.

Bounds: the fp32 allowance of a family (entry point / regime / dtype / row width) is 3x the worst delta against fp64 observed on the MI355X and
committed in profiles/dino_loss_parity_observed.jsonl (the rule of tests/golden_utils.record_parity); a family without a committed
record has the allowance 0, so a new case fails until it has been measured.  bf16 outputs get the derived elementwise bound
|got - ref| <= 2^-8 |ref| + a * rowmax|ref| with a the fp32 allowance of the same case.
"""
import json
import os
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "dino_loss_parity_observed.jsonl")

INV_ST = 1.0 / 0.1
TEACHER_TEMPS = (0.04, 0.07)
KS = (8, 1000, 2056, 4096)      # 1-2 threads; a partial first sweep; whole sweeps + one straggler vector; whole sweeps
ROWS = (1, 7, 37)
RT = 11
DTYPES = (torch.float32, torch.bfloat16)
# regime: (logit scale, centre scale, student shift, teacher + centre shift)
REGIMES = {"flat": (0.02, 0.02, 0.0, 0.0), "trained": (0.25, 0.05, 0.0, 0.0), "peaked": (1.0, 0.3, 0.0, 0.0),
           "shifted": (0.25, 0.05, 30.0, 20.0)}


def dt_name(dt):
    return {torch.float32: "fp32", torch.bfloat16: "bf16"}[dt]


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def ce_ref(s, t, center, tmatch, weights, inv_st, inv_tt):
    """-> (row_loss [Rs], ds [Rs, K]) in fp64 on the CPU.  q = softmax((t - c) inv_tt), logp = log_softmax(s inv_st),
    loss_r = sum_j w_rj (-q_{tmatch[r, j]} . logp_r), ds = d(sum_r loss_r) / ds by autograd.  tmatch [Rs, 2] with weights [Rs] (one per
    row) or [Rs, 4] with weights [Rs, 4] (one per term); an entry -1 is an absent term.  Inputs are widened exactly as stored."""
    s64 = s.detach().cpu().double().clone().requires_grad_(True)
    q = torch.softmax((t.detach().cpu().double() - center.detach().cpu().double().view(1, -1)) * inv_tt, 1)
    logp = torch.log_softmax(s64 * inv_st, 1)
    tm = tmatch.detach().cpu().long().view(s64.shape[0], -1)
    w = weights.detach().cpu().double()
    w = w.view(-1, 1).expand(-1, tm.shape[1]) if w.numel() == tm.shape[0] else w.view(tm.shape)
    rl = torch.zeros(s64.shape[0], dtype=torch.float64)
    for j in range(tm.shape[1]):
        live = tm[:, j] >= 0
        term = -(q[tm[:, j].clamp(min=0)] * logp).sum(1)
        rl = rl + torch.where(live, w[:, j] * term, torch.zeros_like(term))
    rl.sum().backward()
    return rl.detach(), s64.grad.clone()


def teacher_stats_ref(t, center, inv_temp):
    """-> (row_max, row_lse) of z = (t - c) inv_temp in fp64: max_k z, ln sum_k exp(z - max)"""
    z = (t.detach().cpu().double() - center.detach().cpu().double().view(1, -1)) * inv_temp
    mx = z.max(1).values
    return mx, torch.logsumexp(z, 1) - mx


def rowstat_fold_ref(st):
    """base-2 block pairs (m_j, sum 2^(z - m_j)) [R, nb, 2] -> natural-log (row_max, row_lse) in fp64"""
    st = st.detach().cpu().double()
    m, sm = st[..., 0], st[..., 1]
    M = m.max(1).values
    total = (sm * torch.exp2(m - M[:, None])).sum(1)
    return M * float(np.log(2.0)), torch.log(total)


def region_match_ref(sim, Tt, crop_id, cm_row, fill=-7):
    """plain loops over image, row and view: the first maximal index among the Tt teacher tokens of the view, -1 where the student
    row belongs to that view's own crop -> int32 [B * S, 2] (rows never written keep `fill`)"""
    B, S, _ = sim.shape
    v = sim.detach().cpu().double().tolist()
    crop, row = crop_id.cpu().tolist(), cm_row.cpu().tolist()
    out = [[fill, fill] for _ in range(B * S)]
    for b in range(B):
        for s in range(S):
            for iq in range(2):
                if crop[s] == iq:
                    res = -1
                else:
                    best, bj = None, 0
                    for j in range(Tt):
                        x = v[b][s][iq * Tt + j]
                        if best is None or x > best:
                            best, bj = x, j
                    res = iq * B * Tt + b * Tt + bj
                out[row[b * S + s]][iq] = res
    return torch.tensor(out, dtype=torch.int32)


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
def has_term(tmatch):
    return (tmatch.cpu().view(tmatch.shape[0], -1) >= 0).any(1)


def per_row_rel(got, ref, rows=None):
    """max over the rows that have a term of max_k |got - ref| / max_k |ref|"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if ref.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return ((got - ref).abs().max(1).values / ref.abs().max(1).values).max().item()


def per_row_loss_rel(got, ref, rows=None):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if ref.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return ((got - ref).abs() / ref.abs()).max().item()


def bf16_excess(got, ref, a, rows=None):
    """the worst |got - ref| / (2^-8 |ref| + a rowmax|ref|) over the elements of the rows that have a term: <= 1 passes"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if ref.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), "non-finite output"
    bound = 2.0 ** -8 * ref.abs() + a * ref.abs().max(1, keepdim=True).values
    return ((got - ref).abs() / bound).max().item()


def stat_err(got, ref):
    """max |got - ref| / max(1, |ref|)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return ((got - ref).abs() / ref.abs().clamp(min=1.0)).max().item()


def sum_rel(ds, tmatch, weights, inv_st):
    """|sum_k ds[r, k]| / (w_r inv_st nterms): both softmaxes of a row sum to one (two-term tables, rows that have a term)"""
    tm = tmatch.cpu().view(tmatch.shape[0], -1)
    n = (tm >= 0).sum(1).double()
    rows = n > 0
    tot = ds.detach().cpu().double().sum(1).abs()
    return (tot[rows] / (weights.cpu().double()[rows] * inv_st * n[rows])).max().item() if bool(rows.any()) else 0.0


_OBSERVED = None


def observed():
    """{family: {metric: worst committed value}} of profiles/dino_loss_parity_observed.jsonl"""
    global _OBSERVED
    if _OBSERVED is None:
        _OBSERVED = {}
        if os.path.exists(PROFILE):
            with open(PROFILE) as fh:
                for line in fh:
                    if line.strip():
                        rec = json.loads(line)
                        fam = _OBSERVED.setdefault(rec["family"], {})
                        for k, v in rec.items():
                            if isinstance(v, float):
                                fam[k] = max(fam.get(k, 0.0), v)
    return _OBSERVED


def family(entry, regime, dt, K):
    """the unit a bound is measured for: entry point / regime / dtype / row width (a narrow row of the peaked regime can have a
    student and a teacher softmax that nearly cancel, which conditions the per-row metric far worse than at the other widths)"""
    return "%s/%s/%s/K%d" % (entry, regime, dt_name(dt), K)


def bound(family, metric):
    """3x the worst value committed for the family (0 if it was never measured: the case then fails until it has been)"""
    return 3.0 * observed().get(family, {}).get(metric, 0.0)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    """a generator seeded by the case's name (independent of the order in which cases are built)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()) % (2 ** 31))


def logits(regime, Rs, Rt, K, dt, seed=0):
    """-> (s [Rs, K], t [Rt, K] stored as dt, centre fp32 [1, K]) on the CPU"""
    scale, cscale, s_shift, t_shift = REGIMES[regime]
    g = _gen("logits", regime, Rs, Rt, K, seed)
    s = (torch.randn(Rs, K, generator=g) * scale + s_shift).to(dt)
    t = (torch.randn(Rt, K, generator=g) * scale + t_shift).to(dt)
    c = torch.randn(1, K, generator=g) * cscale + t_shift
    return s, t, c


def place(x, cols, rows=None, center=None):
    """a copy of x in which the maximum of each row (of x - center when given) sits at column cols (one int, or one per row):
    a quarter of the row's range above its old maximum; `rows` restricts it to some rows"""
    out = x.clone()
    f = x.float() - (0.0 if center is None else center.view(1, -1))
    R = x.shape[0]
    cols = [cols] * R if isinstance(cols, int) else list(cols)
    for r in (range(R) if rows is None else rows):
        top = f[r].max() + 0.25 * (f[r].max() - f[r].min()) + 1e-3
        out[r, cols[r]] = (top + (0.0 if center is None else center.view(-1)[cols[r]])).to(x.dtype)
    return out


def straggler_col(K, dt):
    """the first column of the vector a thread takes in its last, partial sweep of the 256-thread loop (1024 columns per sweep in
    fp32, 2048 in bf16); with a single partial sweep, the first column of the row's last vector"""
    sweep = 256 * (4 if dt == torch.float32 else 8)
    c = (K - 1) // sweep * sweep
    return c if c > 0 else K - (4 if dt == torch.float32 else 8)


def two_term_tables(Rs, Rt, seed=0, split=False):
    """tmatch int32 [Rs, 2] cycling through (a, b), (a, -1), (-1, b), (-1, -1), with rows that have a == b and a third of the rows
    sharing teacher row 0; weights fp32 [Rs] in 0.01 .. 0.1.  split: a is drawn from the even teacher rows, b from the odd ones."""
    g = _gen("tables2", Rs, Rt, seed)
    a = torch.randint(0, Rt, (Rs,), generator=g)
    b = torch.randint(0, Rt, (Rs,), generator=g)
    if split:
        a, b = a // 2 * 2, (b // 2 * 2 + 1).clamp(max=Rt - 1 - (Rt % 2))
    else:
        b[8::12] = a[8::12]          # a == b
        a[::3] = 0                   # many rows against one teacher row
    tm = torch.stack([a, b], 1).to(torch.int32)
    r = torch.arange(Rs)
    tm[(r % 4 == 2) | (r % 4 == 3), 0] = -1
    tm[(r % 4 == 1) | (r % 4 == 3), 1] = -1
    w = (0.01 + 0.09 * torch.rand(Rs, generator=g)).float()
    return tm.contiguous(), w


def four_term_tables(Rs, Rt, seed=0):
    """tmatch int32 [Rs, 4] with 0 .. 4 live terms per row, weights fp32 [Rs, 4] in 0.01 .. 0.7; row 5 has a live entry of weight
    zero, rows 6 and 7 name one teacher row twice, row 4 (r % 5 == 4) has no live term"""
    g = _gen("tables4", Rs, Rt, seed)
    tm = torch.randint(0, Rt, (Rs, 4), generator=g).to(torch.int32)
    tw = (0.01 + 0.69 * torch.rand(Rs, 4, generator=g)).float()
    for r in range(Rs):
        live = (r + 1) % 5  # 1, 2, 3, 4, 0 live terms
        dead = torch.randperm(4, generator=g)[:4 - live]
        tm[r, dead] = -1
    tm[5] = torch.tensor([1, 2, -1, -1], dtype=torch.int32)
    tw[5, 1] = 0.0
    tm[6] = torch.tensor([3, 3, -1, 4], dtype=torch.int32)
    tm[7] = torch.tensor([-1, 2, 5, 2], dtype=torch.int32)
    return tm.contiguous(), tw.contiguous()


def mixup_tables():
    """the [ncrops * B, 4] tables esvit_amd.loss.DINOLoss._mixup_terms makes of golden_utils.mixup_case() -> (tmatch, weights, B, ncrops)"""
    from esvit_amd.loss import DINOLoss
    from tests import golden_utils as GU
    mc = GU.MIXUP
    T = GU.mixup_case()[3]
    tm, tw, off = DINOLoss(mc["K"], mc["ncrops"], 0.04, 0.07, 5, 10)._mixup_terms(T, mc["B"], torch.device("cpu"))
    assert float(off.abs().max()) == 0.0
    return tm, tw, mc["B"], mc["ncrops"]


def two_term_cases(regime, K, dt):
    """the two-term sweep of one (regime, K, dtype): rows x teacher temperatures, and for K in {1000, 2056} of the trained regime
    the row maxima of s, of the teacher rows of slot 0 and of slot 1 placed at column 0, K - 1 and the straggler vector"""
    out = []
    for Rs in ROWS:
        for tt in TEACHER_TEMPS:
            s, t, c = logits(regime, Rs, RT, K, dt)
            tm, w = two_term_tables(Rs, RT)
            out.append(dict(name="R%d_tt%g" % (Rs, tt), s=s, t=t, c=c, tm=tm, w=w, inv_tt=1.0 / tt, placed=None))
    if regime == "trained" and K in (1000, 2056):
        s, t, c = logits(regime, 37, RT, K, dt, seed=1)
        tm, w = two_term_tables(37, RT, seed=1, split=True)
        for col, cname in ((0, "first"), (K - 1, "last"), (straggler_col(K, dt), "straggler")):
            for what in ("s", "ta", "tb"):
                s2 = place(s, col) if what == "s" else s
                t2 = t if what == "s" else place(t, col, rows=range(0 if what == "ta" else 1, RT, 2), center=c)
                out.append(dict(name="place_%s_%s" % (what, cname), s=s2, t=t2, c=c, tm=tm, w=w, inv_tt=1.0 / 0.04, placed=(what, col)))
    return out


def four_term_cases(regime, K, dt):
    out = []
    tm_m, tw_m, B, nc = mixup_tables()
    for name, (tm, tw), Rt in (("crafted", four_term_tables(24, 12), 12), ("mixup", (tm_m, tw_m), 2 * B)):
        for tt in TEACHER_TEMPS:
            s, t, c = logits(regime, tm.shape[0], Rt, K, dt, seed=2)
            out.append(dict(name="%s_tt%g" % (name, tt), s=s, t=t, c=c, tm=tm, w=tw, inv_tt=1.0 / tt))
    return out


def rowstat_blocks(R, nb, where, seed=0):
    """synthetic statistics of the last-layer GEMM: [R, nb, 2] fp32 pairs (block maximum in base-2 units, sum 2^(z - max) of its up to
    64 columns, so 1 .. 64).  A third of the blocks lie 200 units below (they contribute nothing); the row maximum is put in block
    `where` (negative: from the end; clipped to nb - 1)."""
    g = _gen("rowstat", R, nb, where, seed)
    m = torch.randn(R, nb, generator=g) * 6.0 + 20.0
    m[torch.rand(R, nb, generator=g) < 0.33] -= 200.0
    j = min(where, nb - 1) if where >= 0 else max(nb + where, 0)
    m[:, j] = m.max(1).values + 1.0 + torch.rand(R, generator=g)
    sm = 1.0 + 63.0 * torch.rand(R, nb, generator=g)
    return torch.stack([m, sm], -1).float().contiguous()


# ---- region matching ---------------------------------------------------------------------------------------------------------------
REGION_LAYOUTS = {  # name: (B, ncrops, s_npatch, Tt)
    "b3_49_9": (3, 10, [49, 9], 49),   # S = 170: 1020 work items (not a multiple of 128); ld = 104 with 6 padding columns
    "b1_tt1": (1, 10, [1, 1], 1),      # the smallest legal case
    "b2_tt36": (2, 10, [36, 4], 36),   # ld = 72 = 2 Tt: no padding
}
REGION_KINDS = ("random", "negative", "win_first", "win_last", "tie2", "tie_all")
PAD = 1.0e30


def region_tables(layout):
    from esvit_amd.loss import DDINOLoss
    B, nc, s_np, Tt = REGION_LAYOUTS[layout]
    tb = DDINOLoss(8, nc, 0.04, 0.04, 0, 1)._static(B, s_np, Tt, torch.device("cpu"))
    return B, tb["S"], Tt, -(-2 * Tt // 8) * 8, tb["crop_id"], tb["cm_row"]


def region_sim(layout, kind):
    """-> (sim fp32 [B, S, ld], ties): per (row, view) a random order of Tt distinct multiples of 1/256 (top-2 gap 3.9e-3, exact in
    fp32); the padding columns hold +1e30.  ties = number of indices that share the maximum per (row, view) (1 = no tie)."""
    B, S, Tt, ld, _, _ = region_tables(layout)
    g = _gen("region", layout, kind)
    order = torch.rand(B, S, 2, Tt, generator=g).argsort(-1).float()          # a permutation of 0 .. Tt-1 per (row, view)
    v = order / 256.0 - 0.05
    ties = 1
    if kind == "negative":
        v = v - 1.0
    elif kind in ("win_first", "win_last"):
        j = 0 if kind == "win_first" else Tt - 1
        top = v.max(-1).values
        at = v.argmax(-1, keepdim=True)
        v.scatter_(-1, at, v[..., j:j + 1].clone())
        v[..., j] = top
    elif kind == "tie2" and Tt >= 2:
        j1, j2 = Tt // 3, Tt - 1
        top = v.max(-1).values + 1.0 / 256.0
        v[..., j1] = top
        v[..., j2] = top
        ties = 2
    elif kind == "tie_all":
        v = torch.full_like(v, 0.125)
        ties = Tt
    sim = torch.full((B, S, ld), PAD)
    sim[:, :, :2 * Tt] = v.reshape(B, S, 2 * Tt)
    return sim.contiguous(), ties


def top2_gap_and_ties(sim, Tt):
    """-> (smallest top-2 gap, (min, max) number of maximal indices) over every (row, view), in fp64"""
    B, S, _ = sim.shape
    v = sim[:, :, :2 * Tt].double().reshape(B, S, 2, Tt)
    top = v.max(-1, keepdim=True).values
    n = (v == top).sum(-1)
    gap = float("inf") if Tt < 2 else (lambda k: (k[..., 0] - k[..., 1]).min().item())(v.topk(2, -1).values)
    return gap, (int(n.min()), int(n.max()))


# ---- module level ------------------------------------------------------------------------------------------------------------------
MODULE = dict(B=3, ncrops=10, s_npatch=[49, 9], D=32)


def module_case(K, dt, seed=3):
    """trained-regime inputs of DDINOLoss / DINOLoss: logits stored as dt, nonzero centres, and region features with a clear winner
    in both views: each student token is the sum of one chosen unit teacher token per view plus noise of scale 0.02; token 0 of
    every crop aims at teacher tokens 0 and Tt - 1"""
    B, nc, (Tt, Ts), D = MODULE["B"], MODULE["ncrops"], MODULE["s_npatch"], MODULE["D"]
    g = _gen("module_features", seed)
    sizes = [Tt] * 2 + [Ts] * (nc - 2)
    S = sum(sizes)
    rn = lambda *shape, sc=1.0: torch.randn(*shape, generator=g) * sc  # noqa: E731
    t_fea = rn(2 * B * Tt, D)
    unit = torch.nn.functional.normalize(t_fea, dim=-1).view(2, B, Tt, D)
    rows = []
    for sz in sizes:
        j0, j1 = torch.randint(0, Tt, (B, sz), generator=g), torch.randint(0, Tt, (B, sz), generator=g)
        j0[:, 0], j1[:, 0] = 0, Tt - 1
        f = torch.stack([unit[0, b][j0[b]] + unit[1, b][j1[b]] for b in range(B)])
        rows.append((f + rn(B, sz, D, sc=0.02)).reshape(B * sz, D))
    s_fea = torch.cat(rows)
    g = _gen("module_logits", K, seed)
    return dict(s_cls=rn(nc * B, K, sc=0.25).to(dt), s_reg=rn(B * S, K, sc=0.25).to(dt), t_cls=rn(2 * B, K, sc=0.25).to(dt),
                t_reg=rn(2 * B * Tt, K, sc=0.25).to(dt), s_fea=s_fea, t_fea=t_fea, center=rn(1, K, sc=0.05), center_grid=rn(1, K, sc=0.05),
                npatch=[Tt, Ts], sizes=sizes, S=S, B=B, Tt=Tt)


def module_gap(case):
    """the smallest top-2 gap of the fp64 cosine similarities over every (student token, view)"""
    F = torch.nn.functional
    B, Tt = case["B"], case["Tt"]
    sfn = F.normalize(case["s_fea"].double(), dim=-1)
    tfn = F.normalize(case["t_fea"].double(), dim=-1).view(2, B, Tt, -1)
    off, gaps = 0, []
    for sz in case["sizes"]:
        x = sfn[off:off + B * sz].view(B, sz, -1)
        off += B * sz
        for iq in range(2):
            top = torch.einsum("bsd,btd->bst", x, tfn[iq]).topk(2, -1).values
            gaps.append((top[..., 0] - top[..., 1]).min().item())
    return min(gaps)


def module_ref(case, which, temp=0.04):
    """fp64 loss, gradients and updated centres of esvit_oracle.ddino_loss / dino_loss on the logits as stored"""
    from oracle import esvit_oracle as O
    nc, B, Tt = MODULE["ncrops"], case["B"], case["Tt"]
    d = lambda k: case[k].double()  # noqa: E731
    sc = d("s_cls").requires_grad_(True)
    if which == "ddino":
        sr = d("s_reg").requires_grad_(True)
        loss, bc, bg = O.ddino_loss((sc, sr, d("s_fea"), case["npatch"]), (d("t_cls"), d("t_reg"), d("t_fea"), case["npatch"]),
                                    d("center"), d("center_grid"), temp, nc)
        loss.backward()
        return dict(loss=loss.item(), g_cls=sc.grad, g_reg=sr.grad, center=O.center_update(d("center"), bc, 2 * B),
                    center_grid=O.center_update(d("center_grid"), bg, 2 * B * Tt))
    loss, bc = O.dino_loss(sc, d("t_cls"), d("center"), temp, nc)
    loss.backward()
    return dict(loss=loss.item(), g_cls=sc.grad, center=O.center_update(d("center"), bc, 2 * B))


def run_module(case, which, dev, dt):
    """the package's DDINOLoss / DINOLoss on `dev` -> the same dict as module_ref (tensors on the CPU)"""
    import esvit_amd
    K = case["center"].shape[1]
    to = lambda k: case[k].to(dev)  # noqa: E731
    cls_ = esvit_amd.DDINOLoss if which == "ddino" else esvit_amd.DINOLoss
    lf = cls_(K, MODULE["ncrops"], 0.04, 0.04, 0, 1).to(dev)
    lf.center.copy_(to("center"))
    sc = to("s_cls").requires_grad_(True)
    if which == "ddino":
        lf.center_grid.copy_(to("center_grid"))
        sr = to("s_reg").requires_grad_(True)
        loss = lf((sc, sr, to("s_fea"), case["npatch"]), (to("t_cls"), to("t_reg"), to("t_fea"), case["npatch"]), 0, None)
    else:
        loss = lf(sc, to("t_cls"), 0, None)
    loss.backward()
    lf.synchronize()
    out = dict(loss=loss.item(), g_cls=sc.grad.cpu(), center=lf.center.cpu())
    if which == "ddino":
        out.update(g_reg=sr.grad.cpu(), center_grid=lf.center_grid.cpu())
    return out


# ---- drivers shared by the CPU run (oracle/ops_ref.py, the restatement) and the GPU run (esvit_amd.ops, the kernels) -------------------
def _stats_from(o, kind, t, c, inv_tt, dev):
    """teacher statistics from the library itself (the hand-over of a training step) or from the fp64 reference rounded to fp32"""
    if kind == "ops":
        return o.teacher_row_stats(t, c, inv_tt)
    mx, lse = teacher_stats_ref(t, c, inv_tt)
    return mx.float().to(dev), lse.float().to(dev)


def eval_two_term(o, dev, regime, K, dt, center_mutation=None):
    """every two-term case of (regime, K, dt) through o.dino_ce -> {metric: worst value over the cases}, per-case lines, and the
    exact properties as a list of failures.  center_mutation(c) -> the centre the CE pass sees (the CPU mutation check)."""
    worst, lines, broken = {}, [], []
    for case in two_term_cases(regime, K, dt):
        s, t, c, tm, w = (case[k].to(dev) for k in ("s", "t", "c", "tm", "w"))
        rl64, ds64 = ce_ref(case["s"], case["t"], case["c"], case["tm"], case["w"], INV_ST, case["inv_tt"])
        rows = has_term(case["tm"])
        for kind in ("ops", "ref"):
            mx, lse = _stats_from(o, kind, t, c, case["inv_tt"], dev)
            c_ce = c if center_mutation is None else center_mutation(c)
            rl, ds = o.dino_ce(s, t, c_ce, mx, lse, tm, w, INV_ST, case["inv_tt"])
            m = dict(loss_rel=per_row_loss_rel(rl, rl64, rows))
            if dt == torch.float32:
                m["ds_rel"] = per_row_rel(ds, ds64, rows)
                m["sum_rel"] = sum_rel(ds, case["tm"], case["w"], INV_ST)
            else:
                m["ds_bf16_excess"] = bf16_excess(ds, ds64, bound(family("dino_ce2", regime, torch.float32, K), "ds_rel"), rows)
            lines.append(dict(case="%s_%s" % (case["name"], kind), **m))
            for k, v in m.items():
                worst[k] = max(worst.get(k, 0.0), v)
            # a row without a term: exactly zero
            if bool((~rows).any()) and not (bool((ds.cpu()[~rows] == 0).all()) and bool((rl.cpu()[~rows] == 0).all())):
                broken.append("%s: a row without a term is not exactly zero" % case["name"])
        if case["placed"] is None and case["name"].endswith("tt0.04"):
            mx, lse = _stats_from(o, "ops", t, c, case["inv_tt"], dev)
            rl, ds = o.dino_ce(s, t, c, mx, lse, tm, w, INV_ST, case["inv_tt"])
            # a one-term row: the same bits whether the term sits in slot 0 or in slot 1
            tm_sw = case["tm"].clone()
            one = ((case["tm"] >= 0).sum(1) == 1)
            tm_sw[one] = case["tm"][one].flip(1)
            rl2, ds2 = o.dino_ce(s, t, c, mx, lse, tm_sw.contiguous().to(dev), w, INV_ST, case["inv_tt"])
            if not (torch.equal(rl2, rl) and torch.equal(ds2, ds)):
                broken.append("%s: a one-term row depends on the slot of its term" % case["name"])
            # a random work order changes nothing
            order = torch.randperm(s.shape[0], generator=_gen("order", case["name"])).to(torch.int32).to(dev)
            rl3, ds3 = o.dino_ce(s, t, c, mx, lse, tm, w, INV_ST, case["inv_tt"], row_order=order)
            if not (torch.equal(rl3, rl) and torch.equal(ds3, ds)):
                broken.append("%s: row_order changes the result" % case["name"])
    return worst, lines, broken


def eval_four_term(o, dev, regime, K, dt):
    worst, lines, broken = {}, [], []
    for case in four_term_cases(regime, K, dt):
        s, t, c, tm, tw = (case[k].to(dev) for k in ("s", "t", "c", "tm", "w"))
        rl64, ds64 = ce_ref(case["s"], case["t"], case["c"], case["tm"], case["w"], INV_ST, case["inv_tt"])
        rows = ((case["tm"] >= 0) & (case["w"] != 0)).any(1)   # (a live entry of weight zero contributes nothing)
        dead = ~has_term(case["tm"])
        mx, lse = o.teacher_row_stats(t, c, case["inv_tt"])
        rl, ds = o.dino_ce(s, t, c, mx, lse, tm, None, INV_ST, case["inv_tt"], term_w=tw)
        m = dict(loss_rel=per_row_loss_rel(rl, rl64, rows))
        if dt == torch.float32:
            m["ds_rel"] = per_row_rel(ds, ds64, rows)
        else:
            m["ds_bf16_excess"] = bf16_excess(ds, ds64, bound(family("dino_ce4", regime, torch.float32, K), "ds_rel"), rows)
        lines.append(dict(case=case["name"], **m))
        for k, v in m.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if bool(dead.any()) and not (bool((ds.cpu()[dead] == 0).all()) and bool((rl.cpu()[dead] == 0).all())):
            broken.append("%s: a row without a live term is not exactly zero" % case["name"])
    return worst, lines, broken


STAT_ROWS = (1, 11)


def eval_teacher_stats(o, dev, regime, K, dt):
    worst = {}
    for R in STAT_ROWS:
        for tt in TEACHER_TEMPS:
            _, t, c = logits(regime, 1, R, K, dt, seed=4)
            mx, lse = o.teacher_row_stats(t.to(dev), c.to(dev), 1.0 / tt)
            mx64, lse64 = teacher_stats_ref(t, c, 1.0 / tt)
            m = dict(max_err=stat_err(mx, mx64), lse_err=stat_err(mx.double().cpu() + lse.double().cpu(), mx64 + lse64))
            for k, v in m.items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst


ROWSTAT_R = (1, 5, 128)
ROWSTAT_NB = (1, 63, 64, 65, 1024)
ROWSTAT_WHERE = (0, -1, 64)


def eval_rowstat(o, dev, R, nb):
    worst = {}
    for where in ROWSTAT_WHERE:
        st = rowstat_blocks(R, nb, where)
        mx, lse = o.rowstat_combine(st.to(dev))
        mx64, lse64 = rowstat_fold_ref(st)
        m = dict(max_err=stat_err(mx, mx64), lse_err=stat_err(mx.double().cpu() + lse.double().cpu(), mx64 + lse64))
        for k, v in m.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


CENTER_SHAPES = ((22, 1000, torch.float32), (22, 1000, torch.bfloat16), (294, 72, torch.float32))


def eval_center_chain(o, dev, rows, K, dt, momentum=0.9):
    g = _gen("center", rows, K, dt)
    t = (torch.randn(rows, K, generator=g) * 0.25 + 0.1).to(dt)
    c = torch.randn(1, K, generator=g) * 0.05
    got = o.center_ema(c.clone().to(dev), o.colsum(t.to(dev)), momentum, rows)
    want = c.double() * momentum + t.double().mean(0, keepdim=True) * (1 - momentum)
    return dict(center_rel=((got.cpu().double() - want).abs().max() / want.abs().max()).item())


def eval_module(which, K, dt, dev):
    case = module_case(K, dt)
    ref = module_ref(case, which)
    got = run_module(case, which, dev, dt)
    fam32 = family("module_" + which, "trained", torch.float32, K)
    m = dict(loss_rel=abs(got["loss"] - ref["loss"]) / abs(ref["loss"]))
    for k in ("center", "center_grid"):
        if k in ref:
            m[k + "_rel"] = ((got[k].double() - ref[k]).abs().max() / ref[k].abs().max()).item()
    for k in ("g_cls", "g_reg"):
        if k in ref:
            rows = ref[k].abs().max(1).values > 0
            if dt == torch.float32:
                m[k + "_rel"] = per_row_rel(got[k], ref[k], rows)
            else:
                m[k + "_bf16_excess"] = bf16_excess(got[k], ref[k], bound(fam32, k + "_rel"), rows)
            if bool((~rows).any()) and not bool((got[k][~rows] == 0).all()):
                m[k + "_nonzero_dead_rows"] = 1.0
    return m


def check(family, metrics, record=None, case=None, floor=0.0):
    """record the observed metrics, then assert each against 3x the committed value of its family (bf16 excess: <= 1).  floor: the
    CPU run of the restatement passes a few fp32 roundings here -- see tests/test_dino_loss_cpu.py"""
    if record is not None:
        record(test="dino_loss", family=family, case=case, **metrics)
    print("OBSERVED", family, case, json.dumps(metrics))
    bad = []
    for k, v in metrics.items():
        lim = 1.0 if k.endswith("_bf16_excess") else (0.0 if k.endswith("_nonzero_dead_rows") else max(bound(family, k), floor))
        if not v <= lim:
            bad.append("%s %s: %.3e > %.3e" % (family, k, v, lim))
    assert not bad, bad
