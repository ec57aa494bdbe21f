"""fp64 statement of the training-health monitor (esvit_amd/monitor.py, esvit_amd/csrc/monitor.hip) that tests/test_monitor_{cpu,gpu}.py
compare against, with the bounds they use.  Plain torch on inputs widened exactly as stored (the inverse temperature is the fp32 the
C ABI takes); the statistics are the reference's own (dino_loss_ref.teacher_stats_ref), the code under test receives them rounded to
fp32.  The entropy is stated twice -- in the centred form H = L - sum p d and in the textbook form -sum p ln p -- and the two must
agree to 1e-12.

Bounds, with u = 2^-24, d = z - max, L = lse, p = exp(d - L) and the per-row scale
    S_r = |L| + |max| + max_k |z_k| + sum_k p_k |d_k| (1 + |d_k|):
  entropy          |ent - ref| <= 16 u S_r.  The yardstick is the plain fp32 torch evaluation of the same formula on the CPU (at or
                   below 0.91 u S_r over the four regimes, K in {8, 2056, 4096, 65536}, both dtypes, inverse temperatures 25, 14.3,
                   10); the factor 16 is headroom -- a judgment, not a derivation -- for the kernel's other summation tree (some 50
                   levels at K = 65536) and the hardware exp2 (1 ulp).  The bound itself stays below 1e-3 nats on the whole table.
  column sums      |psum_k - ref| <= 16 u sum_r p_rk (2 + |z_rk| + |max_r| + |L_r| + |d_rk - L_r|) + 1e-37.
                   WIDENED SCALE: the scale first proposed, sum_r p_rk (2 + |d_rk - L_r|), leaves out that the statistics arrive
                   rounded to fp32 (max to u |max|, which moves every p of the row by that much, relatively) and that z itself is
                   rounded at u |z|: the winning logit of a peaked row (d = 0, L ~ 0, |z| = |max| = 145) is then allowed 32 u while fp32
                   torch is off by up to 145 u there (test_monitor_cpu.test_fp32_torch_sits_under_an_eighth_of_the_bounds measures
                   both scales).  The constant stays 16; the scale gains |z| + |max| + |L|.  The absolute term is for columns whose
                   probabilities underflow.
  marginal entropy propagated from the column-sum bound: sum_k |dpbar_k| (1 + |ln pbar_k|), pbar = psum / R.
  argmax           exact: inputs have the row maximum placed (dino_loss_ref.place) a quarter of the row's range above the rest.
"""
import math
import os

import numpy as np
import torch

from tests import dino_loss_ref as DR
from tests.dino_loss_ref import MODULE, REGIMES, logits, place, teacher_stats_ref  # noqa: F401  (shared, unchanged)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "monitor_parity_observed.jsonl")

U = 2.0 ** -24
ENT_FACTOR = 16.0
INV_TEMPS = (25.0, 14.3, 10.0)


def f32(v):
    """the fp32 value the C ABI receives for a Python float"""
    return float(np.float32(v))


# ---- the streaming kernel's three outputs ------------------------------------------------------------------------------------------
def dist_ref(x, center, inv_temp, stats=None, entropy="centred", argmax="first", drop_center=False):
    """fp64 (ent [R], amax [R], psum [K]) and the bounds' scales of p = softmax((x - c) inv_temp).  stats: (max, lse) to use in place
    of the rows' own (the 'statistics of another row' mutant); entropy: 'centred' (L - sum p d), 'textbook' (-sum p ln p) or the
    mutant 'uncentred' (evaluated as the fp32 kernel would: max + L - sum p z with the products rounded to fp32); argmax: 'first' or
    the mutant 'last'; drop_center: the mutant that forgets the centre."""
    x64 = x.detach().cpu().double()
    c64 = torch.zeros(x64.shape[1], dtype=torch.float64) if (center is None or drop_center) else center.detach().cpu().double().view(-1)
    inv = f32(inv_temp)
    z = (x64 - c64.view(1, -1)) * inv
    mx, L = stats if stats is not None else (z.max(1).values, None)
    if L is None:
        L = torch.logsumexp(z, 1) - mx
    mx, L = mx.double(), L.double()
    d = z - mx[:, None]
    lnp = d - L[:, None]
    p = torch.exp(lnp)
    if entropy == "centred":
        ent = L - (p * d).sum(1)
    elif entropy == "textbook":
        ent = -(p * lnp).sum(1)
    else:  # what forming sum p z costs in fp32 when |max| is large: every product carries an error of u |p z|
        ent = (mx + L).float().double() - (p.float() * z.float()).sum(1).double()
    top = z == z.max(1, keepdim=True).values
    K = z.shape[1]
    amax = top.double().argmax(1) if argmax == "first" else K - 1 - top.flip(1).double().argmax(1)
    S = L.abs() + mx.abs() + z.abs().max(1).values + (p * d.abs() * (1 + d.abs())).sum(1)
    col_scale = (p * (2 + z.abs() + mx.abs()[:, None] + L.abs()[:, None] + lnp.abs())).sum(0)
    col_scale_narrow = (p * (2 + lnp.abs())).sum(0)
    return dict(ent=ent, amax=amax.to(torch.int64), psum=p.sum(0), S=S, col_scale=col_scale, col_scale_narrow=col_scale_narrow, max=mx, lse=L)


def ent_bound(ref):
    return ENT_FACTOR * U * ref["S"]


def psum_bound(ref, narrow=False):
    return ENT_FACTOR * U * ref["col_scale_narrow" if narrow else "col_scale"] + 1e-37


def marginal_entropy(psum, R):
    pbar = psum.double() / R
    return -torch.xlogy(pbar, pbar).sum()


def marginal_bound(ref, R, narrow=False):
    pbar = ref["psum"] / R
    dp = psum_bound(ref, narrow) / R
    return (dp * (1 + torch.log(pbar.clamp(min=1e-300)).abs())).sum()


def stats_f32(ref):
    return ref["max"].float(), ref["lse"].float()


def ratios(ent, amax, psum, ref, R):
    """observed error / bound of one call -> dict; argmax mismatches counted"""
    ent, psum = ent.detach().cpu().double(), psum.detach().cpu().double()
    return dict(ent=((ent - ref["ent"]).abs() / ent_bound(ref)).max().item(),
                psum=((psum - ref["psum"]).abs() / psum_bound(ref)).max().item(),
                marg=((marginal_entropy(psum, R) - marginal_entropy(ref["psum"], R)).abs() / marginal_bound(ref, R)).item(),
                amax_wrong=int((amax.detach().cpu().long() != ref["amax"]).sum()),
                ent_abs=(ent - ref["ent"]).abs().max().item(), ent_bound_max=ent_bound(ref).max().item())


def case(regime, R, K, dt, inv_temp, col=None, seed=0, centered=True):
    """seeded rows of a regime with each row's maximum placed at column `col` (default: a seeded column per row) -> (x, centre)"""
    _, t, c = logits(regime, 1, R, K, dt, seed=seed)
    if not centered:
        c = None
    g = DR._gen("monitor_cols", regime, R, K, seed)
    cols = torch.randint(0, K, (R,), generator=g).tolist() if col is None else col
    return place(t, cols, center=c), (None if c is None else c.view(-1).contiguous())


# ---- module level: every quantity of TrainingMonitor in fp64 -------------------------------------------------------------------------
def _level_ref(out, sfx, t, c, inv_tt, s, inv_st, tm, w, student, count_absent=False):
    ref = dist_ref(t, c, inv_tt)
    R = t.shape[0]
    out["teacher_entropy" + sfx] = ref["ent"].mean().item()
    out["teacher_marginal_entropy" + sfx] = marginal_entropy(ref["psum"], R).item()
    out["teacher_pmax" + sfx] = torch.exp(-ref["lse"]).mean().item()
    # KL(q || p_s) per (student row, live term), from the two distributions themselves
    q = torch.softmax((t.double() - c.double().view(1, -1)) * f32(inv_tt), 1)
    logp = torch.log_softmax(s.double() * f32(inv_st), 1)
    tm = tm.view(s.shape[0], -1).long()
    w = w.double()
    w = w.view(-1, 1).expand(-1, tm.shape[1]) if w.numel() == tm.shape[0] else w.view(tm.shape)
    num = den = 0.0
    for j in range(tm.shape[1]):
        live = tm[:, j] >= 0
        qj = q[tm[:, j].clamp(min=0)]
        kl = (qj * (torch.log(qj.clamp(min=1e-300)) - logp)).sum(1)
        if count_absent:  # mutant: an absent term (-1) read as teacher row 0
            live = torch.ones_like(live)
        num = num + (w[:, j] * kl)[live].sum()
        den = den + w[:, j][live].sum()
    out["kl" + sfx] = (num / den).item()
    out["center_absmax" + sfx] = c.double().abs().max().item()
    if student:
        out["student_entropy" + sfx] = dist_ref(s, None, inv_st)["ent"].mean().item()
    out["_S" + sfx] = ref["S"].mean().item()
    out["_marg_bound" + sfx] = marginal_bound(ref, R).item()
    out["_lse_abs" + sfx] = ref["lse"].abs().max().item()
    zs = s.double() * f32(inv_st)
    out["_S_student" + sfx] = dist_ref(s, None, inv_st)["S"].mean().item()
    out["_ce_scale" + sfx] = (torch.logsumexp(zs, 1).abs() + zs.abs().max(1).values).mean().item()
    return ref["amax"]


def match_ref(s_fea, t_fea, B, sizes, Tt, coverage_both_views=False):
    """fp64 region matching from the features: -> (tm_reg [B S, 2] crop-major, match_similarity, match_coverage)"""
    F = torch.nn.functional
    sfn = F.normalize(s_fea.double(), dim=-1)
    tfn = F.normalize(t_fea.double(), dim=-1).view(2, B, Tt, -1)
    tm, off, wins, shares = [], 0, [], []
    for v, sz in enumerate(sizes):
        x = sfn[off:off + B * sz].view(B, sz, -1)
        off += B * sz
        rows = torch.full((B, sz, 2), -1, dtype=torch.int64)
        sets = {}
        for iq in range(2):
            if v == iq:
                continue
            sim = torch.einsum("bsd,btd->bst", x, tfn[iq])
            top, j = sim.max(-1)
            rows[:, :, iq] = iq * B * Tt + torch.arange(B)[:, None] * Tt + j
            wins.append(top.reshape(-1))
            for b in range(B):
                sets[(b, iq)] = set(j[b].tolist())
        if coverage_both_views:  # mutant: the tokens matched in either view over the 2 Tt tokens of both
            for b in range(B):
                shares.append(sum(len(sets[(b, iq)]) for iq in range(2) if (b, iq) in sets) / (2.0 * Tt))
        else:
            shares += [len(st) / float(Tt) for st in sets.values()]
        tm.append(rows.view(B * sz, 2))
    return torch.cat(tm).to(torch.int32), torch.cat(wins).mean().item(), sum(shares) / len(shares)


def module_ref(mc, which, temp=0.04, inv_st=10.0, student=False, count_absent=False, coverage_both_views=False):
    """every key TrainingMonitor reports for one forward of DINOLoss ('dino') / DDINOLoss ('ddino') on dino_loss_ref.module_case
    inputs, in fp64; keys starting with '_' are the scales the tolerances are built from"""
    nc, B, Tt = MODULE["ncrops"], mc["B"], mc["Tt"]
    inv_tt = 1.0 / temp
    out = {}
    tm_cls = torch.full((nc * B, 2), -1, dtype=torch.int64)
    for v in range(nc):
        for iq in range(2):
            if v != iq:
                tm_cls[v * B:(v + 1) * B, iq] = iq * B + torch.arange(B)
    n_terms = 2 * nc - 2
    w_cls = torch.full((nc * B,), (1.0 if which == "dino" else 0.5) / (n_terms * B), dtype=torch.float64)
    amax = _level_ref(out, "", mc["t_cls"], mc["center"], inv_tt, mc["s_cls"], inv_st, tm_cls, w_cls, student, count_absent)
    out["view_agreement"] = (amax[:B] == amax[B:2 * B]).double().mean().item()
    if which == "ddino":
        tm_reg, sim_mean, cover = match_ref(mc["s_fea"], mc["t_fea"], B, mc["sizes"], Tt, coverage_both_views)
        w_reg = torch.cat([torch.full((B * sz,), 0.5 / (n_terms * B * sz), dtype=torch.float64) for sz in mc["sizes"]])
        _level_ref(out, "_grid", mc["t_reg"], mc["center_grid"], inv_tt, mc["s_reg"], inv_st, tm_reg, w_reg, student, count_absent)
        out["match_similarity"], out["match_coverage"] = sim_mean, cover
    return out


def module_tolerance(ref, key):
    """|got - ref| allowed for one key of TrainingMonitor.compute() against module_ref.  Means of row entropies: the mean of the rows'
    bounds.  teacher_pmax = mean exp(-L): L is known to 16 u (1 + |L|) relative.  kl = weighted mean of CE - H: the cross-entropy is
    an lse minus a probability-weighted sum of logits like the entropy itself, evaluated in fp32 with the scale |lse_s| + max |z_s|
    per row; the teacher entropies enter with their own bound.  match_similarity: a 32-term fp32 dot product of two rows normalised
    in fp32, |cos| <= 1: (D + 4) u per value, 64 u taken.  Counts and stored values (view_agreement, match_coverage, center_absmax):
    exact up to the fp64 division."""
    sfx = "_grid" if key.endswith("_grid") else ""
    base = key[:-len(sfx)] if sfx else key
    if base == "teacher_entropy":
        return ENT_FACTOR * U * ref["_S" + sfx]
    if base == "student_entropy":
        return ENT_FACTOR * U * ref["_S_student" + sfx]
    if base == "teacher_marginal_entropy":
        return ref["_marg_bound" + sfx]
    if base == "teacher_pmax":
        return ENT_FACTOR * U * (1 + ref["_lse_abs" + sfx]) * ref[key]
    if base == "kl":
        return ENT_FACTOR * U * (ref["_ce_scale" + sfx] + ref["_S" + sfx])
    if base == "match_similarity":
        return 64 * U
    return 1e-12 * max(1.0, abs(ref[key]))


def public_keys(ref):
    return sorted(k for k in ref if not k.startswith("_"))


LN = math.log
