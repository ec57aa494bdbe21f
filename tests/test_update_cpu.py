"""tests/update_ref.py is the reference's update: its float64 statement against torch.optim.AdamW / torch.optim.SGD over get_params_groups,
the oracle's LARS and the committed LARS fixture; its table builder; and the element bounds of tests/test_update_gpu.py held by a plain
fp32 emulation (numpy, the kernel's operations in the kernel's order, no FMA) on that test's own inputs, before any GPU is involved."""
import os

import numpy as np
import pytest
import torch

from oracle import esvit_oracle as O
from tests import golden_utils as GU
from tests import update_ref as UR

RTOL = 1e-12


def _close(a, b, what):
    assert float((a - b).abs().max()) <= RTOL * max(float(b.abs().max()), 1e-300), (what, float((a - b).abs().max()))


def _net():
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(13, 7), torch.nn.LayerNorm(7), torch.nn.Linear(7, 11)).double()
    return net


def _clip_gradients(params, clip):
    """utils.clip_gradients (utils.py:106-115)"""
    for p in params:
        if p.grad is not None:
            coef = clip / (p.grad.norm(2) + 1e-6)
            if coef < 1:
                p.grad.mul_(coef)


SCHED = [(1e-3, 0.04), (2e-3, 0.05), (5e-4, 0.06)]


def _drive(opt_of, rule):
    from esvit_amd.update import get_params_groups
    net = _net()
    groups = get_params_groups(net)
    group_of = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    opt = opt_of(groups)
    params = list(net.parameters())
    mine = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p)) for p in params]
    b1, b2, eps, mom = 0.9, 0.999, 1e-8, 0.9
    gen = torch.Generator().manual_seed(8)
    clipped = set()
    for t, (lr, wd) in enumerate(SCHED, start=1):
        for i, p in enumerate(params):
            p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64) * (10.0 if i == 0 else 0.01)
        grads = [p.grad.clone() for p in params]
        for gi, pg in enumerate(opt.param_groups):
            pg["lr"] = lr
            if gi == 0:
                pg["weight_decay"] = wd
        _clip_gradients(params, 3.0)
        opt.step()
        for i, (s, g) in enumerate(zip(mine, grads)):
            c = UR.clip_coef(UR.statistics(g)[0][0], 3.0, fp32_scalars=False)
            clipped.add(c < 1.0)
            grp = group_of[id(params[i])]
            if rule == UR.ADAMW:
                s["p"], s["m"], s["v"] = UR.adamw(s["p"], g, s["m"], s["v"], c, lr, wd, grp, b1, b2, eps, 1.0 - b1 ** t, 1.0 - b2 ** t, fp32_scalars=False)
            else:
                s["p"], s["m"] = UR.sgd(s["p"], g, s["m"], c, lr, wd, grp, mom, fp32_scalars=False)
    assert clipped == {True, False}
    for i, (p, s) in enumerate(zip(params, mine)):
        _close(s["p"], p.detach(), ("p", i))
        st = opt.state[p]
        if rule == UR.ADAMW:
            _close(s["m"], st["exp_avg"], ("exp_avg", i))
            _close(s["v"], st["exp_avg_sq"], ("exp_avg_sq", i))
        else:
            _close(s["m"], st["momentum_buffer"], ("momentum_buffer", i))


def test_adamw_statement_matches_torch(lib_built):
    _drive(lambda groups: torch.optim.AdamW(groups), UR.ADAMW)


def test_sgd_statement_matches_torch(lib_built):
    _drive(lambda groups: torch.optim.SGD(groups, lr=0, momentum=0.9), UR.SGD)


def _lars_statement_step(p, g, mu, lr, wd, clip=3.0, fp32_scalars=False):
    group = 0 if p.ndim != 1 else 1
    (gg, _), (pp, _), (gp, _) = UR.statistics(g.reshape(-1), p.reshape(-1))
    c = UR.clip_coef(gg, clip, fp32_scalars=fp32_scalars)
    q = UR.lars_q(gg, pp, gp, c, wd, 0.001, group, fp32_scalars=fp32_scalars)
    return UR.lars(p, g, mu, c, q, lr, wd, group, 0.9, fp32_scalars=fp32_scalars)


def test_lars_statement_matches_oracle():
    gen = torch.Generator().manual_seed(4)
    shapes = {"w": (9, 5), "b": (9,), "conv": (3, 2, 3, 3), "zero_p": (4, 4), "zero_g": (4, 3)}
    p = {n: torch.randn(s, generator=gen, dtype=torch.float64) for n, s in shapes.items()}
    p["zero_p"].zero_()
    mu_o = {n: torch.zeros_like(t) for n, t in p.items()}
    p_o = {n: t.clone() for n, t in p.items()}
    p_s, mu_s = {n: t.clone() for n, t in p.items()}, {n: torch.zeros_like(t) for n, t in p.items()}
    for step, (lr, wd) in enumerate([(0.3, 1e-4), (0.2, 0.0), (0.1, 3e-4)]):
        for n in p:
            g = torch.randn(shapes[n], generator=gen, dtype=torch.float64) * (5.0 if n == "w" else 0.05)
            if n == "zero_g":
                g.zero_()  # with wd == 0 (the second step) |c g + wd p| == 0: q falls back to 1
            p_o[n], mu_o[n] = O.lars_update(p_o[n], O.clip_gradient(g, 3.0), mu_o[n], lr, wd if p_o[n].ndim != 1 else 0.0)
            p_s[n], mu_s[n] = _lars_statement_step(p_s[n], g, mu_s[n], lr, wd)
    for n in p:
        _close(p_s[n], p_o[n], ("p", n))
        _close(mu_s[n], mu_o[n], ("mu", n))


def test_lars_statement_matches_reference_golden():
    gold = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variants.pt"), map_location="cpu", weights_only=False)
    p0, grads = GU.lars_case()
    p = {n: t.double() for n, t in p0.items()}
    mu = {n: torch.zeros_like(t) for n, t in p.items()}
    for (lr, wd), gs in zip(GU.LARS_SCHED, grads):
        for n in p:
            p[n], mu[n] = _lars_statement_step(p[n], gs[n].double(), mu[n], lr, wd)
    for n in p:
        assert (p[n] - gold["lars"]["params"][n].double()).abs().max().item() < 1e-6, n
        assert (mu[n] - gold["lars"]["mu"][n].double()).abs().max().item() < 1e-6, n


def test_lars_q_from_statistics_is_the_ratio_of_norms():
    gen = torch.Generator().manual_seed(6)
    for n in (1, 7, 5000):
        g, p = torch.randn(n, generator=gen, dtype=torch.float64), torch.randn(n, generator=gen, dtype=torch.float64)
        (gg, _), (pp, _), (gp, agp) = UR.statistics(g, p)
        for c, wd in ((1.0, 0.05), (0.25, 0.3), (0.5, 0.0)):
            want = 0.001 * float(p.norm()) / float((c * g + wd * p).norm())
            got = UR.lars_q(gg, pp, gp, c, wd, 0.001, 0, fp32_scalars=False)
            cond = UR.lars_cond(gg, pp, agp, c, wd, g, p, fp32_scalars=False)
            assert abs(got - want) <= 1e-12 * cond * want and cond >= 1.0 - 1e-12, (n, c, wd, got, want)
        assert UR.lars_q(gg, pp, gp, 1.0, 0.05, 0.001, 1) == 1.0  # group 1
    assert UR.lars_q(4.0, 0.0, 0.0, 1.0, 0.05, 0.001, 0) == 1.0   # |p| == 0
    assert UR.lars_q(0.0, 4.0, 0.0, 1.0, 0.0, 0.001, 0) == 1.0    # |u| == 0
    assert UR.clip_coef(1e12, 0.0) == 1.0 and UR.clip_coef(0.0, 3.0) == 1.0 and UR.clip_coef(36.0, 3.0) < 0.5


def test_scalars_enter_as_fp32():
    assert UR.f32(0.9) != 0.9 and UR._one_minus(0.9, True) == float(np.float32(1) - np.float32(0.9)) != 1.0 - 0.9
    bc1, bc2 = UR.unpack_bc(UR.pack_bc(0.9, 0.999, 3))
    assert bc1 == UR.f32(1.0 - 0.9 ** 3) and bc2 == UR.f32(1.0 - 0.999 ** 3)
    assert UR.unpack_bc(UR.pack_bc(0.9, 0.999, UR.T_BC2_ONE)) == (1.0, 1.0)
    assert UR.unpack_bc(UR.pack_bc(0.9, 0.999, 1000))[1] < 1.0
    assert UR.unpack_bc(UR.hyper(UR.SGD)["bc"]) == (0.0, 0.0)


# ---- the builder -------------------------------------------------------------------------------------------------------------------------
def _layouts():
    return [UR.Layout(UR.SPECS), UR.guard_layout()]


def test_chunk_table_is_sorted_and_complete():
    for L in _layouts():
        ch = L.chunks.tolist()
        assert ch == sorted(ch) and len(set(map(tuple, ch))) == len(ch)
        for i, s in enumerate(L.specs):
            assert [c for t, c in ch if t == i] == list(range(-(-s.numel // UR.CHUNK)))
    assert UR.Layout(UR.SPECS).nchunks_of(UR.BIG) == 258


def test_arena_regions_are_aligned_and_apart():
    for L in _layouts():
        for names, size, align in ((UR.F32_NAMES, L.size32, 4), (UR.BF16_NAMES, L.size16, 8)):
            regions = sorted((L.off[k][i], L.off[k][i] + s.numel) for i, s in enumerate(L.specs) for k in names)
            assert all(lo % align == 0 for lo, _ in regions)  # 16 bytes
            assert regions[0][0] >= UR.MOAT and size - regions[-1][1] >= UR.MOAT
            assert all(b[0] - a[1] >= UR.MOAT for a, b in zip(regions, regions[1:]))
        for rule in (UR.ADAMW, UR.SGD, UR.LARS):
            a32, a16 = UR.make_inputs(L, rule, special=L.specs == UR.Layout(UR.SPECS).specs)
            for names, arena in ((UR.F32_NAMES, a32), (UR.BF16_NAMES, a16)):
                mask = L.data_mask(names, rule)
                sent = torch.full((1,), UR.SENTINEL, dtype=arena.dtype)
                assert bool((arena[~mask] == sent).all()) and not bool((arena[mask] == sent).any())
            tab = L.table(1 << 20, 1 << 24, rule, bc=7)
            for i, s in enumerate(L.specs):
                assert tab[i, 0] == (1 << 20) + 4 * L.off["p"][i] and tab[i, 5] == s.numel and tab[i, 6] == s.group and tab[i, 7] == s.has_grad
                assert all(tab[i, k] % 16 == 0 for k in (0, 1, 2, 3, 4, 10, 11))
                if not s.has_grad:  # the row of a frozen parameter
                    assert tab[i, 1] == tab[i, 2] == tab[i, 3] == 0
                assert (tab[i, 3] != 0) == (rule == UR.ADAMW and bool(s.has_grad))
                assert (tab[i, 4] != 0) == bool(s.teacher) and (tab[i, 10] != 0) == bool(s.student_copy) and (tab[i, 11] != 0) == bool(s.teacher_copy)


def test_attributes_cover_whole_tail_and_multichunk():
    """every attribute value on a tensor whose last float4 is whole, on one with a scalar tail and on one of more than one chunk"""
    specs = UR.Layout(UR.SPECS).specs
    for field in ("group", "has_grad", "teacher", "student_copy", "teacher_copy"):
        for value in (0, 1):
            have = [s for s in specs if int(getattr(s, field)) == value]
            assert any(s.numel % 4 == 0 for s in have) and any(s.numel % 4 != 0 for s in have) and any(s.numel > UR.CHUNK for s in have), (field, value)
    assert {s.numel for s in specs} >= {1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 2, 257 * 4096 + 5}


# ---- the bounds hold for plain fp32 ------------------------------------------------------------------------------------------------------
F = np.float32


def emulate(L, rule, h, in32, in16):
    """update.hip in numpy fp32: the same operations in the same order, every one rounded (no FMA); statistics as fp32 chunk sums added
    in chunk order -> (fp32 arena, bf16 arena, statistics)"""
    out32, out16 = in32.clone(), in16.clone()
    S = 3 if rule == UR.LARS else 1
    stats = np.zeros((len(L), S), dtype=F)
    clip, lr, wd, h1, h2, eps, ema_m = (F(h[k]) for k in ("clip", "lr", "wd", "h1", "h2", "eps", "ema_m"))
    one = F(1.0)
    for i, s in enumerate(L.specs):
        p = L.get(out32, "p", i).numpy()
        if s.has_grad:
            g, m = L.get(out32, "g", i).numpy(), L.get(out32, "m", i).numpy()
            for lo in range(0, s.numel, UR.CHUNK):
                gc, pc = g[lo:lo + UR.CHUNK], p[lo:lo + UR.CHUNK]
                stats[i, 0] += np.sum(gc * gc, dtype=F)
                if S == 3:
                    stats[i, 1] += np.sum(pc * pc, dtype=F)
                    stats[i, 2] += np.sum(gc * pc, dtype=F)
            c = one
            if clip > 0:
                coef = clip / (np.sqrt(stats[i, 0]) + F(1e-6))
                if coef < one:
                    c = coef
            if rule == UR.ADAMW:
                v = L.get(out32, "v", i).numpy()
                decay = one - lr * wd if s.group == 0 else one
                bc1, bc2 = (F(x) for x in UR.unpack_bc(h["bc"]))
                step, isb2 = lr / bc1, one / np.sqrt(bc2)
                gs = g * c
                pe = p * decay
                m[:] = m + (one - h1) * (gs - m)
                v[:] = h2 * v + (one - h2) * gs * gs
                denom = np.sqrt(v) * isb2 + eps
                p[:] = pe - step * (m / denom)
            else:
                wdp = wd if s.group == 0 else F(0.0)
                q = one
                if rule == UR.LARS and s.group == 0:
                    pn = np.sqrt(stats[i, 1])
                    un = np.sqrt(max(c * c * stats[i, 0] + F(2.0) * c * wdp * stats[i, 2] + wdp * wdp * stats[i, 1], F(0.0)))
                    if pn > 0 and un > 0:
                        q = h2 * pn / un
                dp = q * (c * g + wdp * p)
                m[:] = h1 * m + dp
                p[:] = p - lr * m
            assert p.dtype == F and m.dtype == F
        if s.student_copy:
            L.get(out16, "pb", i).copy_(torch.from_numpy(p).to(torch.bfloat16))
        if s.teacher:
            t = L.get(out32, "t", i).numpy()
            t[:] = t * ema_m + p * (one - ema_m)
            if s.teacher_copy:
                L.get(out16, "tb", i).copy_(torch.from_numpy(t).to(torch.bfloat16))
    return out32, out16, torch.from_numpy(stats.reshape(-1))


@pytest.mark.parametrize("rule", [UR.ADAMW, UR.SGD, UR.LARS], ids=lambda r: UR.RULE_NAMES[r])
def test_bounds_hold_for_fp32_emulation(rule):
    L = UR.Layout(UR.SPECS)
    for name, over in UR.variants(rule).items():
        over = dict(over)
        in32, in16 = UR.make_inputs(L, rule, zero_moments=over.pop("zero_moments", False), special=True)
        h = UR.hyper(rule, **over)
        out32, out16, stats = emulate(L, rule, h, in32, in16)
        S = 3 if rule == UR.LARS else 1
        w1, b1 = UR.check_statistics(L, in32, stats, S)
        w2, b2 = UR.check_factors(L, rule, h, in32, stats)
        w3, b3 = UR.check_update(L, rule, h, in32, in16, out32, out16, stats)
        print("emulation", UR.RULE_NAMES[rule], name, "statistics %.3f" % w1, {k: round(v, 3) for k, v in {**w2, **w3}.items()})
        assert not (b1 + b2 + b3), (name, b1 + b2 + b3)
        if rule == UR.LARS:
            assert w2["q"] <= 0.05, w2  # (chunked fp32 statistics leave q far inside its bound)


def test_inputs_meet_their_conditions():
    """some tensors clipped and some not, none near the threshold; every product of the update is a normal number; the LARS fallbacks are
    taken; cond <= 8 (check_factors reports a larger one as broken: test_bounds_hold_for_fp32_emulation)"""
    L = UR.Layout(UR.SPECS)
    for rule in (UR.ADAMW, UR.LARS):
        in32, _ = UR.make_inputs(L, rule, special=True)
        h = UR.hyper(rule)
        coefs = []
        for i, s in enumerate(L.specs):
            if not s.has_grad:
                continue
            g = L.get(in32, "g", i).double()
            gg = UR.statistics(g)[0][0]
            coefs.append(h["clip"] / (gg ** 0.5 + 1e-6))
            nz = g[g != 0].abs()
            tiny = 1e-3 * 1e-3  # (1 - b2) and the smallest clip factor of the set
            assert nz.numel() == 0 or float(nz.min()) ** 2 * tiny > 1e-30
        assert any(c < 0.999 for c in coefs) and any(c > 1.001 for c in coefs) and not any(0.999 <= c <= 1.001 for c in coefs), coefs
        assert not L.get(in32, "p", UR.ZERO_P).any() and not L.get(in32, "g", UR.ZERO_G).any()
        assert not L.get(in32, "g", UR.BIG)[UR.ZERO_BLOCK[0]:UR.ZERO_BLOCK[1]].any()
    in32, _ = UR.make_inputs(L, UR.LARS, special=True)
    for over in ({}, dict(clip=0.0), dict(wd=0.0)):  # the count behind K of the LARS buffer takes cs <= CS_MAX
        h = UR.hyper(UR.LARS, **over)
        for i, s in enumerate(L.specs):
            if s.has_grad and s.group == 0:
                (gg, _), (pp, _), (gp, _) = UR.statistics(L.get(in32, "g", i), L.get(in32, "p", i))
                assert UR.lars_cs(gg, pp, gp, UR.clip_coef(gg, h["clip"]), h["wd"]) <= UR.CS_MAX, (over, i)
    assert UR.factors(L, UR.LARS, UR.hyper(UR.LARS), in32, None, UR.ZERO_P)[1] == 1.0
    assert UR.factors(L, UR.LARS, UR.hyper(UR.LARS, wd=0.0), in32, None, UR.ZERO_G)[1] == 1.0
    assert UR.factors(L, UR.LARS, UR.hyper(UR.LARS), in32, None, UR.ZERO_G)[1] == pytest.approx(UR.f32(0.001) / UR.f32(0.05), rel=1e-9)  # u = wd p
