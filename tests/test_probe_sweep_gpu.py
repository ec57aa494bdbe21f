"""Linear-probe sweep on the GPU: the class-index cross-entropy (esvit_dino_ce_fwd_bwd, terms = 0) and the per-member SGD rule
(ESVIT_RULE_SGD_MEMBERS) against fp64 computed from the very same fp32 inputs, and the sweep built from them against its fp64
restatement, the reference's fixture and the parent path (LinearClassifier + torch.optim.SGD) on the same device.

Bounds of the CE test, derived: any summation order of C non-negative fp32 terms is within (C - 1) 2^-24 relative, twice that is
allowed for the exponentials, plus eight roundings of magnitude max|z| for the subtractions and the final sum: per row
|dloss| <= tol = 2 C 2^-24 + 2^-20 max(1, max|z|), and |d ds| / row_w <= 2 tol p64 + 2^-23."""
import numpy as np
import pytest
import torch

from tests import golden_utils as GU

pytestmark = pytest.mark.gpu


def _setup(prec):
    import esvit_amd
    assert torch.cuda.is_available()
    esvit_amd.set_precision(prec)
    return torch.device("cuda:0")


def _teardown():
    import esvit_amd
    esvit_amd.set_precision("bf16")


def _ce_case(ops, dev, B, G, C, regime, seed):
    from esvit_amd.probe import ce_rows_host
    g = torch.Generator().manual_seed(seed)
    Rs = B * G
    z = torch.randn(Rs, C, generator=g) * (30.0 if regime == "x30" else 3.0)
    t = torch.randint(0, C, (B,), generator=g)
    if regime == "first":
        t.zero_()
    elif regime == "last":
        t.fill_(C - 1)
    trow = t.view(B, 1).expand(B, G).reshape(-1)
    if regime == "max":  # the target is the row maximum
        z[torch.arange(Rs), trow] = z.max(1).values + 1.0
    zd, td = z.to(dev), trow.to(torch.int32).to(dev)
    w = torch.full((Rs,), 1.0 / B, dtype=torch.float32, device=dev)
    keep = zd.clone()
    rl_none, ds_none = ops.probe_ce(zd, td, None, want_grad=False)
    assert ds_none is None and torch.equal(zd, keep)  # no gradient asked for: the logits are untouched
    rl, ds = ops.probe_ce(zd, td, w, inplace=False)
    assert torch.equal(zd, keep) and torch.equal(rl, rl_none)
    zin = zd.clone()
    rl_in, ds_in = ops.probe_ce(zin, td, w, inplace=True)
    assert ds_in.data_ptr() == zin.data_ptr() and torch.equal(ds_in, ds) and torch.equal(rl_in, rl)  # in place == out of place, bit for bit
    # fp64 from the same fp32 logits
    z64 = z.double()
    lse = torch.logsumexp(z64, 1)
    loss64 = lse - z64.gather(1, trow.view(-1, 1))[:, 0]
    p64 = torch.softmax(z64, 1)
    tol = 2.0 * C * 2.0 ** -24 + 2.0 ** -20 * z64.abs().max(1).values.clamp(min=1.0)
    dl = (rl[:, 0].double().cpu() - loss64).abs()
    print("probe_ce B=%d G=%d C=%d %s: worst loss error %.3e of %.3e" % (B, G, C, regime, dl.max().item(), tol[dl.argmax()].item()))
    assert bool((dl <= tol).all()), (regime, dl.max().item())
    want_ds = p64.clone()
    want_ds[torch.arange(Rs), trow] -= 1.0
    dd = (ds.double().cpu() / w.double().cpu().view(-1, 1) - want_ds).abs()
    room = 2.0 * tol.view(-1, 1) * p64 + 2.0 ** -23
    print("probe_ce B=%d G=%d C=%d %s: worst gradient error / bound %.3f" % (B, G, C, regime, (dd / room).max().item()))
    assert bool((dd <= room).all()), (regime, (dd / room).max().item())
    # ranks are comparisons: equal to the restatement on the same fp32 values
    rank_ref = ce_rows_host(z.view(B, G, C), t)[0][:, :, 1].reshape(-1)
    assert torch.equal(rl[:, 1].cpu(), rank_ref)
    if regime == "max":
        assert not rl[:, 1].any()
    return zd, td, w, rl, ds


def _ce_shapes():
    from esvit_amd import ops
    thr = ops.probe_ce_reg_row()
    return [(1, 1, 4), (3, 3, 12), (130, 3, 1000), (5, 2, thr), (5, 2, thr + 4)]


@pytest.mark.parametrize("case", range(5))
def test_probe_ce_against_fp64(case, lib_built):
    from esvit_amd import ops
    dev = _setup("fp32")
    try:
        B, G, C = _ce_shapes()[case]
        for i, regime in enumerate(("x3", "x30", "max", "first", "last")):
            zd, td, w, rl, ds = _ce_case(ops, dev, B, G, C, regime, seed=100 * case + i)
        # a row of NaN logits (and one holding an inf): loss NaN, rank C, and nothing else moves
        Rs = B * G
        bad_rows = [Rs // 2] if Rs < 3 else [Rs // 2, Rs - 1]
        zb = zd.clone()
        zb[bad_rows[0]] = float("nan")
        if len(bad_rows) > 1:
            zb[bad_rows[1], C // 2] = float("inf")
        rlb, dsb = ops.probe_ce(zb, td, w, inplace=False)
        good = torch.ones(Rs, dtype=torch.bool, device=dev)
        good[bad_rows] = False
        assert torch.isnan(rlb[~good, 0]).all() and bool((rlb[~good, 1] == C).all()) and torch.isnan(dsb[~good]).all()
        assert torch.equal(rlb[good], rl[good]) and torch.equal(dsb[good], ds[good])
    finally:
        _teardown()


def test_probe_ce_is_deterministic(lib_built):
    """more workgroups than the chip holds at once, ten launches: the same bits"""
    from esvit_amd import ops
    dev = _setup("fp32")
    try:
        B, G, C = 1024, 8, 1000
        g = torch.Generator().manual_seed(7)
        z = (torch.randn(B * G, C, generator=g) * 3.0).to(dev)
        t = torch.randint(0, C, (B,), generator=g).to(torch.int32).view(B, 1).expand(B, G).reshape(-1).contiguous().to(dev)
        w = torch.full((B * G,), 1.0 / B, dtype=torch.float32, device=dev)
        rl0, ds0 = ops.probe_ce(z, t, w, inplace=False)
        rl0, ds0 = rl0.clone(), ds0.clone()
        for _ in range(9):
            rl, ds = ops.probe_ce(z, t, w, inplace=False)
            assert torch.equal(rl, rl0) and torch.equal(ds, ds0)
    finally:
        _teardown()


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _member_tables(ops, dev, ps, gs, mus, member_of, lrs, wds):
    chunk = ops.update_chunk_elems()
    tab = np.zeros((len(ps), 12), dtype=np.int64)
    chunks = []
    for i, (p, g, mu) in enumerate(zip(ps, gs, mus)):
        m = member_of[i]
        hyper = _bits(lrs[m]) | (_bits(wds[m]) << 32)
        hyper -= (1 << 64) if hyper >= 1 << 63 else 0
        tab[i, 0], tab[i, 1], tab[i, 2], tab[i, 5], tab[i, 7], tab[i, 9] = p.data_ptr(), g.data_ptr(), mu.data_ptr(), p.numel(), 1 | (m << 32), hyper
        chunks.extend((i, ci) for ci in range(-(-p.numel() // chunk)))
    return torch.from_numpy(tab).to(dev), torch.tensor(chunks, dtype=torch.int32).to(dev), len(chunks)


def _adamw_once(ops, dev):
    """one existing-style AdamW call (clip 3, two tensors, a chunk tail) on fixed inputs -> the updated tensors"""
    g = torch.Generator().manual_seed(99)
    n = (ops.update_chunk_elems() + 40, 300)
    p = [torch.randn(k, generator=g).to(dev) for k in n]
    gr = [torch.randn(k, generator=g).to(dev) for k in n]
    m = [0.1 * torch.randn(k, generator=g).to(dev) for k in n]
    v = [0.01 * torch.rand(k, generator=g).to(dev) for k in n]
    chunk = ops.update_chunk_elems()
    tab = np.zeros((2, 12), dtype=np.int64)
    chunks = []
    bc = _bits(1.0 - 0.9 ** 3) | (_bits(1.0 - 0.999 ** 3) << 32)
    for i in range(2):
        tab[i, :6] = [p[i].data_ptr(), gr[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), 0, n[i]]
        tab[i, 6], tab[i, 7], tab[i, 8] = i, 1, bc
        chunks.extend((i, ci) for ci in range(-(-n[i] // chunk)))
    tab_d, ch_d = torch.from_numpy(tab).to(dev), torch.tensor(chunks, dtype=torch.int32).to(dev)
    sq = torch.zeros(2, dtype=torch.float32, device=dev)
    skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.grad_sqnorm(tab_d, 2, ch_d, len(chunks), sq, stats=1)
    ops.fused_clip_update_ema(ops.RULE_ADAMW, tab_d, 2, ch_d, len(chunks), sq, 3.0, 1e-3, 0.05, 0.9, 0.999, 1e-8, 0.996, skipped=skipped)
    torch.cuda.synchronize()
    assert int(skipped.item()) == 0
    return p + m + v


def test_sgd_members_rule_against_fp64(lib_built):
    from esvit_amd import ops
    dev = _setup("fp32")
    try:
        before = _adamw_once(ops, dev)
        M, mom = 3, 0.9
        sizes = (ops.update_chunk_elems() + 4, 240)  # a member's "weight" (a chunk and a tail) and "bias" (well under a chunk)
        lrs, wds = (0.01, 0.05, 0.3), (0.0, 1e-3, 1e-3)
        gen = torch.Generator().manual_seed(17)
        member_of = [m for m in range(M) for _ in sizes]
        p0 = [torch.randn(n, generator=gen) for _ in range(M) for n in sizes]
        grads = [[torch.randn(n, generator=gen) for _ in range(M) for n in sizes] for _ in range(2)]
        f32 = lambda x: float(np.float32(x))  # noqa: E731  (the kernel's scalars are fp32)

        def run(poison_step=None):
            ps, mus = [t.clone().to(dev) for t in p0], [torch.zeros_like(t).to(dev) for t in p0]
            gs = [torch.zeros_like(t).to(dev) for t in p0]
            tab, ch, nch = _member_tables(ops, dev, ps, gs, mus, member_of, lrs, wds)
            sq = torch.zeros(len(ps), dtype=torch.float32, device=dev)
            skipped = torch.zeros(M, dtype=torch.int32, device=dev)
            for step in range(2):
                for gd, gh in zip(gs, grads[step]):
                    gd.copy_(gh)
                if poison_step == step:
                    gs[3][3] = float("inf")  # member 1's bias gradient
                p_in, mu_in = [t.clone() for t in ps], [t.clone() for t in mus]
                ops.grad_sqnorm(tab, len(ps), ch, nch, sq, stats=1)
                ops.fused_clip_update_ema(ops.RULE_SGD_MEMBERS, tab, len(ps), ch, nch, sq, 0.0, 0.0, 0.0, mom, 0.0, 0.0, 0.0, skipped=skipped)
                if poison_step is None:  # against fp64 from this step's own fp32 inputs
                    for i in range(len(ps)):
                        lr, wd, m32 = f32(lrs[member_of[i]]), f32(wds[member_of[i]]), f32(mom)
                        p64, g64, mu64 = p_in[i].double(), gs[i].double(), mu_in[i].double()
                        want_mu = m32 * mu64 + (g64 + wd * p64)
                        room = 4.0 * 2.0 ** -24 * ((m32 * mu64).abs() + g64.abs() + (wd * p64).abs())
                        assert bool(((mus[i].double() - want_mu).abs() <= room).all()), (step, i)
                        want_p = p64 - lr * mus[i].double()
                        room = 4.0 * 2.0 ** -24 * (p64.abs() + (lr * mus[i].double()).abs())
                        assert bool(((ps[i].double() - want_p).abs() <= room).all()), (step, i)
                    if step == 1:
                        assert all(bool(mu_in[i].any()) for i in range(len(ps)))  # the second step saw a non-zero buffer
                elif poison_step == step:
                    for i in (2, 3):  # member 1: nothing moved
                        assert torch.equal(ps[i], p_in[i]) and torch.equal(mus[i], mu_in[i])
            return ps, mus, skipped

        ps, mus, skipped = run()
        assert skipped.tolist() == [0, 0, 0]
        # the guard: member 1's bias gradient is inf at the second step
        ps_b, mus_b, skipped_b = run(poison_step=1)
        assert skipped_b.tolist() == [0, 1, 0]
        for i in (0, 1, 4, 5):  # every other member: the un-poisoned run, bit for bit
            assert torch.equal(ps_b[i], ps[i]) and torch.equal(mus_b[i], mus[i]), i
        assert all(bool(torch.isfinite(t).all()) for t in ps_b + mus_b)
        # rules 0 - 2 are what they were
        after = _adamw_once(ops, dev)
        assert all(torch.equal(a, b) for a, b in zip(before, after))
    finally:
        _teardown()


def test_sweep_steps_against_fp64_restatement(lib_built, monkeypatch):
    from esvit_amd import eval as E, ops
    dev = _setup("fp32")
    try:
        B, D, G = 130, 68, 5
        lrs = (0.01, 0.05, 0.1, 0.3, 0.5)
        calls = {"ce": 0, "rule3": 0}
        real_ce, real_up = ops.probe_ce, ops.fused_clip_update_ema
        monkeypatch.setattr(ops, "probe_ce", lambda *a, **k: (calls.__setitem__("ce", calls["ce"] + 1), real_ce(*a, **k))[1])
        monkeypatch.setattr(ops, "fused_clip_update_ema",
                            lambda rule, *a, **k: (calls.__setitem__("rule3", calls["rule3"] + (rule == ops.RULE_SGD_MEMBERS)), real_up(rule, *a, **k))[1])
        for C, kernels in ((12, True), (10, False)):  # G * C = 60: not a multiple of 64;  C = 10: the torch route (rows are not 16 bytes)
            calls["ce"] = calls["rule3"] = 0
            g = torch.Generator().manual_seed(61 + C)
            data = [(torch.randn(B, D, generator=g), torch.randint(0, C, (B,), generator=g)) for _ in range(3)]
            torch.manual_seed(13)
            sweep = E.LinearProbeSweep(D, C, lrs)
            ref = E.LinearProbeSweep(D, C, lrs).double()
            ref.init_from(sweep.weight[0].double())
            sweep = sweep.to(dev)
            for f, t in data:
                got = sweep.step(f.to(dev), t.to(dev))
                want = ref.step(f.double(), t)
                assert (got.double().cpu() - want).abs().max().item() < 3e-3
            assert (sweep.weight.double().cpu() - ref.weight).abs().max().item() < 3e-4
            assert (sweep.bias.double().cpu() - ref.bias).abs().max().item() < 3e-4
            assert not sweep.diverged.any()
            assert (calls["ce"], calls["rule3"]) == ((3, 3) if kernels else (0, 0)), (C, calls)
    finally:
        _teardown()


def test_fixture_on_the_gpu_and_against_the_parent_path(lib_built):
    from esvit_amd import eval as E
    from tests.test_composition_cpu import build_nano
    from tests.test_probe_sweep_cpu import check_fixture
    dev = _setup("fp32")
    try:
        g, c, model, sweep, val = check_fixture(dev, wtol=3e-4, ltol=3e-3)  # the bounds of check_linear_probe(dev, tol=3e-4)
        # the parent path on the same device: LinearClassifier + F.cross_entropy + torch.optim.SGD
        clf = E.LinearClassifier(g["dim"], c["num_labels"])
        GU.linear_probe_init(clf)
        clf = clf.to(dev)
        opt = torch.optim.SGD(clf.parameters(), c["lr"], momentum=0.9, weight_decay=0)
        tr, va = GU.linear_probe_data()
        depths = list(GU.NANO["depths"])
        for ep in range(2):
            E.train_linear_epoch(model, clf, opt, tr, ep, c["n_last_blocks"], c["avgpool"], depths)
        one = E.validate_network(va, model, clf, c["n_last_blocks"], c["avgpool"], depths)
        assert (sweep.weight[1] - clf.linear.weight).abs().max().item() < 3e-4 and (sweep.bias[1] - clf.linear.bias).abs().max().item() < 3e-4
        assert one["acc1"] == pytest.approx(val[1]["acc1"], abs=1e-9) and one["acc5"] == pytest.approx(val[1]["acc5"], abs=1e-9), (one, val[1])
    finally:
        _teardown()


def test_accuracies_end_to_end_against_fp64(lib_built):
    from esvit_amd import eval as E, ops
    from tests.test_probe_sweep_cpu import PrecomputedFeatures
    dev = _setup("fp32")
    try:
        B, D, C, G = 256, 64, 1000, 3
        g = torch.Generator().manual_seed(71)
        feats, target = torch.randn(B, D, generator=g), torch.randint(0, C, (B,), generator=g)
        sweep = E.LinearProbeSweep(D, C, (0.1, 0.2, 0.3))
        sweep.weight.data.copy_(torch.randn(G, C, D, generator=g) * (3.0 / 8.0))  # logits ~ N(0, 3^2)
        sweep.bias.data.copy_(0.1 * torch.randn(G, C, generator=g))
        # fp64 restatement from the same fp32 numbers; rows whose decision hangs on less than 1e-4 are set aside
        z = torch.einsum("bd,gcd->bgc", feats.double(), sweep.weight.double()) + sweep.bias.double().unsqueeze(0)
        zt = z.gather(2, target.view(B, 1, 1).expand(B, G, 1))
        others = z.scatter(2, target.view(B, 1, 1).expand(B, G, 1), float("-inf"))
        top = others.topk(5, dim=2).values
        hit1, hit5 = zt[..., 0] > top[..., 0], zt[..., 0] > top[..., 4]
        near1, near5 = (zt[..., 0] - top[..., 0]).abs() < 1e-4, (zt[..., 0] - top[..., 4]).abs() < 1e-4
        assert near1.float().mean().item() <= 0.01 and near5.float().mean().item() <= 0.01
        sweep = sweep.to(dev)
        val, best = E.validate_linear_sweep([(feats, target)], PrecomputedFeatures(), sweep, 4, False, None)
        tgt = target.to(torch.int32).view(B, 1).expand(B, G).contiguous().view(-1).to(dev)
        rank = ops.probe_ce(sweep.logits(feats.to(dev)).reshape(B * G, C), tgt, None, want_grad=False)[0].view(B, G, 2)[:, :, 1].cpu()
        assert torch.equal((rank < 1)[~near1], hit1[~near1]) and torch.equal((rank < 5)[~near5], hit5[~near5])
        for m in range(G):
            assert abs(val[m]["acc1"] - 100.0 * hit1[:, m].sum().item() / B) <= 100.0 * near1[:, m].sum().item() / B + 1e-9
            assert abs(val[m]["acc5"] - 100.0 * hit5[:, m].sum().item() / B) <= 100.0 * near5[:, m].sum().item() / B + 1e-9
        acc1 = [v["acc1"] for v in val]
        assert best == acc1.index(max(acc1))
    finally:
        _teardown()
