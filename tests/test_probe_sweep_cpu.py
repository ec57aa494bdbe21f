"""Linear-probe sweep (esvit_amd/probe.py), the parts that need no GPU: the host branch against G stand-alone LinearClassifier +
torch.optim.SGD runs in fp64, against the reference's fixture, member independence under a diverging member, the single all-reduce
on two gloo ranks, the state_dict round trip, the rank rule, and the argument checks of the two library modes (cross-compiled,
nothing launched)."""
import copy
import math
import os
import sys
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import golden_utils as GU
from tests.test_composition_cpu import build_nano, cpu_ops  # noqa: F401  (cpu_ops: the fixture that swaps the kernels for their restatement)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


class PrecomputedFeatures:
    """stands in for the backbone: the loader's "images" are the features already"""

    def forward_return_n_last_blocks(self, x, n, avgpool, depths):
        return x


def _data(batches, B, D, C, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn(B, D, generator=g), torch.randint(0, C, (B,), generator=g)) for _ in range(batches)]


def _standalone(w0, lr, wd, data, epochs, cosine=True):
    """the parent path for ONE (lr, wd): LinearClassifier + F.cross_entropy + torch.optim.SGD (+ CosineAnnealingLR), in fp64
    -> (classifier, optimizer, per-epoch mean losses, per-epoch lrs)"""
    from esvit_amd import eval as E
    clf = E.LinearClassifier(w0.shape[1], w0.shape[0]).double()
    clf.linear.weight.data.copy_(w0)
    opt = torch.optim.SGD(clf.parameters(), lr, momentum=0.9, weight_decay=wd)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, epochs, eta_min=0) if cosine else None
    losses, lrs = [], []
    for ep in range(epochs):
        lrs.append(opt.param_groups[0]["lr"])
        tot = 0.0
        for f, t in data:
            loss = torch.nn.functional.cross_entropy(clf(f.double()), t)
            opt.zero_grad()
            loss.backward()
            opt.step()
            tot += loss.item()
        losses.append(tot / len(data))
        if sched is not None:
            sched.step()
    return clf, opt, losses, lrs


def test_sweep_equals_standalone_probes_fp64(lib_built):
    from esvit_amd import eval as E
    D, C, epochs = 16, 5, 3
    lrs, wds = (0.01, 0.05, 0.3), (0.0, 1e-3)
    data = _data(3, 8, D, C, seed=11)
    torch.manual_seed(3)
    sweep = E.LinearProbeSweep(D, C, lrs, wds).double()
    assert sweep.members == 6 and sweep.weight.shape == (6, C, D) and sweep.weight.is_contiguous() and sweep.bias.shape == (6, C)
    assert all(torch.equal(sweep.weight[g], sweep.weight[0]) for g in range(6)) and not sweep.bias.any()  # one draw, replicated
    w0 = sweep.weight[0].clone()
    members = [(lr, wd) for lr in lrs for wd in wds]
    alone = [_standalone(w0, lr, wd, data, epochs) for lr, wd in members]
    for ep in range(epochs):
        sweep.set_lrs([a[3][ep] for a in alone])  # the schedulers' own values
        stats = E.train_linear_sweep_epoch(PrecomputedFeatures(), sweep, data, ep, 4, False, None)
        for g, a in enumerate(alone):
            assert abs(stats[g]["loss"] - a[2][ep]) < 1e-12 and stats[g]["lr"] == a[3][ep], (ep, g, stats[g], a[2][ep])
    for g, (clf, opt, _, _) in enumerate(alone):
        assert (sweep.weight[g] - clf.linear.weight).abs().max().item() < 1e-12
        assert (sweep.bias[g] - clf.linear.bias).abs().max().item() < 1e-12
        assert (sweep.weight_momentum[g] - opt.state[clf.linear.weight]["momentum_buffer"]).abs().max().item() < 1e-12
        assert (sweep.bias_momentum[g] - opt.state[clf.linear.bias]["momentum_buffer"]).abs().max().item() < 1e-12
    assert not sweep.diverged.any()
    # set_epoch: the closed form of CosineAnnealingLR(eta_min=0) against the scheduler's own recursion
    T = 7
    opts = [torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr) for lr, _ in members]
    scheds = [torch.optim.lr_scheduler.CosineAnnealingLR(o, T, eta_min=0) for o in opts]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ep in range(T):
            sweep.set_epoch(ep, T)
            for g, s in enumerate(scheds):
                want = s.get_last_lr()[0]
                assert abs(sweep.lrs[g] - want) <= 1e-12 * want, (ep, g, sweep.lrs[g], want)
                s.step()


def _fixture_sweep(dev):
    from esvit_amd import eval as E
    g = torch.load(os.path.join(GOLD, "linear_probe.pt"), weights_only=False)
    c = GU.LINEAR_PROBE
    model = build_nano()
    GU.fill_state_dict(model.state_dict(), 0)
    model = model.to(dev).eval()
    clf = E.LinearClassifier(g["dim"], c["num_labels"])
    GU.linear_probe_init(clf)
    sweep = E.LinearProbeSweep(g["dim"], c["num_labels"], (0.005, c["lr"], 0.5))
    sweep.init_from(clf.linear.weight, clf.linear.bias)
    return g, c, model, sweep.to(dev)


def check_fixture(dev, wtol, ltol):
    """the member at the fixture's learning rate reproduces tests/golden/linear_probe.pt (the reference's own loop): weights and bias
    within wtol, losses within ltol, accuracies within 1e-3; its export, loaded into LinearClassifier, validates to the same numbers"""
    from esvit_amd import eval as E
    g, c, model, sweep = _fixture_sweep(dev)
    tr, va = GU.linear_probe_data()
    depths = list(GU.NANO["depths"])
    stats = [E.train_linear_sweep_epoch(model, sweep, tr, ep, c["n_last_blocks"], c["avgpool"], depths) for ep in range(2)]
    val, best = E.validate_linear_sweep(va, model, sweep, c["n_last_blocks"], c["avgpool"], depths)
    assert len(val) == 3 and best == max(range(3), key=lambda i: (val[i]["acc1"], -i))
    m = 1
    for got, want in zip(stats, g["train"]):
        assert abs(got[m]["loss"] - want["loss"]) < ltol and abs(got[m]["lr"] - want["lr"]) < 1e-9, (got[m], want)
    assert abs(val[m]["loss"] - g["val"]["loss"]) < ltol, (val[m], g["val"])
    assert val[m]["acc1"] == pytest.approx(g["val"]["acc1"], abs=1e-3) and val[m]["acc5"] == pytest.approx(g["val"]["acc5"], abs=1e-3)
    assert (sweep.weight[m].cpu() - g["weight"]).abs().max().item() < wtol
    assert (sweep.bias[m].cpu() - g["bias"]).abs().max().item() < wtol
    # export -> LinearClassifier (the module tree of the reference's probe checkpoint) -> the existing validate_network
    clf = E.LinearClassifier(g["dim"], c["num_labels"])
    assert list(sweep.export(m).keys()) == g["keys"]
    clf.load_state_dict(sweep.export(m))
    one = E.validate_network(va, model, clf.to(dev), c["n_last_blocks"], c["avgpool"], depths)
    # (two fp32 evaluations of the same loss, each within the CE kernel's per-row bound 2 C 2^-24 + 2^-20 max|z| at C = 12, |z| < 8)
    assert abs(one["loss"] - val[m]["loss"]) < 2e-5 and one["acc1"] == pytest.approx(val[m]["acc1"], abs=1e-3), (one, val[m])
    assert one["acc5"] == pytest.approx(val[m]["acc5"], abs=1e-3)
    return g, c, model, sweep, val


def test_fixture_member_matches_reference_golden(cpu_ops, lib_built):  # noqa: F811
    check_fixture("cpu", wtol=2e-4, ltol=2e-3)  # the bounds of check_linear_probe("cpu")


# Features of magnitude 1e140: with them a learning rate of 1e30 overflows fp64 ITSELF at the second step (weights ~ 1e30 * 1e140, logits
# ~ 1e170 * 1e140 * D), while the sane members stay around 1e140 / 1e280 -- finite -- for the handful of steps run here.
HUGE = 1e140


def _run_steps(sweep, data, steps):
    losses, trace = [], []
    for i in range(steps):
        f, t = data[i % len(data)]
        losses.append(sweep.step(f.double(), t).clone())
        trace.append((sweep.weight.clone(), sweep.bias.clone()))
    return losses, trace


def test_members_are_independent_and_a_diverging_member_is_frozen(lib_built):
    from esvit_amd import eval as E
    D, C, steps = 8, 4, 6
    g = torch.Generator().manual_seed(21)
    data = [(HUGE * torch.randn(8, D, generator=g, dtype=torch.float64), torch.randint(0, C, (8,), generator=g)) for _ in range(3)]
    w0 = 0.01 * torch.randn(C, D, generator=g, dtype=torch.float64)
    # precondition, on the stand-alone fp64 loop: lr = 1e30 is non-finite within two steps
    from esvit_amd.eval import LinearClassifier
    clf = LinearClassifier(D, C).double()
    clf.linear.weight.data.copy_(w0)
    opt = torch.optim.SGD(clf.parameters(), 1e30, momentum=0.9, weight_decay=0)
    seen = []
    for f, t in data[:2]:
        loss = torch.nn.functional.cross_entropy(clf(f), t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        seen.append(bool(torch.isfinite(loss)) and bool(torch.isfinite(clf.linear.weight).all()) and bool(torch.isfinite(clf.linear.bias).all()))
    assert seen[0] and not seen[1], seen
    # ... and the sane learning rates stay finite over the steps of this test
    for lr in (0.01, 0.3):
        c2, _, losses, _ = _standalone(w0, lr, 1e-3, data * 2, 1, cosine=False)
        assert math.isfinite(losses[0]) and bool(torch.isfinite(c2.linear.weight).all())
    with_bad = E.LinearProbeSweep(D, C, (0.01, 0.3, 1e30), (0.0, 1e-3)).double()
    without = E.LinearProbeSweep(D, C, (0.01, 0.3), (0.0, 1e-3)).double()
    with_bad.init_from(w0)
    without.init_from(w0)
    la, ta = _run_steps(with_bad, data, steps)
    lb, _ = _run_steps(without, data, steps)
    # every other member: bit-identical to the sweep that never had the bad one
    for name in ("weight", "bias", "weight_momentum", "bias_momentum"):
        assert torch.equal(getattr(with_bad, name)[:4], getattr(without, name)), name
    assert all(torch.equal(a[:4], b) for a, b in zip(la, lb))
    assert torch.isfinite(without.weight).all() and all(torch.isfinite(b).all() for b in lb)
    assert with_bad.diverged.tolist() == [False] * 4 + [True] * 2 and not without.diverged.any()
    # the bad members: flagged, finite, frozen at the values they had when their gradient first went non-finite
    assert with_bad.skipped.tolist() == [0] * 4 + [steps - 1] * 2
    for name in ("weight", "bias", "weight_momentum", "bias_momentum"):
        assert torch.isfinite(getattr(with_bad, name)[4:]).all(), name
    assert torch.equal(with_bad.weight[4:], ta[0][0][4:]) and torch.equal(with_bad.bias[4:], ta[0][1][4:])
    assert not torch.equal(ta[0][0][4], w0)  # (it did take its first step)


def _gloo_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(max(1, (os.cpu_count() or 2) // world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from esvit_amd import eval as E
    D, C, steps = 12, 6, 3
    lrs, wds = (0.02, 0.2), (0.0, 1e-3)
    data = _data(steps, 8, D, C, seed=31)
    torch.manual_seed(5)
    sweep = E.LinearProbeSweep(D, C, lrs, wds).double()
    w0 = sweep.weight[0].clone()
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        local = []
        for f, t in data:  # this rank's half of every batch
            local.append(sweep.step(f[rank * 4:(rank + 1) * 4].double(), t[rank * 4:(rank + 1) * 4]))
    finally:
        dist.all_reduce = real
    ok = len(calls) == steps  # exactly one all-reduce per step
    ok = ok and sweep.weight.dtype == torch.float64
    for g, (lr, wd) in enumerate((lr, wd) for lr in lrs for wd in wds):  # one process, the whole batch
        clf, opt, _, _ = _standalone(w0, lr, wd, data, 1, cosine=False)
        ok = ok and (sweep.weight[g] - clf.linear.weight).abs().max().item() < 1e-12 and (sweep.bias[g] - clf.linear.bias).abs().max().item() < 1e-12
        ok = ok and (sweep.weight_momentum[g] - opt.state[clf.linear.weight]["momentum_buffer"]).abs().max().item() < 1e-12
    # the rank-averaged loss of the first batch is the whole batch's loss at the initial weights
    first = local[0].clone()
    dist.all_reduce(first)
    z = data[0][0].double() @ w0.t()
    ok = ok and (first / world - torch.nn.functional.cross_entropy(z, data[0][1])).abs().max().item() < 1e-12
    out[rank] = bool(ok)
    dist.destroy_process_group()


def test_world2_gloo_one_all_reduce_per_step(lib_built):
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(world, 29641, out), nprocs=world, join=True)
    assert dict(out) == {0: True, 1: True}, dict(out)


def test_state_dict_round_trip_resumes_mid_run(lib_built):
    from esvit_amd import eval as E
    D, C = 8, 4
    g = torch.Generator().manual_seed(41)
    data = [(HUGE * torch.randn(8, D, generator=g, dtype=torch.float64), torch.randint(0, C, (8,), generator=g)) for _ in range(4)]
    torch.manual_seed(9)
    a = E.LinearProbeSweep(D, C, (0.02, 1e30), (0.0, 1e-3)).double()
    a.set_epoch(1, 5)
    _run_steps(a, data[:3], 3)
    assert a.diverged.tolist() == [False, False, True, True]
    sd = copy.deepcopy(a.state_dict())
    b = E.LinearProbeSweep(D, C, (1.0, 2.0), (0.5, 0.25)).double()  # other hyper-parameters, another draw: all of it must come from the checkpoint
    b.load_state_dict(sd)
    assert b.base_lrs == a.base_lrs and b.member_wds == a.member_wds and b.lrs == a.lrs and b.momentum == a.momentum
    assert torch.equal(b.diverged, a.diverged) and torch.equal(b.skipped, a.skipped)
    la, _ = _run_steps(a, data[3:], 2)
    lb, _ = _run_steps(b, data[3:], 2)
    for name in ("weight", "bias", "weight_momentum", "bias_momentum", "skipped"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert all(torch.equal(x[:2], y[:2]) for x, y in zip(la, lb))
    assert set(a.state_dict().keys()) == set(sd.keys())


def _place_in_stable_order(z, t):
    order = torch.sort(z, descending=True, stable=True)[1]
    return int((order == t).nonzero()[0, 0])


def test_rank_rule_and_ties(lib_built):
    from esvit_amd import eval as E
    from esvit_amd.probe import ce_rows_host
    C = 8
    flat = torch.zeros(C)  # every class tied: the target's rank is its index
    cases = [(flat, 0, 0), (flat, 1, 1), (flat, 4, 4), (flat, 5, 5),
             (torch.tensor([5., 3, 3, 1, 3, 0, 7, 3]), 2, 3),   # 7 and 5 above, one equal 3 in front
             (torch.tensor([2., 2, 2, 2, 9, 2, 2, 2]), 5, 5),   # the 9 above, four equal in front
             (torch.tensor([2., 2, 2, 2, 9, 2, 2, 2]), 3, 4),
             (torch.tensor([1., 2, 3, 4, 5, 6, 7, 8]), 0, 7)]
    z = torch.stack([c[0] for c in cases]).view(len(cases), 1, C)
    t = torch.tensor([c[1] for c in cases])
    rl, _ = ce_rows_host(z, t)
    assert rl[:, 0, 1].tolist() == [float(c[2]) for c in cases]
    g = torch.Generator().manual_seed(51)
    zi = torch.randint(-2, 3, (64, 3, 12), generator=g).float()  # integer logits: ties everywhere
    ti = torch.randint(0, 12, (64,), generator=g)
    ri = ce_rows_host(zi, ti)[0][:, :, 1]
    for b in range(64):
        for m in range(3):
            assert int(ri[b, m]) == _place_in_stable_order(zi[b, m], int(ti[b]))
    # through the public interface: weights zero, the bias IS the logit row; top-1 <=> rank < 1, top-5 <=> rank < 5
    sweep = E.LinearProbeSweep(4, C, (0.1, 0.2, 0.3, 0.4))
    sweep.weight.data.zero_()
    sweep.bias.data.copy_(torch.stack([cases[0][0], cases[4][0], cases[5][0], cases[7][0]]))
    loader = [(torch.zeros(1, 4), torch.tensor([tt])) for tt in (0, 2, 5, 4)]  # ranks per member: (0,0,0,.), ...
    val, best = E.validate_linear_sweep(loader, PrecomputedFeatures(), sweep, 4, False, None)
    want_rank = [[_place_in_stable_order(sweep.bias[m], tt) for tt in (0, 2, 5, 4)] for m in range(4)]
    for m in range(4):
        assert val[m]["acc1"] == pytest.approx(25.0 * sum(r < 1 for r in want_rank[m])) and val[m]["acc5"] == pytest.approx(25.0 * sum(r < 5 for r in want_rank[m]))
    assert want_rank[0] == [0, 2, 5, 4] and want_rank[2][2] == 5 and want_rank[3][3] == 3
    assert best == max(range(4), key=lambda i: (val[i]["acc1"], -i))
    firsts = [i for i in range(4) if val[i]["acc1"] == max(v["acc1"] for v in val)]
    assert best == firsts[0]  # the FIRST maximum
    # fewer than five classes: "top 5" is top min(5, C)
    small = E.LinearProbeSweep(4, 3, (0.1,))
    small.weight.data.zero_()
    small.bias.data.copy_(torch.tensor([[1., 1, 0]]))
    val, best = E.validate_linear_sweep([(torch.zeros(3, 4), torch.tensor([0, 1, 2]))], PrecomputedFeatures(), small, 4, False, None)
    assert best == 0 and val[0]["acc5"] == pytest.approx(100.0) and val[0]["acc1"] == pytest.approx(100.0 / 3)


def test_library_argument_checks_come_before_any_launch(lib_built):
    """plausible, never dereferenced addresses: the checks of the two new modes answer before any device call"""
    from esvit_amd import _lib, ops
    lib = _lib.lib

    def ce(dtype=_lib.F32, t=None, term_w=None, K=12, row_w=0x3000, ds=0x5000, center=None, row_order=None, s_max=None, s_lse=None, tmatch=0x2000):
        rc = lib.esvit_dino_ce_fwd_bwd(dtype, 0x1000, t, center, None, None, tmatch, row_w, 0, term_w, 1.0, 1.0, 8, K, 0x4000, ds, row_order, s_max,
                                       s_lse, None)
        return rc, lib.esvit_last_error().decode()

    for kw in (dict(t=0x8000), dict(term_w=0x8000), dict(dtype=_lib.BF16), dict(K=10), dict(K=0), dict(center=0x8000), dict(row_order=0x8000),
               dict(s_max=0x8000, s_lse=0x9000), dict(tmatch=None), dict(row_w=None)):
        rc, msg = ce(**kw)
        assert rc == -1 and "terms = 0" in msg, (kw, rc, msg)
    # the other term counts are what they were: 2 and 4 only
    rc = lib.esvit_dino_ce_fwd_bwd(_lib.F32, 0x1000, 0x1100, 0x1200, 0x1300, 0x1400, 0x2000, 0x3000, 3, None, 1.0, 1.0, 8, 16, 0x4000, 0x5000, None,
                                   None, None, None)
    assert rc == -1
    assert ops.RULE_SGD_MEMBERS == 3
    rc = lib.esvit_fused_clip_update_ema(ops.RULE_SGD_MEMBERS, 0x1000, 2, 0x2000, 2, 0x3000, 0.0, 0.0, 0.0, 0.9, 0.0, 0.0, 0.0, None, None)
    assert rc == -1 and "skipped" in lib.esvit_last_error().decode()
    assert lib.esvit_fused_clip_update_ema(4, 0x1000, 2, 0x2000, 2, 0x3000, 0.0, 0.0, 0.0, 0.9, 0.0, 0.0, 0.0, 0x4000, None) == -1
    hdr = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "ESVIT_RULE_SGD_MEMBERS %d" % ops.RULE_SGD_MEMBERS in hdr and "ESVIT_Q_PROBE_CE_REG_ROW %d" % ops.Q_PROBE_CE_REG_ROW in hdr
    assert ops.probe_ce_reg_row() >= 1024 and ops.probe_ce_reg_row() % 4 == 0
