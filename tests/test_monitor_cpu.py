"""The training-health monitor without a GPU: the fp32 torch route of esvit_amd.monitor (what runs when the ops module in use has no
dist_stats entry: oracle/ops_ref.py) against the fp64 statement of tests/monitor_ref.py, the plumbing (no host synchronisation in
observe, period arithmetic, ESVIT_MONITOR, train_one_epoch, two gloo ranks), the argument checks of the library's new mode, and the
mutants of the statement, each caught by a named case."""
import math
import os
import types

import pytest
import torch
import torch.multiprocessing as mp

from tests import dino_loss_ref as DR
from tests import golden_utils as GU
from tests import monitor_ref as MR
from tests.test_composition_cpu import cpu_ops, nano_pair  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = [(regime, K, R) for regime in MR.REGIMES for K, R in ((8, 37), (2056, 37), (4096, 37), (65536, 3))]


def fallback(x, c, inv, ref):
    from esvit_amd.monitor import dist_stats_torch
    return dist_stats_torch(x, c, MR.f32(inv), MR.stats_f32(ref))


# ---- the statement and its bounds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime,K,R", TABLE)
def test_fp32_torch_sits_under_an_eighth_of_the_bounds(regime, K, R):
    """the yardstick of the bounds: plain fp32 torch on the same formula; the two forms of the fp64 entropy agree to 1e-12; the entropy
    bound stays below 1e-3 nats on the centred table; and the column-sum scale first proposed (without |z| + |max| + |L|) is NOT met by fp32 torch at the
    peaked K = 65536 case, which is why monitor_ref widens the scale and not the constant"""
    for dt in DR.DTYPES:
        for inv in MR.INV_TEMPS:
            for centered in (True, False):
                x, c = MR.case(regime, R, K, dt, inv, centered=centered)
                ref = MR.dist_ref(x, c, inv)
                assert (ref["ent"] - MR.dist_ref(x, c, inv, entropy="textbook")["ent"]).abs().max().item() < 1e-12
                if centered:  # (rows without a centre in the shifted regime sit at |z| = 500 and beyond: their bound is larger by that much)
                    assert MR.ent_bound(ref).max().item() < 1e-3
                r = MR.ratios(*fallback(x, c, inv, ref), ref, R)
                print("OBSERVED", regime, K, R, DR.dt_name(dt), inv, centered, r)
                assert r["amax_wrong"] == 0
                assert r["ent"] <= 0.125 and r["psum"] <= 0.125 and r["marg"] <= 0.125, r
    if regime == "peaked" and K == 65536:
        x, c = MR.case(regime, R, K, torch.float32, 25.0)
        ref = MR.dist_ref(x, c, 25.0)
        psum = fallback(x, c, 25.0, ref)[2].double()
        assert ((psum - ref["psum"]).abs() / MR.psum_bound(ref, narrow=True)).max().item() > 1.0


def test_closed_forms():
    K, R = 4096, 5
    x = torch.full((R, K), 0.375)
    c = torch.full((K,), 0.125)
    ref = MR.dist_ref(x, c, 25.0)
    assert (ref["ent"] - math.log(K)).abs().max().item() < 1e-12
    ent, amax, psum = fallback(x, c, 25.0, ref)
    assert ((ent.double() - math.log(K)).abs() <= MR.ent_bound(ref)).all()
    assert abs(MR.marginal_entropy(psum, R).item() - math.log(K)) <= MR.marginal_bound(ref, R).item()
    assert amax.tolist() == [0] * R  # every column ties: the lowest index
    # one column dominates: H ~ 0, the marginal entropy of rows that all pick the same column too
    x = torch.zeros(R, K)
    x[:, 77] = 4.0
    ref = MR.dist_ref(x, None, 25.0)
    ent, amax, psum = fallback(x, None, 25.0, ref)
    assert ref["ent"].max().item() < 1e-30 and ent.abs().max().item() <= MR.ent_bound(ref).max().item() and amax.tolist() == [77] * R
    assert MR.marginal_entropy(psum, R).item() < 1e-6


def test_nan_rule_of_the_fallback():
    x, c = MR.case("trained", 5, 64, torch.float32, 25.0)
    ref = MR.dist_ref(x, c, 25.0)
    clean = fallback(x, c, 25.0, ref)
    for bad_value in (float("nan"), float("inf"), float("-inf")):
        xb = x.clone()
        xb[2, 9] = bad_value
        ent, amax, psum = fallback(xb, c, 25.0, ref)
        keep = [0, 1, 3, 4]
        assert torch.isnan(ent[2]) and amax[2].item() == -1 and torch.isnan(psum).all()
        assert torch.equal(ent[keep], clean[0][keep]) and torch.equal(amax[keep], clean[1][keep])


# ---- mutants of the statement, each caught by a named case -----------------------------------------------------------------------------
def _kernel_outputs_pass(ref, mutant):
    """the comparison the tests apply to the code under test, applied to a mutant of the statement"""
    return bool(((mutant["ent"] - ref["ent"]).abs() <= MR.ent_bound(ref)).all()) and bool((mutant["amax"] == ref["amax"]).all()) and \
        bool(((mutant["psum"] - ref["psum"]).abs() <= MR.psum_bound(ref)).all())


def test_mutant_centre_dropped_is_caught_by_the_trained_case():
    x, c = MR.case("trained", 7, 2056, torch.float32, 25.0)
    ref = MR.dist_ref(x, c, 25.0)
    assert _kernel_outputs_pass(ref, ref)
    assert not _kernel_outputs_pass(ref, MR.dist_ref(x, c, 25.0, stats=(ref["max"], ref["lse"]), drop_center=True))


def test_mutant_statistics_of_another_row_is_caught_by_the_trained_case():
    x, c = MR.case("trained", 7, 2056, torch.float32, 25.0)
    ref = MR.dist_ref(x, c, 25.0)
    assert not _kernel_outputs_pass(ref, MR.dist_ref(x, c, 25.0, stats=(ref["max"].roll(1), ref["lse"].roll(1))))


def _sequential_fp32_entropy(x, inv, ref, centred):
    """the entropy with every product and every partial sum of the K-term sum rounded to fp32, one after the other -- the worst
    summation order a kernel could choose -- in the centred form L - sum p d or the uncentred one (max + L) - sum p z"""
    z = (x.double() * MR.f32(inv)).float()
    mx, L = MR.stats_f32(ref)
    p = torch.exp((z - mx[:, None]) - L[:, None])
    if centred:
        return (L - torch.cumsum(p * (z - mx[:, None]), 1)[:, -1]).double()
    return ((mx + L) - torch.cumsum(p * z, 1)[:, -1]).double()


def test_mutant_uncentred_sum_is_caught_by_the_shifted_student_case():
    """rows of the shifted regime without a centre (student rows: z near 300 at inverse temperature 10), K = 65536: sum p z loses
    u |max| per partial sum, sum p d does not"""
    x, _ = MR.case("shifted", 3, 65536, torch.float32, 10.0, centered=False)
    x = x + 10.0  # (the student shift of the regime: logits near 30)
    ref = MR.dist_ref(x, None, 10.0)
    assert ref["max"].min().item() > 250
    ok = ((_sequential_fp32_entropy(x, 10.0, ref, True) - ref["ent"]).abs() <= MR.ent_bound(ref)).all()
    caught = ((_sequential_fp32_entropy(x, 10.0, ref, False) - ref["ent"]).abs() > MR.ent_bound(ref)).any()
    assert bool(ok) and bool(caught)


def tie_case(K, dt, cols):
    """bit-equal maxima at `cols` of every row, with equal centre entries there"""
    x, c = MR.case("trained", 4, K, dt, 25.0, col=cols[0])
    for j in cols[1:]:
        x[:, j] = x[:, cols[0]]
        c[j] = c[cols[0]]
    return x, c


def test_mutant_last_index_on_ties_is_caught_by_the_tie_case():
    x, c = tie_case(2056, torch.float32, (5, 1030, 2055))
    ref = MR.dist_ref(x, c, 25.0)
    assert ref["amax"].tolist() == [5] * 4 and fallback(x, c, 25.0, ref)[1].tolist() == [5] * 4
    assert not _kernel_outputs_pass(ref, MR.dist_ref(x, c, 25.0, argmax="last"))


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
def run_module(which, mc, dev, monitor):
    """one forward / backward of DINOLoss / DDINOLoss on dino_loss_ref.module_case inputs -> (loss, gradients, the loss module)"""
    import esvit_amd
    K = mc["center"].shape[1]
    to = lambda k: mc[k].to(dev)  # noqa: E731
    lf = (esvit_amd.DDINOLoss if which == "ddino" else esvit_amd.DINOLoss)(K, DR.MODULE["ncrops"], 0.04, 0.04, 0, 1).to(dev)
    lf.monitor = monitor
    lf.center.copy_(to("center"))
    sc = to("s_cls").requires_grad_(True)
    if which == "ddino":
        lf.center_grid.copy_(to("center_grid"))
        sr = to("s_reg").requires_grad_(True)
        loss = lf((sc, sr, to("s_fea"), mc["npatch"]), (to("t_cls"), to("t_reg"), to("t_fea"), mc["npatch"]), 0, None)
    else:
        sr = None
        loss = lf(sc, to("t_cls"), 0, None)
    loss.backward()
    lf.synchronize()
    return loss.detach(), [sc.grad] + ([] if sr is None else [sr.grad]), lf


def check_module(which, dt, dev):
    """every key against fp64, and loss / gradients bit-equal with and without the monitor"""
    from esvit_amd.monitor import TrainingMonitor
    mc = DR.module_case(1000, dt)
    ref = MR.module_ref(mc, which, student=True)
    loss0, g0, _ = run_module(which, mc, dev, None)
    loss1, g1, lf = run_module(which, mc, dev, TrainingMonitor(period=1, student=True))
    assert torch.equal(loss0, loss1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    got = lf.monitor.compute()
    assert sorted(got) == MR.public_keys(ref)
    bad, seen = [], {}
    for k in got:
        tol = MR.module_tolerance(ref, k)
        seen[k] = abs(got[k] - ref[k]) / tol
        if not abs(got[k] - ref[k]) <= tol:
            bad.append((k, got[k], ref[k], tol))
    print("OBSERVED", which, DR.dt_name(dt), seen)
    assert not bad, bad
    return got, ref, seen


@pytest.mark.parametrize("which", ["dino", "ddino"])
@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
def test_module_quantities_against_fp64(cpu_ops, which, dt):  # noqa: F811
    got, ref, _ = check_module(which, dt, "cpu")
    if which == "ddino":
        # mutants of the statement: absent terms counted in kl, coverage over both views at once
        for kw, key in ((dict(count_absent=True), "kl"), (dict(count_absent=True), "kl_grid"), (dict(coverage_both_views=True), "match_coverage")):
            mut = MR.module_ref(DR.module_case(1000, dt), which, student=True, **kw)
            assert abs(mut[key] - got[key]) > MR.module_tolerance(ref, key), (kw, key)


def test_observe_never_synchronises(cpu_ops, monkeypatch):  # noqa: F811
    from esvit_amd.monitor import TrainingMonitor
    mc = DR.module_case(1000, torch.float32)
    mon = TrainingMonitor(period=1, student=True)
    inner = mon.observe

    def guarded(*a, **kw):
        def refuse(*_a, **_k):
            raise AssertionError("observe read a value back from the device")
        with monkeypatch.context() as m:
            for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__float__", "__int__"):
                m.setattr(torch.Tensor, name, refuse)
            return inner(*a, **kw)
    mon.observe = guarded
    run_module("ddino", mc, "cpu", mon)
    assert mon.observed == 1 and len(mon.compute()) == 15


def test_period_arithmetic_and_reset(cpu_ops):  # noqa: F811
    import esvit_amd
    from esvit_amd.monitor import TrainingMonitor
    mc = DR.module_case(1000, torch.float32)
    mon = TrainingMonitor(period=3)
    lf = esvit_amd.DINOLoss(1000, DR.MODULE["ncrops"], 0.04, 0.04, 0, 1)
    lf.monitor = mon
    seen = []
    for _ in range(7):
        before = mon.observed
        lf(mc["s_cls"], mc["t_cls"], 0, None)
        seen.append(mon.observed - before)
    assert seen == [1, 0, 0, 1, 0, 0, 1]
    assert "student_entropy" not in mon.compute() and "teacher_entropy" in mon.compute()
    mon.reset()
    assert mon.observed == 0 and mon.compute() == {}
    for bad in (0, -2, 1.5, "3"):
        with pytest.raises(ValueError):
            TrainingMonitor(period=bad)


def test_environment_variable(monkeypatch, lib_built):
    import esvit_amd
    monkeypatch.delenv("ESVIT_MONITOR", raising=False)
    assert esvit_amd.DINOLoss(16, 4, 0.04, 0.04, 0, 1).monitor is None and esvit_amd.DDINOLoss(16, 4, 0.04, 0.04, 0, 1).monitor is None
    monkeypatch.setenv("ESVIT_MONITOR", "4")
    for cls in (esvit_amd.DINOLoss, esvit_amd.DDINOLoss):
        mon = cls(16, 4, 0.04, 0.04, 0, 1).monitor
        assert mon.period == 4 and mon.student is False
    for bad in ("0", "-1", "ten", "1.5", " 3", "+3"):
        monkeypatch.setenv("ESVIT_MONITOR", bad)
        for cls in (esvit_amd.DINOLoss, esvit_amd.DDINOLoss):
            with pytest.raises(ValueError, match="ESVIT_MONITOR"):
                cls(16, 4, 0.04, 0.04, 0, 1)


def test_view_agreement_and_zero_kl(cpu_ops):  # noqa: F811
    """identical teacher views agree on every image; a student whose logits are tau_s / tau_t times the centred teacher logits has
    the teacher's distribution: KL = 0"""
    from esvit_amd.monitor import TrainingMonitor
    mc = dict(DR.module_case(1000, torch.float32))
    B, nc = mc["B"], DR.MODULE["ncrops"]
    mc["t_cls"] = mc["t_cls"][:B].repeat(2, 1)
    mc["s_cls"] = ((mc["t_cls"][:B] - mc["center"]) * (0.1 / 0.04)).repeat(nc, 1)
    _, _, lf = run_module("dino", mc, "cpu", TrainingMonitor(period=1))
    got = lf.monitor.compute()
    ref = MR.module_ref(mc, "dino")
    assert got["view_agreement"] == 1.0 and ref["view_agreement"] == 1.0
    assert abs(ref["kl"]) < 1e-9 and abs(got["kl"]) <= MR.module_tolerance(ref, "kl")


# ---- train_one_epoch ------------------------------------------------------------------------------------------------------------------
class Loader:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter([(b, None) for b in self.batches])


def cpu_updater(student, teacher):
    """a FusedClipAdamWEMA in name (train_one_epoch takes it as it is) whose step is plain SGD + EMA in torch: the update kernels need
    a GPU, the loop around them does not"""
    from esvit_amd.update import FusedClipAdamWEMA

    class CpuUpdater(FusedClipAdamWEMA):
        def __init__(self):
            self.rule, self.student, self.teacher = "sgd", student, teacher

        def step(self, lr, weight_decay, ema_momentum, clip_grad=3.0, skip_last_layer=False):
            with torch.no_grad():
                for p in self.student.parameters():
                    if p.grad is not None:
                        p.add_(p.grad, alpha=-float(lr))
                for q, k in zip(self.student.parameters(), self.teacher.parameters()):
                    k.mul_(ema_momentum).add_((1 - ema_momentum) * q.detach())

        def take_skipped(self):
            return 0

        def zero_grad(self, set_to_none=True):
            for p in self.student.parameters():
                p.grad = None
    return CpuUpdater()


def run_epoch(monitor, batches, n_it=None):
    """engine.train_one_epoch over nano Swin crops on the CPU (kernels: the torch restatement; Tensor.cuda: the identity)"""
    import esvit_amd
    from esvit_amd import engine
    student, teacher = nano_pair()
    loss_fn = esvit_amd.DDINOLoss(GU.NANO_HEAD["out_dim"], 10, 0.04, 0.07, 5, 10)
    loss_fn.monitor = monitor
    n = len(batches)
    args = types.SimpleNamespace(clip_grad=3.0, freeze_last_layer=1, batch_size_per_gpu=2, num_mixup_views=0)
    stats = engine.train_one_epoch(student, teacher, teacher, loss_fn, Loader(batches), cpu_updater(student, teacher), [1e-3] * n, [0.04] * n,
                                   [0.99] * n, 0, None, None, args)
    return stats, student


def test_train_one_epoch_keys_and_identical_trajectory(cpu_ops, monkeypatch, capsys):  # noqa: F811
    from esvit_amd.monitor import TrainingMonitor
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    batches = [GU.make_crops(2, seed=70 + i) for i in range(3)]
    plain, s0 = run_epoch(None, batches)
    assert set(plain) == {"loss", "lr", "wd"}
    capsys.readouterr()
    mon = TrainingMonitor(period=2, student=True)
    with_mon, s1 = run_epoch(mon, batches)
    printed = capsys.readouterr().out
    assert {k: with_mon[k] for k in plain} == plain
    assert all(torch.equal(a, b) for a, b in zip(s0.parameters(), s1.parameters()))
    new = set(with_mon) - set(plain)
    assert new == {"teacher_entropy", "teacher_marginal_entropy", "teacher_pmax", "kl", "center_absmax", "student_entropy", "view_agreement",
                   "teacher_entropy_grid", "teacher_marginal_entropy_grid", "teacher_pmax_grid", "kl_grid", "center_absmax_grid",
                   "student_entropy_grid", "match_similarity", "match_coverage"}
    assert all(math.isfinite(with_mon[k]) for k in new)
    K = GU.NANO_HEAD["out_dim"]
    assert 0 < with_mon["teacher_entropy"] <= math.log(K) + 1e-6 and 0 < with_mon["match_coverage"] <= 1 and with_mon["kl"] >= -1e-6
    # looks at iterations 0 and 2 (the last): one line each, steps 0 and 2 observed
    assert printed.count("monitor [it ") == 2


def _epoch_worker(rank, world, port, out):
    from tests.test_dist_cpu import _init
    _init(rank, world, port)
    import esvit_amd.functional as Fn
    import esvit_amd.loss as L
    import esvit_amd.params as P
    from esvit_amd.monitor import TrainingMonitor
    from oracle import ops_ref
    for mod in (Fn, L, P):
        mod.ops = ops_ref
    ops_ref.set_act_dtype(torch.float32)
    torch.Tensor.cuda = lambda self, *a, **k: self
    batches = [GU.make_crops(2, seed=90 + 10 * rank + i) for i in range(2)]
    stats, _ = run_epoch(TrainingMonitor(period=1), batches)
    out[rank] = stats
    import torch.distributed as dist
    dist.destroy_process_group()


def test_two_gloo_ranks_get_the_same_averaged_values(lib_built):
    out = mp.Manager().dict()
    mp.spawn(_epoch_worker, args=(2, 29641, out), nprocs=2, join=True)
    a, b = out[0], out[1]
    assert set(a) == set(b) and len(a) == 3 + 13
    for k in a:
        if k not in ("lr", "wd"):
            assert a[k] == b[k], (k, a[k], b[k])


# ---- the library's new mode ---------------------------------------------------------------------------------------------------------
def test_library_argument_checks_come_before_any_launch(lib_built):
    """plausible, never dereferenced addresses: the checks of terms = -1 answer -1 before any device call and name the mode"""
    from esvit_amd import _lib, ops
    lib = _lib.lib

    def call(dtype=_lib.BF16, s=0x1000, t=None, center=0x2000, t_max=None, tmatch=None, row_w=None, term_w=None, inv=25.0, Rs=40, K=64,
             row_loss=0x4000, ds=0x5000, row_order=None, s_max=0x6000, s_lse=0x7000):
        rc = lib.esvit_dino_ce_fwd_bwd(dtype, s, t, center, t_max, None, tmatch, row_w, -1, term_w, inv, 1.0, Rs, K, row_loss, ds, row_order, s_max,
                                       s_lse, None)
        return rc, lib.esvit_last_error().decode()

    for kw in (dict(s_max=None), dict(s_lse=None), dict(s_max=None, s_lse=None), dict(t=0x8000), dict(t_max=0x8000), dict(tmatch=0x8000),
               dict(row_w=0x8000), dict(term_w=0x8000), dict(row_order=0x8000), dict(K=12), dict(K=0), dict(K=1 << 24), dict(dtype=2), dict(dtype=-1),
               dict(s=None), dict(row_loss=None), dict(ds=None), dict(Rs=0), dict(inv=0.0), dict(inv=-1.0), dict(s=0x1008), dict(ds=0x5004),
               dict(center=0x2004)):
        rc, msg = call(**kw)
        assert rc == -1 and "terms = -1" in msg, (kw, rc, msg)
    # the query: the slab height, and K column sums + one partial per slab + one record per (row, block of 65536 columns)
    slab = ops.query(ops.Q_DIST_STATS, 0)
    assert slab == ops.dist_stats_slab() == 32
    assert ops.query(ops.Q_DIST_STATS, 1, 64) == 2 * 64 + 4 and ops.query(ops.Q_DIST_STATS, slab, 64) == 2 * 64 + 4 * slab
    assert ops.query(ops.Q_DIST_STATS, slab + 1, 65544) == 3 * 65544 + 4 * (slab + 1) * 2
    assert ops.query(ops.Q_DIST_STATS, 12544, 65536) == (1 + 12544 // slab) * 65536 + 4 * 12544
    assert ops.query(ops.Q_DIST_STATS, -1, 64) == -1 and ops.query(ops.Q_DIST_STATS, 5, 0) == -1
    hdr = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "#define ESVIT_Q_DIST_STATS %d" % ops.Q_DIST_STATS in hdr and "terms = -1: DISTRIBUTION STATISTICS" in hdr
    assert "esvit_query(ESVIT_Q_DIST_STATS, Rs, K)" in hdr
