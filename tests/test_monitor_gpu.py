"""-m gpu: the row-statistics mode of esvit_dino_ce_fwd_bwd (terms = -1, esvit_amd/csrc/monitor.hip) through the C ABI against the fp64
statement and the bounds of tests/monitor_ref.py, and the monitor on the device: ops.dist_stats against the torch route, the
DDINOLoss module, two trainer steps with the statistics handed over by the last-layer GEMMs.  The observed error / bound ratios are
recorded (golden_utils.record_parity; committed as profiles/monitor_parity_observed.jsonl) -- for the record, not as a bound."""
import ctypes as C

import pytest
import torch

from tests import dino_loss_ref as DR
from tests import golden_utils as GU
from tests import monitor_ref as MR
from tests.test_composition_cpu import nano_pair
from tests.test_monitor_cpu import check_module, tie_case

pytestmark = pytest.mark.gpu

MOAT = 64
SENTINEL = -7.25


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def slab():
    from esvit_amd import ops
    return ops.dist_stats_slab()


def raw_call(x, c, inv, stats, dev=None, expect=0):
    """one launch through the C ABI into buffers with sentinel moats around row_loss and around the queried extent of the buffer
    -> (ent, amax, psum, every float the call could write) on the CPU; the moats are checked here"""
    from esvit_amd import _lib, ops
    dev = dev or _dev()
    R, K = x.shape
    n = ops.query(ops.Q_DIST_STATS, R, K)
    assert n == (1 + -(-R // slab())) * K + 4 * R * -(-K // 65536)
    xd = x.to(dev).contiguous()
    cd = None if c is None else c.to(dev).float().contiguous()
    mx, lse = (s.to(dev).float().contiguous() for s in stats)
    out = torch.full((2 * R + 2 * MOAT,), SENTINEL, dtype=torch.float32, device=dev)
    buf = torch.full((n + 2 * MOAT,), SENTINEL, dtype=torch.float32, device=dev)
    p = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + 4 * off)  # noqa: E731
    rc = _lib.lib.esvit_dino_ce_fwd_bwd(_lib.BF16 if x.dtype == torch.bfloat16 else _lib.F32, p(xd), None, p(cd), None, None, None, None, -1, None,
                                        MR.f32(inv), 1.0, R, K, p(out, MOAT), p(buf, MOAT), None, p(mx), p(lse),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == expect, (rc, _lib.lib.esvit_last_error().decode())
    torch.cuda.synchronize()
    out, buf = out.cpu(), buf.cpu()
    for t in (out, buf):
        assert bool((t[:MOAT] == SENTINEL).all()) and bool((t[-MOAT:] == SENTINEL).all()), "a write outside the documented extent"
    body = out[MOAT:-MOAT].view(R, 2)
    return body[:, 0].clone(), body[:, 1].clone(), buf[MOAT:MOAT + K].clone(), torch.cat([out, buf])


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_case(x, c, inv, record=None, **tag):
    """reference statistics rounded to fp32, two launches with equal bits, every output against its bound -> the ratios"""
    R = x.shape[0]
    ref = MR.dist_ref(x, c, inv)
    ent, amax, psum, everything = raw_call(x, c, inv, MR.stats_f32(ref))
    again = raw_call(x, c, inv, MR.stats_f32(ref))[3]
    assert same_bits(everything, again), "two identical launches differ"
    assert bool((amax == amax.round()).all())
    r = MR.ratios(ent, amax.long(), psum, ref, R)
    if record is not None:
        record.append(dict(tag, **r))
    assert r["amax_wrong"] == 0, (tag, r)
    assert r["ent"] <= 1.0 and r["psum"] <= 1.0 and r["marg"] <= 1.0, (tag, r)
    return r


def _flush(test, records):
    worst = {}
    for r in records:
        for k in ("ent", "psum", "marg", "ent_abs"):
            worst[k] = max(worst.get(k, 0.0), r[k])
    GU.record_parity(test="monitor", case=test, cases=len(records), **worst)


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
@pytest.mark.parametrize("regime", sorted(MR.REGIMES))
def test_row_statistics_against_fp64(regime, dt, lib_built):
    """K: one vector / a whole sweep plus a straggler vector / whole sweeps; R: one row, slab - 1, slab + 1 and 2 slab + 5 (the partly
    filled last slab, the fold over three partials); centre given and NULL; inverse temperatures 25 and 10; K = 65536 at R = 3, and
    K = 65544 (a second block of columns of one vector: the fold over two records per row)"""
    s = slab()
    records = []
    for K, rows in ((8, (1, s - 1, s + 1, 2 * s + 5)), (2056, (1, s - 1, s + 1, 2 * s + 5)), (4096, (1, s - 1, s + 1, 2 * s + 5)), (65536, (3,)), (65544, (3,))):
        for R in rows:
            for centered in (True, False):
                for inv in (25.0, 10.0):
                    x, c = MR.case(regime, R, K, dt, inv, centered=centered)
                    run_case(x, c, inv, records, regime=regime, dt=DR.dt_name(dt), K=K, R=R, centered=centered, inv_temp=inv)
    _flush("table/%s/%s" % (regime, DR.dt_name(dt)), records)


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
def test_placed_maximum_first_last_and_straggler_column(dt, lib_built):
    records = []
    for K in (2056, 4096):
        for col in (0, K - 1, DR.straggler_col(K, dt)):
            x, c = MR.case("trained", slab() + 1, K, dt, 25.0, col=col)
            r = run_case(x, c, 25.0, records, K=K, col=col)
            assert r["amax_wrong"] == 0
    for col in (65535, 65536, 65543):  # the winner in the last vector of the first block of columns, in the second block
        x, c = MR.case("trained", 3, 65544, dt, 25.0, col=col)
        run_case(x, c, 25.0, records, K=65544, col=col)
    _flush("placed/%s" % DR.dt_name(dt), records)


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
def test_ties_take_the_lowest_index(dt, lib_built):
    """bit-equal maxima with equal centre entries: within one thread's vector, across threads of a wave, across waves, across sweeps"""
    for K, cols in ((8, (2, 5)), (2056, (5, 6)), (2056, (40, 700)), (2056, (9, 2050)), (4096, (300, 1030, 4095)), (4096, (2100, 2047 + 2048))):
        x, c = tie_case(K, dt, cols)
        ref = MR.dist_ref(x, c, 25.0)
        assert ref["amax"].tolist() == [cols[0]] * x.shape[0]
        ent, amax, psum, _ = raw_call(x, c, 25.0, MR.stats_f32(ref))
        assert amax.tolist() == [float(cols[0])] * x.shape[0], (K, cols, amax)
        assert bool(((ent.double() - ref["ent"]).abs() <= MR.ent_bound(ref)).all())


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
def test_a_bad_row_between_clean_rows(dt, lib_built):
    """NaN / inf logits or statistics: that row NaN and -1, every column sum NaN, every other row's outputs bit for bit what they were"""
    s = slab()
    for R, K, bad_row, bad_col in ((2 * s + 5, 2056, s + 3, 1031), (3, 65544, 1, 65540)):  # (K = 65544: the second of two column blocks sees the logit)
        _bad_row_case(dt, R, K, bad_row, bad_col)


def _bad_row_case(dt, R, K, bad_row, bad_col):
    x, c = MR.case("trained", R, K, dt, 25.0)
    ref = MR.dist_ref(x, c, 25.0)
    mx, lse = MR.stats_f32(ref)
    ent0, amax0, psum0, _ = raw_call(x, c, 25.0, (mx, lse))
    assert bool(torch.isfinite(ent0).all()) and bool(torch.isfinite(psum0).all())
    keep = [r for r in range(R) if r != bad_row]
    for what in ("nan_logit", "inf_logit", "ninf_logit", "nan_max", "nan_lse", "inf_max"):
        xb, mb, lb = x.clone(), mx.clone(), lse.clone()
        if what.endswith("logit"):
            xb[bad_row, bad_col] = {"nan": float("nan"), "inf": float("inf"), "ninf": float("-inf")}[what.split("_")[0]]
        elif what.endswith("max"):
            mb[bad_row] = float("nan") if what.startswith("nan") else float("inf")
        else:
            lb[bad_row] = float("nan")
        ent, amax, psum, _ = raw_call(xb, c, 25.0, (mb, lb))
        assert bool(torch.isnan(ent[bad_row])) and amax[bad_row].item() == -1.0, (what, ent[bad_row], amax[bad_row])
        assert bool(torch.isnan(psum).all()), what
        assert same_bits(ent[keep], ent0[keep]) and same_bits(amax[keep], amax0[keep]), what


def test_refused_calls_write_nothing(lib_built):
    x, c = MR.case("trained", 5, 64, torch.float32, 25.0)
    ref = MR.dist_ref(x, c, 25.0)
    out = raw_call(x, c, 0.0, MR.stats_f32(ref), expect=-1)[3]   # a zero inverse temperature
    assert bool((out == SENTINEL).all())
    out = raw_call(x[:, :60].contiguous(), c[:60].contiguous(), 25.0, MR.stats_f32(ref), expect=-1)[3]   # K % 8 != 0
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
def test_ops_dist_stats_against_the_torch_route(dt, lib_built):
    """the same fp32 statistics (the library's own, esvit_teacher_row_stats) into the kernel and into monitor.dist_stats_torch: both
    lie within their bound of the fp64 value for these statistics, so within two bounds of each other; student rows without a centre too"""
    from esvit_amd import ops
    from esvit_amd.monitor import dist_stats_torch
    dev = _dev()
    for K, R, centered, inv in ((2056, slab() + 1, True, 25.0), (4096, 2 * slab() + 5, False, 10.0)):
        x, c = MR.case("trained", R, K, dt, inv, centered=centered)
        xd, cd = x.to(dev), (torch.zeros(K) if c is None else c).to(dev)
        stats = ops.teacher_row_stats(xd, cd, MR.f32(inv))
        ent, amax, psum = ops.dist_stats(xd, cd if centered else None, MR.f32(inv), stats)
        assert ent.dtype == torch.float32 and amax.dtype == torch.int32 and psum.shape == (K,)
        ent2, amax2, psum2 = dist_stats_torch(xd, cd if centered else None, MR.f32(inv), stats)
        ref = MR.dist_ref(x, c, inv)
        assert torch.equal(amax.cpu(), amax2.cpu()) and torch.equal(amax.cpu().long(), ref["amax"])
        assert bool(((ent - ent2).abs().cpu().double() <= 2 * MR.ent_bound(ref)).all())
        assert bool(((psum - psum2).abs().cpu().double() <= 2 * MR.psum_bound(ref)).all())


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
def test_ddino_module_on_the_device(dt, lib_built):
    """the DDINOLoss module of the CPU test on the device: loss and gradients bit-equal with the monitor on and off, every key against fp64"""
    import esvit_amd
    try:
        esvit_amd.set_precision("fp32" if dt == torch.float32 else "bf16")
        _, _, seen = check_module("ddino", dt, _dev())
        GU.record_parity(test="monitor", case="module_ddino/%s" % DR.dt_name(dt), **seen)
    finally:
        esvit_amd.set_precision("bf16")


def test_trainer_steps_with_the_statistics_from_the_gemm(lib_built, monkeypatch):
    """two EsvitTrainer.step of the nano Swin configuration, monitor period 1: the monitor reads the statistics the heads' last-layer
    GEMMs handed over (not one esvit_teacher_row_stats launch), and the losses have the bits of the monitor-off run"""
    import esvit_amd
    import esvit_amd.loss as L
    from esvit_amd import ops
    from esvit_amd import params as P
    from esvit_amd.engine import EsvitTrainer
    from esvit_amd.monitor import TrainingMonitor
    dev = _dev()
    esvit_amd.set_precision("bf16")
    calls = {"t": 0, "d": 0}
    f0, d0 = ops.teacher_row_stats, ops.dist_stats
    monkeypatch.setattr(ops, "teacher_row_stats", lambda *a, **k: (calls.__setitem__("t", calls["t"] + 1), f0(*a, **k))[1])
    monkeypatch.setattr(ops, "dist_stats", lambda *a, **k: (calls.__setitem__("d", calls["d"] + 1), d0(*a, **k))[1])
    was = esvit_amd.is_deterministic()
    esvit_amd.set_deterministic(True)  # (the second loss depends on the first update: its bits are promised in this mode)
    crops = [[c.to(dev) for c in GU.make_crops(64, seed=40 + i)] for i in range(2)]  # B = 64: every logits tensor in whole 128-row tiles

    def run(monitor):
        P.clear()
        student, teacher = nano_pair()
        student, teacher = student.to(dev), teacher.to(dev)
        loss_fn = L.DDINOLoss(GU.NANO_HEAD["out_dim"], 10, 0.04, 0.07, 5, 10).to(dev)
        loss_fn.monitor = monitor
        tr = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=0)
        calls["t"] = calls["d"] = 0
        losses = [tr.step(crops[i], 5e-4, 0.04, 0.996, epoch=i) for i in range(2)]
        torch.cuda.synchronize()
        tr.reducer.close()
        return torch.stack(losses).cpu(), dict(calls)

    try:
        off, n_off = run(None)
        mon = TrainingMonitor(period=1)
        on, n_on = run(mon)
        assert n_off == {"t": 0, "d": 0} and n_on == {"t": 0, "d": 4}, (n_off, n_on)
        assert same_bits(on, off), (on, off)
        got = mon.compute()
        assert mon.observed == 2 and len(got) == 13 and all(v == v and abs(v) < 1e30 for v in got.values()), got
        K = GU.NANO_HEAD["out_dim"]
        assert 0 < got["teacher_entropy_grid"] <= torch.log(torch.tensor(float(K))).item() + 1e-5 and 0 < got["match_coverage"] <= 1
    finally:
        esvit_amd.set_deterministic(was)
