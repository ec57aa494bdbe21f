"""The fp64 statement of the DINO loss (tests/dino_loss_ref.py) and the inputs of tests/test_dino_loss_gpu.py, proved without a GPU:
ce_ref is anchored to the oracle's dino_loss / ddino_loss (themselves anchored to the reference project's goldens), every GPU case
runs on the fp32 / bf16 restatement (oracle/ops_ref.py) under the same metrics and bounds, the region-matching inputs have the gaps
and ties they claim, and two mutations of the restatement are caught by the cases meant to catch them."""
import pytest
import torch

from oracle import esvit_oracle as O
from oracle import ops_ref
from tests import dino_loss_ref as DR
from tests import golden_utils as GU

CPU = torch.device("cpu")
# The bounds are the GPU's (3x the deltas committed in profiles/dino_loss_parity_observed.jsonl).  Where the kernel's delta happened to
# come out below the resolution of fp32 itself (a scalar loss that rounded the lucky way: 7e-9), 3x that figure says nothing about the
# inputs, and plain fp32 torch, whose summation order changes from build to build, cannot be held to it: the restatement is held to the
# GPU bound or to ten fp32 roundings, whichever is larger.  A wrong table or a badly conditioned input shows at 1e-4 and above.
FLOOR = 10 * 2.0 ** -24
REG_K = [(r, K) for r in ("flat", "trained", "peaked") for K in DR.KS] + [("shifted", 2056)]
IDS = ["%s-K%d" % rk for rk in REG_K]


@pytest.fixture(autouse=True)
def _fp32_restatement(lib_built):
    ops_ref.set_act_dtype(torch.float32)
    yield
    ops_ref.set_act_dtype(torch.float32)


# ---- ce_ref == the oracle, to fp64 round-off ----------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def test_ce_ref_equals_oracle_dino_loss():
    from esvit_amd.loss import DINOLoss
    B, nc, K = 3, 10, 72
    g = torch.Generator().manual_seed(11)
    s, t, c = torch.randn(nc * B, K, generator=g) * 0.25, torch.randn(2 * B, K, generator=g) * 0.25, torch.randn(1, K, generator=g) * 0.05
    tm, w = DINOLoss(K, nc, 0.04, 0.07, 0, 1)._static(B, CPU)
    exact = torch.full((nc * B,), 1.0 / ((2 * nc - 2) * B), dtype=torch.float64)
    assert torch.equal(w, exact.float())  # the host table holds the correctly rounded weight; the anchor uses the exact one
    rl, ds = DR.ce_ref(s, t, c, tm, exact, DR.INV_ST, 1.0 / 0.07)
    s64 = s.double().requires_grad_(True)
    loss, _ = O.dino_loss(s64, t.double(), c.double(), 0.07, nc)
    loss.backward()
    assert abs(rl.sum().item() - loss.item()) <= 1e-12 * abs(loss.item())
    assert _rel(ds, s64.grad) <= 1e-12


def test_ce_ref_equals_oracle_mixup_loss():
    mc = GU.MIXUP
    s, t, c, T = GU.mixup_case()
    tm, tw, B, nc = DR.mixup_tables()
    n_terms = 2 * nc - 2
    # the exact weights of the table's live entries: T_v[a, b] / (n_terms B) for student row (v, b) against teacher row iq B + a
    T64 = torch.stack([m.double() for m in T])
    exact = torch.zeros(tm.shape, dtype=torch.float64)
    for r in range(tm.shape[0]):
        v, b = divmod(r, B)
        for j in range(4):
            if tm[r, j] >= 0:
                exact[r, j] = T64[v, int(tm[r, j]) % B, b] / (n_terms * B)
    assert torch.allclose(tw.double()[tm >= 0], exact[tm >= 0], rtol=2e-7, atol=0)  # (the weight of an absent term is never read)
    # and the table drops nothing: per student row and view the live weights sum to the column sum of T_v
    for iq in range(2):
        live = exact[:, 2 * iq:2 * iq + 2].sum(1).view(nc, B) * (n_terms * B)
        want = T64.sum(1)
        want[iq] = 0
        assert torch.allclose(live, want, rtol=1e-12, atol=0)
    temp = O.teacher_temp(2, 0.04, 0.07, 5, 10)
    rl, ds = DR.ce_ref(s, t, c, tm, exact, DR.INV_ST, 1.0 / temp)
    s64 = s.double().requires_grad_(True)
    loss, _ = O.dino_loss(s64, t.double(), c.double(), temp, mc["ncrops"], targets_mixup=[m.double() for m in T])
    loss.backward()
    assert abs(rl.sum().item() - loss.item()) <= 1e-12 * abs(loss.item())
    assert _rel(ds, s64.grad) <= 1e-12


def test_ce_ref_equals_oracle_ddino_loss():
    """cls rows with DDINOLoss._static's tables, region rows with region_match_ref on the fp64 cosine similarities"""
    from esvit_amd.loss import DDINOLoss
    case = DR.module_case(72, torch.float32)
    assert DR.module_gap(case) >= 1e-3
    B, Tt, S, nc = case["B"], case["Tt"], case["S"], DR.MODULE["ncrops"]
    tb = DDINOLoss(72, nc, 0.04, 0.04, 0, 1)._static(B, case["npatch"], Tt, CPU)
    n_terms = 2 * nc - 2
    w_cls = torch.full((nc * B,), 0.5 / (n_terms * B), dtype=torch.float64)
    w_reg = torch.cat([torch.full((B * sz,), 0.5 / (n_terms * B * sz), dtype=torch.float64) for sz in case["sizes"]])
    assert torch.equal(tb["w_cls"], w_cls.float()) and torch.equal(tb["w_reg"], w_reg.float())
    cm = tb["cm_row"].long()
    assert torch.equal(cm.sort().values, torch.arange(B * S))  # every row is written exactly once through cm_row
    F = torch.nn.functional
    sfn = F.normalize(case["s_fea"].double(), dim=-1)[cm].view(B, S, -1)                     # image-major
    tfn = F.normalize(case["t_fea"].double(), dim=-1)[tb["t_perm"].long()].view(B, 2 * Tt, -1)
    sim = torch.bmm(sfn, tfn.transpose(1, 2))
    tm_reg = DR.region_match_ref(sim, Tt, tb["crop_id"], tb["cm_row"])
    assert int((tm_reg == -7).sum()) == 0
    rl_c, ds_c = DR.ce_ref(case["s_cls"], case["t_cls"], case["center"], tb["tm_cls"], w_cls, DR.INV_ST, 25.0)
    rl_g, ds_g = DR.ce_ref(case["s_reg"], case["t_reg"], case["center_grid"], tm_reg, w_reg, DR.INV_ST, 25.0)
    ref = DR.module_ref(case, "ddino")
    assert abs(rl_c.sum().item() + rl_g.sum().item() - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert _rel(ds_c, ref["g_cls"]) <= 1e-12 and _rel(ds_g, ref["g_reg"]) <= 1e-12


# ---- every GPU case on the restatement, same metrics, same bounds --------------------------------------------------------------------
def _o(dt):
    ops_ref.set_act_dtype(dt)
    return ops_ref


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
@pytest.mark.parametrize("regime,K", REG_K, ids=IDS)
def test_two_term_cases_on_the_restatement(regime, K, dt):
    worst, _, broken = DR.eval_two_term(_o(dt), CPU, regime, K, dt)
    assert not broken, broken
    DR.check(DR.family("dino_ce2", regime, dt, K), worst, case="restatement", floor=FLOOR)


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
@pytest.mark.parametrize("regime", ["trained", "flat"])
@pytest.mark.parametrize("K", DR.KS)
def test_four_term_cases_on_the_restatement(regime, K, dt):
    worst, _, broken = DR.eval_four_term(_o(dt), CPU, regime, K, dt)
    assert not broken, broken
    DR.check(DR.family("dino_ce4", regime, dt, K), worst, case="restatement", floor=FLOOR)


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
@pytest.mark.parametrize("regime", list(DR.REGIMES))
@pytest.mark.parametrize("K", DR.KS)
def test_teacher_stats_cases_on_the_restatement(regime, K, dt):
    DR.check(DR.family("teacher_row_stats", regime, dt, K), DR.eval_teacher_stats(_o(dt), CPU, regime, K, dt), case="restatement", floor=FLOOR)


def test_rowstat_cases_on_the_restatement():
    worst = {}
    for R in DR.ROWSTAT_R:
        for nb in DR.ROWSTAT_NB:
            for k, v in DR.eval_rowstat(ops_ref, CPU, R, nb).items():
                worst[k] = max(worst.get(k, 0.0), v)
    DR.check("rowstat_combine/fp32", worst, case="restatement", floor=FLOOR)


def test_rowstat_blocks_are_what_they_claim():
    for where in DR.ROWSTAT_WHERE:
        st = DR.rowstat_blocks(5, 65, where).double()
        m = st[..., 0]
        top = m.max(1).values
        assert bool((m.argmax(1) == (where if where >= 0 else 65 + where)).all())
        far = m < top[:, None] - 200
        assert int(far.sum()) > 0 and bool((torch.exp2(m - top[:, None])[far].float() == 0).all())  # they contribute exactly nothing in fp32


def test_center_chain_on_the_restatement():
    for rows, K, dt in DR.CENTER_SHAPES:
        DR.check("center_chain/%s" % DR.dt_name(dt), DR.eval_center_chain(_o(dt), CPU, rows, K, dt), case="restatement_%dx%d" % (rows, K), floor=FLOOR)


@pytest.mark.parametrize("layout", list(DR.REGION_LAYOUTS))
def test_region_cases_have_their_gaps_and_ties_and_the_restatement_matches(layout):
    B, S, Tt, ld, crop_id, cm_row = DR.region_tables(layout)
    assert torch.equal(cm_row.long().sort().values, torch.arange(B * S))
    for kind in DR.REGION_KINDS:
        sim, ties = DR.region_sim(layout, kind)
        gap, (nmin, nmax) = DR.top2_gap_and_ties(sim, Tt)
        if Tt == 1:
            assert (nmin, nmax) == (1, 1)
        elif ties == 1:
            assert gap >= 1e-3 and (nmin, nmax) == (1, 1), (kind, gap)
        else:
            assert (nmin, nmax) == (ties, ties) and gap == 0.0, (kind, nmin, nmax)
        if ld > 2 * Tt:
            assert bool((sim[:, :, 2 * Tt:] == DR.PAD).all())
        want = DR.region_match_ref(sim, Tt, crop_id, cm_row)
        assert int((want == -7).sum()) == 0
        got = ops_ref.region_match(sim, Tt, crop_id, cm_row, torch.full((B * S, 2), -7, dtype=torch.int32))
        assert torch.equal(got, want), kind
        live = want[want >= 0]
        if kind == "win_first":
            assert bool((live % Tt == 0).all())
        if kind == "win_last":
            assert bool((live % Tt == Tt - 1).all())
        if kind == "tie2" and Tt >= 2:
            assert bool((live % Tt == Tt // 3).all())
        if kind == "tie_all":
            assert bool((live % Tt == 0).all())


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
@pytest.mark.parametrize("K", [72, 1000])
@pytest.mark.parametrize("which", ["ddino", "dino"])
def test_modules_on_the_restatement(which, K, dt, monkeypatch):
    import esvit_amd.loss as L
    monkeypatch.setattr(L, "ops", _o(dt))
    assert DR.module_gap(DR.module_case(K, dt)) >= 1e-3
    DR.check(DR.family("module_" + which, "trained", dt, K), DR.eval_module(which, K, dt, CPU), case="restatement", floor=FLOOR)


# ---- the cases discriminate: two mutations of the restatement --------------------------------------------------------------------------
def _drop_center_tail(c):
    c = c.clone()
    c[:, -8:] = 0
    return c


@pytest.mark.parametrize("regime,K", [("flat", 1000), ("flat", 2056), ("flat", 4096)])
def test_dropping_the_centre_in_the_last_columns_fails_the_flat_case(regime, K):
    worst, _, _ = DR.eval_two_term(ops_ref, CPU, regime, K, torch.float32, center_mutation=_drop_center_tail)
    assert worst["ds_rel"] > DR.bound(DR.family("dino_ce2", regime, torch.float32, K), "ds_rel") > 0
    assert worst["ds_rel"] > 1e-4  # (whatever the committed bound: two orders above fp32 round-off)


@pytest.mark.parametrize("K", [1000, 2056])
def test_dropping_the_centre_in_the_last_columns_fails_the_tail_placed_cases(K):
    _, lines, _ = DR.eval_two_term(ops_ref, CPU, "trained", K, torch.float32, center_mutation=_drop_center_tail)
    fam = DR.family("dino_ce2", "trained", torch.float32, K)
    lim = DR.bound(fam, "ds_rel")
    tail = [ln for ln in lines if ln["case"].startswith(("place_ta_last", "place_tb_last"))]
    assert len(tail) == 4 and lim > 0
    for ln in tail:
        assert ln["ds_rel"] > max(lim, 1e-3) and ln["loss_rel"] > max(DR.bound(fam, "loss_rel"), 1e-4), ln


def _dino_ce_first_offset_for_both(s, t, center, t_max, t_lse, tmatch, row_w, inv_st, inv_tt, **kw):
    """oracle/ops_ref.dino_ce (two-term form) with one mistake: the second term is normalised with the first term's row statistics"""
    z = s.float() * inv_st
    lse = torch.logsumexp(z, 1)
    ps = torch.exp(z - lse[:, None])
    tm = tmatch.view(-1, 2).long()
    n = (tm >= 0).sum(1).float()
    first = torch.where(tm[:, 0] >= 0, tm[:, 0], tm[:, 1]).clamp(min=0)
    off = (t_max[first] + t_lse[first])[:, None]
    pt = torch.zeros_like(z)
    for j in range(2):
        ii = tm[:, j].clamp(min=0)
        pt = pt + torch.exp((t.float()[ii] - center.view(1, -1)) * inv_tt - off) * (tm[:, j] >= 0)[:, None]
    return row_w * (n * lse - (pt * z).sum(1)), (row_w * inv_st)[:, None] * (n[:, None] * ps - pt)


def test_one_offset_for_both_terms_fails_a_two_term_case():
    class Mutant:
        teacher_row_stats = staticmethod(ops_ref.teacher_row_stats)
        dino_ce = staticmethod(_dino_ce_first_offset_for_both)
    good, _, _ = DR.eval_two_term(ops_ref, CPU, "trained", 1000, torch.float32)
    fam = DR.family("dino_ce2", "trained", torch.float32, 1000)
    DR.check(fam, good, case="restatement", floor=FLOOR)
    worst, lines, _ = DR.eval_two_term(Mutant, CPU, "trained", 1000, torch.float32)
    assert worst["ds_rel"] > max(DR.bound(fam, "ds_rel"), 1e-3)
    assert worst["sum_rel"] > max(DR.bound(fam, "sum_rel"), 1e-3)  # the teacher terms no longer sum to one
    # the case has two-term rows whose two teacher rows differ (and their statistics with them)
    tm = DR.two_term_tables(37, DR.RT)[0]
    both = (tm >= 0).all(1)
    assert int((tm[both, 0] != tm[both, 1]).sum()) >= 3
