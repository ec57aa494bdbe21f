"""The DINO loss kernels on the MI355X (esvit_amd/csrc/dino_loss.hip behind esvit_amd.ops and esvit_amd.loss) against the fp64 statement
of tests/dino_loss_ref.py: every entry point, the regimes of a fresh, a trained and an un-normalised head, row widths that leave a
partial sweep or a straggler vector, row maxima placed where a column fault would hide, every term count, and the exact properties
that need no tolerance.  The cases, metrics and bounds are those tests/test_dino_loss_cpu.py proves on the restatement.

Every fp32 bound is 3x the delta committed in profiles/dino_loss_parity_observed.jsonl for the case's family (entry point / regime /
dtype / row width).  One family is badly conditioned by construction and its figures say so: at K = 8 in the peaked regime a student
and a teacher softmax that are both one-hot at the same column leave a row whose exact gradient is 1.3e-5 of the two terms that
cancel in it, so the per-row metric reads 1.4e-1 on the kernel and 6e-2 on plain fp32 torch, against 1e-5 at the other widths."""
import pytest
import torch

from tests import dino_loss_ref as DR
from tests import golden_utils as GU

pytestmark = pytest.mark.gpu

REG_K = [(r, K) for r in ("flat", "trained", "peaked") for K in DR.KS] + [("shifted", 2056)]  # (shifted adds no code path over trained)
IDS = ["%s-K%d" % rk for rk in REG_K]


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


DEV = torch.device("cuda:0")


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
@pytest.mark.parametrize("regime,K", REG_K, ids=IDS)
def test_dino_ce_two_terms(ops, regime, K, dt):
    """loss and gradient per row against ce_ref with the library's own teacher statistics and with the fp64 ones; rows without a term
    are exactly zero, a one-term row does not depend on its slot, row_order changes nothing; in fp32 the gradient of a row sums to
    zero within the allowance"""
    worst, lines, broken = DR.eval_two_term(ops, DEV, regime, K, dt)
    for ln in lines:
        print("CASE", regime, K, DR.dt_name(dt), ln)
    assert not broken, broken
    DR.check(DR.family("dino_ce2", regime, dt, K), worst, record=GU.record_parity, case="mi355x")


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
@pytest.mark.parametrize("regime", ["trained", "flat"])
@pytest.mark.parametrize("K", DR.KS)
def test_dino_ce_four_weighted_terms(ops, regime, K, dt):
    """dino_ce_terms_kernel: 0 .. 4 live terms, a live entry of weight zero, one teacher row named twice, and the tables
    DINOLoss._mixup_terms makes of the mixup fixture; a row without a live term is exactly zero"""
    worst, lines, broken = DR.eval_four_term(ops, DEV, regime, K, dt)
    for ln in lines:
        print("CASE", regime, K, DR.dt_name(dt), ln)
    assert not broken, broken
    DR.check(DR.family("dino_ce4", regime, dt, K), worst, record=GU.record_parity, case="mi355x")


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
@pytest.mark.parametrize("regime", list(DR.REGIMES))
@pytest.mark.parametrize("K", DR.KS)
def test_teacher_row_stats(ops, regime, K, dt):
    """row_max and row_max + row_lse (what the CE kernel consumes) against fp64, 1 and 11 rows, both temperatures"""
    DR.check(DR.family("teacher_row_stats", regime, dt, K), DR.eval_teacher_stats(ops, DEV, regime, K, dt), record=GU.record_parity, case="mi355x")


@pytest.mark.parametrize("R", DR.ROWSTAT_R)
def test_rowstat_combine(ops, R):
    """the fold of the last-layer GEMM's block statistics on synthetic blocks: fewer rows than a workgroup's four, fewer / exactly /
    more blocks than a wave's 64 lanes, blocks far below the row maximum, the maximum in the first, the last and the 65th block"""
    worst = {}
    for nb in DR.ROWSTAT_NB:
        for k, v in DR.eval_rowstat(ops, DEV, R, nb).items():
            worst[k] = max(worst.get(k, 0.0), v)
    DR.check("rowstat_combine/fp32", worst, record=GU.record_parity, case="mi355x_R%d" % R)


@pytest.mark.parametrize("layout", list(DR.REGION_LAYOUTS))
def test_region_match(ops, layout):
    """argmax + row assembly, bit for bit: every row written through cm_row (sentinel gone), the padding columns never win, the
    first maximal index wins a tie"""
    B, S, Tt, ld, crop_id, cm_row = DR.region_tables(layout)
    for kind in DR.REGION_KINDS:
        sim, _ = DR.region_sim(layout, kind)
        want = DR.region_match_ref(sim, Tt, crop_id, cm_row)
        tm = torch.full((B * S, 2), -7, dtype=torch.int32, device=DEV)
        got = ops.region_match(sim.to(DEV), Tt, crop_id.to(DEV), cm_row.to(DEV), tm).cpu()
        assert int((got == -7).sum()) == 0, (layout, kind)
        assert torch.equal(got, want), (layout, kind, int((got != want).sum()))


@pytest.mark.parametrize("rows,K,dt", DR.CENTER_SHAPES, ids=lambda v: DR.dt_name(v) if isinstance(v, torch.dtype) else str(v))
def test_center_chain(ops, rows, K, dt):
    """colsum -> center_ema against c m + mean(t) (1 - m) in fp64"""
    DR.check("center_chain/%s" % DR.dt_name(dt), DR.eval_center_chain(ops, DEV, rows, K, dt), record=GU.record_parity, case="mi355x_%dx%d" % (rows, K))


@pytest.mark.parametrize("prec,dt", [("fp32", torch.float32), ("bf16", torch.bfloat16)])
@pytest.mark.parametrize("K", [72, 1000])
@pytest.mark.parametrize("which", ["ddino", "dino"])
def test_loss_modules_in_the_trained_regime(ops, which, K, prec, dt):
    """esvit_amd.DDINOLoss / DINOLoss end to end (matching, statistics, CE, centre update) against the oracle in fp64 on the logits
    as stored: the loss, both gradients per row, both centres after the update"""
    import esvit_amd
    esvit_amd.set_precision(prec)
    try:
        DR.check(DR.family("module_" + which, "trained", dt, K), DR.eval_module(which, K, dt, DEV), record=GU.record_parity, case="mi355x")
    finally:
        esvit_amd.set_precision("bf16")


@pytest.mark.parametrize("dt", DR.DTYPES, ids=DR.dt_name)
def test_a_row_width_that_is_no_multiple_of_eight_is_refused(ops, dt):
    K = 1004
    s, t, c = (x.to(DEV) for x in DR.logits("trained", 4, 3, K, dt))
    with pytest.raises(RuntimeError, match="K=1004"):
        ops.teacher_row_stats(t, c, 25.0)
    mx, lse = torch.zeros(3, device=DEV), torch.zeros(3, device=DEV)
    tm, w = DR.two_term_tables(4, 3)
    ds_probe = []
    with pytest.raises(RuntimeError, match="K=1004"):
        ds_probe.append(ops.dino_ce(s, t, c, mx, lse, tm.to(DEV), w.to(DEV), 10.0, 25.0))
    assert not ds_probe
    torch.cuda.synchronize()  # nothing was launched: the stream is clean
