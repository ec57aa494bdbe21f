"""-m gpu: the ragged multi-crop route of CvT on the HIP path.

(1) the grouped mode of esvit_pad_crop_tokens / esvit_dwconv3x3 / esvit_col_sums2 / esvit_col_affine2 (include/esvit_hip.h) against the G
    separate calls it replaces, bit for bit; (2) the route against the per-group schedule; (3) the reference's fixtures with the route
    on, under the bounds of the per-group tests; (4) three trainer steps with the route on against off."""
import os

import pytest
import torch

from tests import golden_utils as GU
from tests.test_composition_cpu import check_cvt_variant, check_nano_cvt, nano_cvt_pair, run_nano_cvt_step
from tests.test_oracle_cpu import GOLD
from tests.test_step_gpu import NANO_BF16, _setup, _teardown, _to

pytestmark = pytest.mark.gpu

# (observed deltas go through GU.record_parity; the lines of a run on the MI355X are kept in profiles/cvt_ragged_parity_observed.jsonl)

# (nB, H, W) and the padded grid: 14 and 7 are the windows' multiples (6 -> 7), 3 -> 4 exercises a third geometry
GROUPS = {1: [((2, 14, 14), (14, 14))], 2: [((2, 14, 14), (14, 14)), ((3, 6, 6), (7, 7))],
          3: [((2, 14, 14), (14, 14)), ((3, 6, 6), (7, 7)), ((1, 3, 3), (4, 4))]}
# esvit_col_sums2 launches min(rows, 512) blocks of 256 / (C / 4) position lanes: 9800 rows are more than one sweep of the 512 blocks at both
# widths (16 and 5 lanes) and take the 32-slice finish, 147 and 9 rows are less than one sweep and take the 8-slice finish; no row count is
# a multiple of the lanes
SUM_ROWS = {1: [9800], 2: [9800, 147], 3: [9800, 147, 9]}
CASES = [(torch.bfloat16, 64), (torch.bfloat16, 192), (torch.float32, 64)]
MOAT = 64  # elements of NaN before, between and after the outputs (a multiple of 16 bytes in both dtypes)


class Slab:
    """outputs as slices of ONE NaN-filled buffer with moats around them: anything written outside an output shows"""

    def __init__(self, shapes, dtype, dev):
        sizes = [int(torch.tensor(s).prod()) for s in shapes]
        self.buf = torch.full((MOAT + sum(n + MOAT for n in sizes),), float("nan"), dtype=dtype, device=dev)
        self.views, self.spans, at = [], [], MOAT
        for s, n in zip(shapes, sizes):
            self.views.append(self.buf[at:at + n].view(s))
            self.spans.append((at, at + n))
            at += n + MOAT

    def moats_intact(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for a, b in self.spans:
            keep[a:b] = False
        return bool(torch.isnan(self.buf[keep]).all()) and int(keep.sum()) == MOAT * (len(self.spans) + 1)


def _rand(shape, dtype, dev, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want) and not bool(torch.isnan(got.float()).any())


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("dtype,C", CASES)
def test_grouped_pad_crop_and_dwconv_equal_their_separate_calls(dtype, C, G, lib_built):
    """pad, crop, depthwise 3x3 and its flipped form: one launch over the groups == the plain call per group, torch.equal; the NaN moats
    around every output stay; a second launch gives the same bits"""
    from esvit_amd import ops
    dev = torch.device("cuda:0")
    grp = GROUPS[G]
    xs = [_rand((nB * H * W, C), dtype, dev, 10 + i) for i, ((nB, H, W), _) in enumerate(grp)]
    pad_geo = [(nB, H, W, Hp, Wp) for ((nB, H, W), (Hp, Wp)) in grp]
    want_pad = [ops.pad_crop_tokens(x, *g) for x, g in zip(xs, pad_geo)]
    slab = Slab([w.shape for w in want_pad], dtype, dev)
    for _ in range(2):
        got = ops.pad_crop_tokens_grouped(xs, pad_geo, outs=slab.views)
        assert all(_same(a, b) for a, b in zip(got, want_pad)) and slab.moats_intact()
    crop_geo = [(nB, Hp, Wp, H, W) for ((nB, H, W), (Hp, Wp)) in grp]
    want_crop = [ops.pad_crop_tokens(x, *g) for x, g in zip(want_pad, crop_geo)]
    slab = Slab([w.shape for w in want_crop], dtype, dev)
    for _ in range(2):
        got = ops.pad_crop_tokens_grouped(want_pad, crop_geo, outs=slab.views)
        assert all(_same(a, b) for a, b in zip(got, want_crop)) and all(torch.equal(a, x) for a, x in zip(got, xs)) and slab.moats_intact()
    w9 = _rand((C, 9), torch.float32, dev, 3)
    dw_geo = [(nB, Hp, Wp) for ((nB, _, _), (Hp, Wp)) in grp]
    for flip in (False, True):
        want = [ops.dwconv3x3(x, w9, *g, flip=flip) for x, g in zip(want_pad, dw_geo)]
        slab = Slab([w.shape for w in want], dtype, dev)
        for _ in range(2):
            got = ops.dwconv3x3_grouped(want_pad, w9, dw_geo, flip=flip, outs=slab.views)
            assert all(_same(a, b) for a, b in zip(got, want)) and slab.moats_intact(), flip
    if G == 1:  # ... and without `outs` the one-group launch is the plain call
        assert _same(ops.dwconv3x3_grouped(want_pad, w9, dw_geo)[0], ops.dwconv3x3(want_pad[0], w9, *dw_geo[0]))
        assert _same(ops.pad_crop_tokens_grouped(xs, pad_geo)[0], want_pad[0])


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("dtype,C", CASES)
def test_grouped_col_sums2_and_col_affine2_equal_their_separate_calls(dtype, C, G, lib_built, monkeypatch):
    """the BatchNorm kernels: per-group sums [G, 2, C] with the partition and reduction order of the plain call on each group (torch.equal
    on sums of 9800 rows), the affine forms the BatchNorm forward (act 0 without x2), its backward (act 0 with x2: three coefficient
    vectors) and the stem (act 3 / 4) use, every group with its own coefficients"""
    from esvit_amd import ops
    dev = torch.device("cuda:0")
    rows = SUM_ROWS[G]
    a = [_rand((r, C), dtype, dev, 20 + i) * 0.5 + 0.25 for i, r in enumerate(rows)]
    b = [_rand((r, C), dtype, dev, 30 + i) for i, r in enumerate(rows)]
    for second in (b, a):  # BatchNorm backward (a = dy, b = d) and the statistics (b = a)
        want = torch.stack([ops.col_sums2(x, y) for x, y in zip(a, second)], 0)
        # the scratch of the grouped call lies in a NaN-filled workspace: a partial row it does not write would poison the sums
        monkeypatch.setattr(ops, "_WS", {})
        ops.workspace(1, dev, slot=1).fill_(float("nan"))
        for _ in range(2):
            got = ops.col_sums2_grouped(a, second)
            assert _same(got, want)
    coef = [[_rand((C,), torch.float32, dev, 40 + 3 * i + j) for j in range(3)] for i in range(G)]
    for act, with_x2 in ((0, False), (0, True), (3, False), (4, True)):
        x2s = b if with_x2 else None
        a2s = [c[1] for c in coef] if (act == 0 and with_x2) else None
        want = [ops.col_affine2(a[i], coef[i][0], coef[i][2], None if x2s is None else x2s[i], None if a2s is None else a2s[i], act=act) for i in range(G)]
        slab = Slab([w.shape for w in want], dtype, dev)
        for _ in range(2):
            got = ops.col_affine2_grouped(a, [c[0] for c in coef], [c[2] for c in coef], x2s, a2s, act=act, outs=slab.views)
            assert all(_same(x, y) for x, y in zip(got, want)) and slab.moats_intact(), (act, with_x2)


def _ragged_pair(dev, ragged):
    student, teacher = nano_cvt_pair(dev)
    student.ragged_multi_crop = ragged
    return student, teacher


def test_ragged_equals_per_group_on_the_hip_path(lib_built):
    """nano CvT, fp32 mode: outputs, loss, every parameter gradient (2e-5 of the per-group side's maximum, 20 times that for the gradients: the
    bounds of test_ragged_multi_crop_equals_reference_schedule_gpu) and the BatchNorm buffers"""
    import esvit_amd.loss as L
    from esvit_amd import functional as Fn
    dev = _setup("fp32")
    tol = 2e-5
    try:
        res, multi = [], []
        orig = Fn.cvt_block_multi
        Fn.cvt_block_multi = lambda *a, **k: (multi.append(1), orig(*a, **k))[1]
        try:
            for ragged in (True, False):
                student, teacher = _ragged_pair(dev, ragged)
                s_out, _, loss = run_nano_cvt_step(student, teacher, L, dev=dev)
                res.append((s_out, loss, {n: p.grad.detach().clone() for n, p in student.named_parameters() if p.grad is not None},
                            {k: v.detach().clone() for k, v in student.state_dict().items() if "running_" in k or "num_batches" in k}, len(multi)))
        finally:
            Fn.cvt_block_multi = orig
        (sa, la, ga, ba, na), (sb, lb, gb, bb, nb) = res
        assert na == sum(GU.NANO_CVT["depths"]) and nb == na  # the ragged pass took the multi blocks, the per-group pass none
        assert list(sa[3]) == list(sb[3])
        for a, b in zip(sa[:3], sb[:3]):
            assert (a - b).abs().max().item() <= tol * (b.abs().max().item() + 1e-12)
        assert abs(la.item() - lb.item()) <= tol
        assert ga.keys() == gb.keys()
        for n in ga:
            assert (ga[n] - gb[n]).abs().max().item() <= 20 * tol * (gb[n].abs().max().item() + 1e-12), n
        for k in ba:
            if "num_batches" in k:
                assert torch.equal(ba[k], bb[k]), k
            else:
                assert (ba[k] - bb[k]).abs().max().item() <= tol * (bb[k].abs().max().item() + 1e-12), k
    finally:
        _teardown()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_nano_cvt_step_with_the_route_on_matches_reference_golden(prec, lib_built):
    """the reference's nano CvT step (tests/golden/nano_cvt_step.pt) with the route on, under exactly the bounds of
    test_nano_cvt_step_matches_reference_golden"""
    import esvit_amd.loss as L
    g = torch.load(os.path.join(GOLD, "nano_cvt_step.pt"), weights_only=False)
    dev = _setup(prec)
    try:
        student, teacher = _ragged_pair(dev, True)
        s_out, t_out, loss = run_nano_cvt_step(student, teacher, L, dev=dev)
        got = {n: p.grad for n, p in student.named_parameters() if p.grad is not None}
        GU.record_parity(test="nano_cvt_step_ragged", prec=prec, abs_err=abs(loss.item() - g["ddino_loss"]),
                         worst_grad_norm_rel=max(max(abs(got[n].norm().item() - ref) - 1e-6, 0.0) / (ref + 1e-12) for n, ref in g["grad_norms"].items()))
        if prec == "fp32":
            check_nano_cvt(g, student, s_out, t_out, loss, rt=5e-4, loss_tol=1e-4, grad_tol=3e-3, buf_tol=1e-4)
        else:
            assert abs(loss.item() - g["ddino_loss"]) < NANO_BF16["nano_cvt_step"][0], (loss.item(), g["ddino_loss"])
            assert sorted(got) == sorted(g["grad_norms"])
            for n, ref in g["grad_norms"].items():
                assert abs(got[n].norm().item() - ref) <= NANO_BF16["nano_cvt_step"][1] * ref + 1e-6, (n, got[n].norm().item(), ref)
    finally:
        _teardown()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(GU.NANO_CVT_VARIANTS))
def test_cvt_variants_with_the_route_on_match_reference_golden(name, prec, lib_built, monkeypatch):
    """REL_POS_EMBED / SHIFT / RES_STEM with the route on (the models read ESVIT_CVT_RAGGED when they are built), under the bounds of
    test_cvt_variants_step_matches_reference_golden"""
    import esvit_amd.loss as L
    monkeypatch.setenv("ESVIT_CVT_RAGGED", "1")
    dev = _setup(prec)
    try:
        if prec == "fp32":
            student = check_cvt_variant(name, L, dev=dev, rt=5e-4, loss_tol=1e-4, grad_tol=3e-3, buf_tol=1e-4)
        else:
            student = check_cvt_variant(name, L, dev=dev, rt=6e-2, loss_tol=3e-3, grad_tol=0.08, buf_tol=2e-2, probes=False)
        assert student.ragged_multi_crop
    finally:
        _teardown()


def test_nano_cvt_rpe_w14_with_the_route_on_matches_reference_golden(lib_built, monkeypatch):
    """14x14 windows at head_dim 64 with a table per attention behind the residual stem (tests/golden/nano_cvt_rpe_w14.pt; bf16, the only
    mode these kernels have at head_dim 64) with the route on: loss, outputs, gradient norms and BatchNorm buffers under the bounds of
    test_nano_cvt_rpe_w14_step_matches_reference_golden; the three table gradients as relative L2 error against the fixture, within 3 x
    the largest error the per-group schedule shows for them in the same session (the project's rule for bf16 bounds: 3 x observed)"""
    import esvit_amd.loss as L
    from tests.test_rpe_hd64_cpu import load_fixture, nano_pair, run_step
    g = load_fixture()
    dev = _setup("bf16")

    def rel_l2(got, ref):
        return ((got.double() - ref.double()).norm() / ref.double().norm()).item()
    try:
        errs = {}
        for arm in ("0", "1"):
            monkeypatch.setenv("ESVIT_CVT_RAGGED", arm)
            student, teacher = nano_pair(g["case"], dev)
            assert student.ragged_multi_crop == (arm == "1")
            s_out, t_out, loss = run_step(g["case"], student, teacher, L, dev=dev)
            got = dict(student.named_parameters())
            errs[arm] = {n: rel_l2(got[n].grad.float().cpu(), ref) for n, ref in g["table_grads"].items()}
            if arm == "1":
                GU.record_parity(test="nano_cvt_rpe_w14_ragged", prec="bf16", abs_err=abs(loss.item() - g["ddino_loss"]), table_rel_l2=errs["1"],
                                 table_rel_l2_per_group=errs["0"])
                check_nano_cvt(g, student, s_out, t_out, loss, rt=6e-2, loss_tol=3e-3, grad_tol=0.08, buf_tol=2e-2)
        bound = 3 * max(errs["0"].values())
        for n, e in errs["1"].items():
            assert e <= bound, (n, e, errs["0"])
    finally:
        _teardown()


def test_three_trainer_steps_with_the_route_on_against_off(lib_built):
    """EsvitTrainer, nano CvT, bf16, drop-path 0: three steps with the route on and off from the same start.  Losses finite and equal to
    the bounds of test_trainer_step_with_logit_statistics_from_the_gemm's three-step comparison (first loss: same parameters, summation order
    only; later ones 1e-3), parameters within the AdamW step bound (2 lr per element and step: 6 lr), the teacher's BatchNorm buffers equal"""
    import esvit_amd.loss as L
    from esvit_amd import params as P
    from esvit_amd.engine import EsvitTrainer
    dev = _setup("bf16")
    lr = 5e-4

    def run(ragged):
        P.clear()
        student, teacher = _ragged_pair(dev, ragged)
        loss_fn = L.DDINOLoss(GU.NANO_HEAD["out_dim"], 5, 0.04, 0.07, 5, 10).to(dev)
        tr = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=0)
        losses = [tr.step(_to(GU.make_crops(2, n_local=3, sizes=GU.NANO_CVT["sizes"], seed=70 + i), dev), lr, 0.04, 0.996, epoch=i).item() for i in range(3)]
        torch.cuda.synchronize()
        tr.reducer.close()
        return losses, {k: v.detach().float().clone() for k, v in student.state_dict().items()}, {k: v.detach().float().clone() for k, v in teacher.state_dict().items()}

    try:
        l_on, p_on, t_on = run(True)
        l_off, p_off, t_off = run(False)
        assert all(x == x and abs(x) != float("inf") for x in l_on + l_off), (l_on, l_off)
        assert max(abs(a - b) / abs(b) for a, b in zip(l_on, l_off)) < 1e-3, (l_on, l_off)
        worst = max((p_on[k] - p_off[k]).abs().max().item() for k in p_on if p_on[k].numel() and "running_" not in k and "num_batches" not in k)
        assert worst < 6 * lr, worst
        for k in t_on:  # the teacher runs one group either way: its buffers see the same inputs up to the EMA of the student's parameters
            if "running_" in k:
                assert torch.allclose(t_on[k], t_off[k], rtol=2e-2, atol=2e-2), k
            elif "num_batches" in k:
                assert torch.equal(t_on[k], t_off[k]), k
    finally:
        _teardown()
