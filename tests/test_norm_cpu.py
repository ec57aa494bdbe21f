"""The fp64 statement of the normalisation kernels (tests/norm_ref.py) and the cases of tests/test_norm_gpu.py, proved without a GPU: every
hand-written backward agrees with torch's fp64 autograd of the forward, the merge gather with the slicing-and-cat form of the reference
model, the case table with the restated ln_cfg / ln_dispatch / row_iters_dispatch (and the library's own answer to the block-count
question), oracle/ops_ref.py and an fp32 emulation that reduces in the kernels' order stay under every bound of every case, with and
without the restatement's allowance (the largest ratio per output is printed), and every mutant of the emulation exceeds a bound on each case named for it."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref
from tests import norm_ref as NR

CPU = torch.device("cpu")
PARAMS = NR.params()
MAXR = {}  # entry -> output -> (largest ratio, case)


@pytest.fixture(autouse=True)
def _built(lib_built):
    ops_ref.set_act_dtype(torch.float32)
    yield
    ops_ref.set_act_dtype(torch.float32)


def _close(a, b, ab):
    return bool(((a - b).abs() <= 1e-12 * ab + 1e-290).all())


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def test_width_table_is_the_restated_ln_cfg_and_reaches_all_twelve_instantiations():
    from esvit_amd import ops
    seen = set()
    for C, inst, _ in NR.WIDTHS:
        assert NR.ln_dispatch(*NR.ln_cfg(C)) == inst, (C, NR.ln_cfg(C), inst)
        seen.add(inst)
        G, it, rpb = NR.ln_shape(C)
        assert rpb * G == 256 and G * it * 4 >= C
        for rows in (1, 2 * rpb + 1, 1024 * rpb, 1024 * rpb + 1, 40000):
            assert ops.query(ops.Q_LN_BWD_BLOCKS, rows, C) == NR.ln_bwd_blocks(rows, C), (rows, C)
    assert seen == set(NR.LN_INSTANCES) and len(seen) == 12
    for C in NR.REFUSED_LN:
        assert NR.ln_cfg(C) is None and ops.query(ops.Q_LN_BWD_BLOCKS, 5, C) == 0
    launched = {(c["C"], dt) for c, dt in PARAMS if c["kind"] in ("ln", "merge")}
    assert {NR.ln_shape(C)[:2] for C, dt in launched if dt == torch.float32} == set(NR.LN_INSTANCES)
    assert {NR.ln_shape(C)[:2] for C, dt in launched if dt == torch.bfloat16} == set(NR.LN_INSTANCES)
    for C, rows in NR.MULTI_PASS:  # 1024 blocks: some lane groups take two trips, the others one
        rpb = NR.ln_shape(C)[2]
        assert NR.ln_bwd_blocks(rows, C) == 1024 and 1024 * rpb < rows < 2 * 1024 * rpb
    assert sorted({NR.ln_shape(C)[0] for C, _ in NR.MULTI_PASS}) == [8, 16, 32, 64]
    # the partly filled widths: the last used iteration holds fewer than G vectors, or whole iterations idle
    part = {C: (C // 4) % NR.ln_shape(C)[0] for C, _, _ in NR.WIDTHS}
    assert part[4] == 1 and part[48] == 12 and part[160] == 40 and part[320] == 16 and part[576] == 16
    assert -(-(1280 // 4) // 64) == 5 and -(-(1792 // 4) // 64) == 7
    lds = lambda C: NR.ln_shape(C)[2] * 2 * (C // 4) * 16  # noqa: E731
    assert lds(1536) == 48 * 1024 and lds(1280) < 48 * 1024 < lds(1792) < lds(2048) <= 160 * 1024


def test_row_widths_reach_every_row_iters_value():
    assert [NR.row_iters(D) for D in NR.ROW_WIDTHS] == [1, 1, 2, 2, 4, 4, 8, 8]
    assert (260 // 4) % 64 == 1 and (1028 // 4) % 64 == 1  # one lane in the last iteration
    assert all(D % 4 or D > 2048 for D in NR.REFUSED_ROW)


def test_merge_geometries():
    assert [4 * c for _, _, _, c in NR.MERGES] == [384, 384, 512, 1024, 2048]
    assert any(H != W for _, H, W, _ in NR.MERGES)


# ---- the statement is right ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,rows,eps", [(4, 3, 1e-6), (96, 7, 1e-5), (320, 5, 1e-6), (1792, 3, 1e-5)])
def test_layernorm_statement_equals_autograd(C, rows, eps):
    x = NR.data(("ag", C, "x"), (rows, C)).double().requires_grad_(True)
    gamma = (1 + NR.data(("ag", C, "g"), (C,), scale=0.2)).double().requires_grad_(True)
    beta = NR.data(("ag", C, "b"), (C,), scale=0.1).double().requires_grad_(True)
    dy, g_in = NR.data(("ag", C, "dy"), (rows, C)).double(), NR.data(("ag", C, "gin"), (rows, C)).double()
    y = F.layer_norm(x, (C,), gamma, beta, eps)
    (y * dy).sum().backward()
    fw = NR.ln_forward(x.detach(), gamma.detach(), beta.detach(), eps, C, torch.float32)
    assert _close(fw["y"], y.detach(), fw["ab_y"])
    bw = NR.ln_backward(x.detach(), dy, fw["mean"], fw["rstd"], gamma.detach(), C, g_in=g_in)
    assert _close(bw["dx"], x.grad + g_in, bw["ab_dx"]) and _close(bw["dgamma"], gamma.grad, bw["ab_dgamma"]) and _close(bw["dbeta"], beta.grad, bw["ab_dbeta"])


@pytest.mark.parametrize("nB,H,W,Cin", NR.MERGES)
def test_merge_gather_is_the_slicing_and_cat_form(nB, H, W, Cin):
    """swin_transformer.py PatchMerging: x0 = x[:, 0::2, 0::2], x1 = x[:, 1::2, 0::2], x2 = x[:, 0::2, 1::2], x3 = x[:, 1::2, 1::2], cat"""
    x = NR.data(("mg", nB, H, W), (nB, H * W, Cin)).double().requires_grad_(True)
    xg = x.view(nB, H, W, Cin)
    cat = torch.cat([xg[:, 0::2, 0::2], xg[:, 1::2, 0::2], xg[:, 0::2, 1::2], xg[:, 1::2, 1::2]], -1).reshape(-1, 4 * Cin)
    src = NR.merge_rows(nB, H, W)
    assert torch.equal(x.detach().view(-1, Cin)[src].reshape(-1, 4 * Cin), cat.detach())
    assert sorted(src.reshape(-1).tolist()) == list(range(nB * H * W))  # the scatter writes every token row once
    # the scatter of the backward is the adjoint of the gather
    w = NR.data(("mg", "w"), tuple(cat.shape)).double()
    (cat * w).sum().backward()
    dx = torch.zeros(nB * H * W, Cin, dtype=torch.float64)
    dx[src.reshape(-1)] = w.reshape(-1, Cin)
    assert torch.equal(dx, x.grad.view(-1, Cin))


@pytest.mark.parametrize("D", [4, 260, 2048])
def test_l2_and_weight_norm_statements_equal_autograd(D):
    x = NR.data(("ag2", D, "x"), (5, D)).double().requires_grad_(True)
    dz = NR.data(("ag2", D, "dz"), (5, D)).double()
    z = F.normalize(x, dim=-1, p=2)
    (z * dz).sum().backward()
    fw = NR.l2_forward(x.detach(), D, torch.float32)
    bw = NR.l2_backward(dz, fw["z"], fw["inv"], D, torch.float32)
    assert _close(fw["z"], z.detach(), fw["ab_z"]) and _close(bw["dx"], x.grad, bw["ab_dx"])
    assert float(NR.l2_forward(torch.zeros(1, D, dtype=torch.float64), D, torch.float32)["inv"]) == 1.0 / 1e-12
    v = NR.data(("ag2", D, "v"), (5, D), scale=0.05).double().requires_grad_(True)
    gw = (1 + NR.data(("ag2", D, "g"), (5, 1), scale=0.1)).double().requires_grad_(True)
    w = torch._weight_norm(v, gw, 0)
    (w * dz).sum().backward()
    fw = NR.wn_forward(v.detach(), gw.detach(), D, torch.float32)
    bw = NR.wn_backward(dz, v.detach(), gw.detach(), fw["inv"], D)
    assert _close(fw["w"], w.detach(), fw["ab_w"]) and _close(bw["dv"], v.grad, bw["ab_dv"]) and _close(bw["dg"], gw.grad, bw["ab_dg"])


# ---- the bounds are not too tight --------------------------------------------------------------------------------------------------------
def _note(entry, case, m):
    for k, v in m.items():
        if k.startswith("ratio_"):
            best = MAXR.setdefault(entry, {})
            if v > best.get(k, (-1.0, ""))[0]:
                best[k] = (v, case["name"])


@pytest.mark.parametrize("case,dt", PARAMS, ids=NR.ids(PARAMS))
def test_restatement_and_emulation_stay_under_every_bound(case, dt):
    """oracle/ops_ref (fp32 arithmetic on the case's inputs) and the emulation in the kernels' order (storing in the case's dtype) under
    the final bounds, and under the derived bounds alone: the restatement's allowance is there for the device's rsqrtf and division,
    no case on the CPU needs it"""
    derived = NR.statement(case, dt)
    for entry, got in (("ops_ref_fp32", NR.run(ops_ref, CPU, case, dt, cast=torch.float32)), ("emulation", NR.run(NR.Emulation(), CPU, case, dt, repeat=True))):
        m = NR.metrics(case, dt, got)
        _note(entry, case, m)
        NR.check(entry, case, dt, m)
        m = NR.metrics(case, dt, got, ref=derived)
        _note(entry + "_derived_only", case, m)
        NR.check(entry + "_derived_only", case, dt, m)


def test_bounds_grow_with_mean_over_std_and_not_with_its_square():
    """bd_rstd / rstd at |mean| / std = 1e3 and 3e4: between u |mean| / std and 100 u |mean| / std, far below u (mean / std)^2"""
    for name, k in (("ln_num_mean1000_w96_e6", 1e3), ("ln_num_mean300_w1024_e5", 3e4)):
        ref = NR.statement(NR.BY_NAME[name], torch.float32)
        rel = float((ref["bd_rstd"] / ref["rstd"]).max())
        print(name, "bd_rstd / rstd = %.3g, u k = %.3g, u k^2 = %.3g" % (rel, NR.U * k, NR.U * k * k))
        assert NR.U * k < rel < 100 * NR.U * k and rel < 0.1 * NR.U * k * k


def test_constant_row_bounds_are_derived_not_zero():
    for name in ("ln_num_const_w96_e6", "ln_num_const_w1024_e5"):
        case = NR.BY_NAME[name]
        ref, x = NR.statement(case, torch.float32), NR.inputs(case, torch.float32)
        eps = NR._f32(case["eps"])
        assert torch.equal(ref["y"], x["beta"].double().expand_as(ref["y"])) and bool(((ref["rstd"] - eps ** -0.5).abs() <= 1e-15 * eps ** -0.5).all())
        lead = NR.U * x["x"].double().abs()[:, :1] * eps ** -0.5 * x["gamma"].double().abs()  # u |mean| eps^-1/2 |gamma|
        assert bool((ref["bd_y"] > lead).all()) and bool((ref["bd_y"] < 40 * lead + 2 * NR.U).all())


# ---- the bounds are not too loose ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", NR.MUTANTS)
def test_every_mutant_is_caught_by_its_named_cases(mutant):
    caught = []
    for name in NR.MUTANT_CASES[mutant]:
        case = NR.BY_NAME[name]
        for dt in NR.MUTANT_DTS.get(mutant, case["dts"]):
            m = NR.metrics(case, dt, NR.run(NR.Emulation(mutant), CPU, case, dt))
            bad = NR.failures(m)
            caught.append("%s-%s: %s" % (name, NR.dt_name(dt), ", ".join(bad)))
            assert bad, "mutant %s escapes %s in %s: %s" % (mutant, name, NR.dt_name(dt), m)
    print("MUTANT", mutant, "caught by", caught)


def test_mutant_table_is_complete():
    assert set(NR.MUTANT_CASES) == set(NR.MUTANTS) and len(NR.MUTANTS) == 13
    assert all(n in NR.BY_NAME for ns in NR.MUTANT_CASES.values() for n in ns)


def test_zz_largest_ratio_per_output():
    """(runs last in the file) the largest err / bound of the restatement and of the emulation over the whole table"""
    for entry, best in sorted(MAXR.items()):
        print("MAX RATIO", entry, {k: "%.4g (%s)" % v for k, v in sorted(best.items())})
        assert all(v[0] <= 1.0 for v in best.values())
