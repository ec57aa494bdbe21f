"""The fp64 statement of the fused MLP kernels (tests/mlp_fused_ref.py) and the cases of tests/test_mlp_fused_gpu.py, proved without a GPU:
the statement agrees with torch's fp64 autograd of the unfused formula, the GELU allowances in the docstring are what the transcribed forms
give, the case table reaches the instantiations, workgroup counts, live waves and tiles per workgroup it claims, the fp32 emulation stays
under every bound on every case (the largest ratio per output is printed) and, summed in two other orders, within 1.2 of itself, every
mutant of the emulation exceeds a criterion on each case named for it, and every case catches a mutant."""
import pytest
import torch
import torch.nn.functional as F

from tests import mlp_fused_ref as MR


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    return ops


def _close(a, b, ab):
    return bool(((a - b).abs() <= 1e-11 * ab + 1e-290).all())


def _ids(cases):
    return [c["name"] for c in cases]


# ---- the case table -------------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_what_it_claims(ops):
    G = ops.mlp_fused_dw_grid(torch.bfloat16, 96, 1 << 40)
    assert G == MR.DW_CUS  # (no device: the library answers with the size of an MI355X)
    assert [m for m in MR.dw_row_counts(G)] == [1, 63, 64, 65, 229, 64 * G + 1, 128 * G + 77]
    seen = {}
    for c in MR.CASES:
        inst, w, R, _ = MR.INSTANCES[(c["kind"], c["C"])]
        geo = MR.geometry(c, G)
        assert geo["inst"] == inst
        if c["kind"] == "dw":
            assert (geo["tiles"], geo["wgs"], geo["per_wg"]) == MR.dw_geometry_table(G)[c["M"]], c["name"]
            assert ops.mlp_fused_dw_grid(torch.bfloat16, 96, c["M"]) == geo["wgs"]
        else:
            assert c["M"] == MR.row_counts(w, R)[c["label"]]
            wgs, live = MR.LABEL_GEOMETRY[c["label"]]
            assert (geo["wgs"], geo["live"]) == (wgs, R // w if live is None else live), c["name"]
        seen.setdefault((c["kind"], c["C"], c["nn"]), set()).add((c["label"], c["family"]))
    # twelve instantiations behind three entry points, and the on-chip kernel
    assert len(seen) == 4 * 2 + 2 + 4 + 1
    for (kind, C, nn), got in seen.items():
        labels = [lab for lab, fam in got if fam == "dense"]
        assert len(labels) == (7 if kind == "dw" else 8)
        assert {fam for lab, fam in got} == {"dense", "tracer", "numerics"}
        assert ops.mlp_fused_supported(torch.bfloat16, C, backward=kind in ("bwd", "dw"))
    assert not ops.mlp_fused_supported(torch.bfloat16, 384, backward=True) and not ops.mlp_fused_supported(torch.bfloat16, 160)
    assert 4 * 384 // MR.HCH == 48 and MR.CHUNKS_384 == (0, 1, 22, 23, 46, 47)  # the peeled iterations of mlp32p_fwd_body and one steady pair


def test_tracer_shows_every_hidden_unit_and_channel():
    for C in (96, 128, 192, 256, 384):
        kind = "fwd"
        hidden, chans = set(), set()
        for k in range(4):
            inp = MR.inputs(MR.BY_NAME["%s_c%d_rbig_tracer_k%d" % (kind, C, k)])
            assert int((inp["W1"] != 0).sum(1).max()) == 1 and int((inp["W1"] != 0).sum(0).max()) == 4 and int((inp["W2"] != 0).sum(1).max()) == 1
            hidden |= set(torch.nonzero(inp["W2"])[:, 1].tolist())
            chans |= set(torch.nonzero(inp["W1"])[:, 1].tolist())
            assert inp["b1"].unique().numel() == 4 * C
        assert hidden == set(range(4 * C)) and chans == set(range(C))
    for q in MR.CHUNKS_384:
        live = set(torch.nonzero(MR.inputs(MR.BY_NAME["fwd_c384_rbig_tracer_q%d" % q])["W2"])[:, 1].tolist())
        assert live == set(range(32 * q, 32 * q + 32))


def test_row_scales_and_numerics_rows_are_where_the_table_says():
    for name in ("fwd_c96_rbig_dense", "bwd_c192_rbig_dense", "train_c384_rbig_dense"):
        c = MR.BY_NAME[name]
        inp, w = MR.inputs(c), MR.INSTANCES[(c["kind"], c["C"])][1]
        rs = inp["rs"]
        assert rs[0] == 0 and rs[-1] == 0 and rs[w - 1] == 0 and rs[w] == 0 and set(rs.tolist()) == set(torch.tensor(MR.ROWSCALES).tolist())
        ro = inp["rs_out"]
        assert ro[0] == 0 and ro[-1] == 0 and ro[w - 1] == 0 and ro[w] == 0 and not torch.equal(ro, rs)
        assert bool(((ro == 0) & (rs != 0)).any()) and bool(((ro != 0) & (rs == 0)).any())
    c = MR.BY_NAME["fwd_c384_rbig_numerics_e6"]
    inp = MR.inputs(c)
    x = inp["x"].double()
    ratio = x.mean(1).abs() / x.std(1, unbiased=False).clamp(min=1e-30)
    assert bool((ratio[0::6] > 90).all()) and bool((x[1::6].std(1) == 0).all()) and bool((ratio[5::6] > 90).all())
    A = MR._hidden(inp, c, MR.BF, "gelu43", x, MR.ln_stmt(x, inp["gamma"].double(), inp["beta"].double(), 1e-6, 10))["A"]
    assert float(A.min()) < -11 and float(A.max()) > 11
    for v in (4.5, -4.5, 0.0):
        assert bool((A == v).any())


def test_every_pre_activation_lies_inside_the_measured_range():
    for c in MR.CASES:
        if c["M"] > 400:  # (the two largest on-chip row counts draw the same distributions)
            continue
        inp = MR.inputs(c)
        x = inp["x"].double()
        ln = MR.ln_stmt(x, inp["gamma"].double(), inp["beta"].double(), MR._f32(c["eps"]), MR.ln_depth(c["kind"], c["C"]))
        hd = MR._hidden(inp, c, MR.BF, "gelu_f", x, ln)
        assert float((hd["A"].abs() + hd["e_A"]).max()) <= MR.A_RANGE, c["name"]


def test_gelu_allowances_are_the_measured_ones():
    dev = MR.gelu_deviation()
    print("GELU deviation", dev)
    for form, (v, d) in MR.GELU_DOC.items():
        assert abs(dev[form][0] / v - 1) < 0.05 and (d is None or abs(dev[form][1] / d - 1) < 0.05), (form, dev[form])
        assert 2 * dev[form][0] < MR.BF * 0.1  # small next to b
    x = torch.tensor([4.5, -4.5, 5.0, -5.0, 12.0, 0.0, -0.0])
    assert torch.equal(MR.gelu43(x)[2] / 5.0, MR.gelu43(x)[0] / 4.5)  # the clamp: the CDF saturates
    assert float(MR.gelu43(x)[5]) == 0.0 and float(MR.gelu_f(x)[6]) == 0.0


# ---- the statement is right --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bwd_c96_rbig_dense", "bwd_c96_rbig_tracer_k2", "bwd_c96_rbig_numerics_e5"])
def test_statement_equals_autograd_of_the_unfused_formula(name):
    case = dict(MR.BY_NAME[name], kind="dw")  # (the inputs of the backward case, every output the on-chip kernel adds)
    inp = MR.inputs(case)
    C, M = case["C"], case["M"]
    W1b, W2b = MR._weights(inp)
    x = inp["x"].double().requires_grad_(True)
    prm = {k: inp[k].double().clone().requires_grad_(True) for k in ("gamma", "beta", "b1", "b2")}
    W1, W2 = W1b.clone().requires_grad_(True), W2b.clone().requires_grad_(True)
    rs, ro, gy = inp["rs"].double().view(M, 1), inp["rs_out"].double().view(M, 1), inp["gy"].double()
    h = F.layer_norm(x, (C,), prm["gamma"], prm["beta"], MR._f32(case["eps"]))
    a1 = h @ W1.t() + prm["b1"]
    a1.retain_grad()
    y = x + rs * (F.gelu(a1) @ W2.t() + prm["b2"])
    y.backward(gy)
    ref = MR.statement(case)
    fwd = MR.statement(dict(case, kind="fwd", nn=False))
    assert _close(fwd["y"], y.detach(), fwd["ab_y"])
    assert _close(ref["gx"], x.grad, ref["ab_gx"]) and _close(ref["gx_act"], ro * x.grad, ro * ref["ab_gx"])
    assert _close(ref["dW2"], W2.grad, ref["ab_dW2"] + 1e-3 * ref["ab_db2"].view(-1, 1)) and _close(ref["db2"], prm["b2"].grad, ref["ab_db2"]) and _close(ref["db1"], prm["b1"].grad, ref["ab_db1"] + 1e-4 * ref["ab_db2"].sum())
    bw = MR.statement(dict(case, kind="bwd"))
    assert _close(bw["da1"], a1.grad, (rs * gy).abs() @ W2b.abs() * 1.2) and _close(bw["a1g"], F.gelu(a1).detach(), torch.ones(1, dtype=torch.float64))
    fold = MR.fold_stmt(ref["G"], ref["db1"], W1b, inp["gamma"].double(), inp["beta"].double())
    slack = 1e-4 * ref["ab_db2"].sum()  # (autograd's GELU' is 1 + erf: absolute, not relative, accuracy in the lower tail)
    assert _close(fold["dW"], W1.grad, fold["ab_dW"] + ref["ab_G"] + slack) and _close(fold["dgamma"], prm["gamma"].grad, fold["ab_dgamma"] + ref["ab_G"].sum(0) + slack)
    assert _close(fold["dbeta"], prm["beta"].grad, fold["ab_dbeta"] + 1.0)


def test_next_norm_and_training_outputs_of_the_statement():
    case = MR.BY_NAME["fwd_c128_nn_rbig_dense"]
    inp, ref = MR.inputs(case), MR.statement(case)
    want = F.layer_norm(ref["y"], (128,), inp["gamma_n"].double(), inp["beta_n"].double(), MR._f32(case["eps"]))
    assert _close(ref["xw"], want, want.abs() + 1.0) and _close(ref["mean_n"], ref["y"].mean(1), ref["y"].abs().mean(1))
    case = MR.BY_NAME["train_c384_rbig_dense"]
    inp, ref = MR.inputs(case), MR.statement(case)
    x = inp["x"].double()
    want = F.layer_norm(x, (384,), inp["gamma"].double(), inp["beta"].double(), MR._f32(case["eps"]))
    assert _close(ref["h"], want, want.abs() + 1.0) and _close(ref["a1g"], F.gelu(ref["a1"]), torch.ones(1, dtype=torch.float64))
    assert _close(ref["rstd"], (x.var(1, unbiased=False) + MR._f32(case["eps"])) ** -0.5, ref["rstd"])


@pytest.mark.parametrize("J,C", MR.FOLD_SHAPES)
def test_ln_fold_finish_statement_and_emulation(J, C):
    inp = MR.fold_inputs(J, C)
    d = {k: v.double() for k, v in inp.items() if k != "prev"}
    for prev in (None, inp["prev"]):
        ref = MR.fold_stmt(d["G"], d["db"], d["W"], d["gamma"], d["beta"], prev=None if prev is None else tuple(p.double() for p in prev))
        got = MR.fold_emulate(inp["G"], inp["db"], inp["W"], inp["gamma"], inp["beta"], prev=prev)
        m = {"ratio_" + k: MR.ratio(got[k], ref[k], ref["bd_" + k]) for k in ("dW", "dgamma", "dbeta")}
        print("FOLD", J, C, prev is not None, m)
        assert all(v <= 1.0 for v in m.values()), m
        broken = dict(got, dgamma=got["dgamma"] - (0 if prev is None else prev[0].double()) + 1e-5 * ref["ab_dgamma"])
        assert MR.ratio(broken["dgamma"], ref["dgamma"], ref["bd_dgamma"]) > 1.0


def test_cast_weight_statement_is_the_documented_permutation():
    p = MR.perm32(64).tolist()
    assert p[:8] == [0, 1, 2, 3, 16, 17, 18, 19] and p[8:16] == [4, 5, 6, 7, 20, 21, 22, 23] and p[32:36] == [32, 33, 34, 35] and sorted(p) == list(range(64))
    src = MR.data(("cw",), (5, 64))
    assert torch.equal(MR.cast_weight_stmt(src, True, False), src.t().to(torch.bfloat16))
    assert torch.equal(MR.cast_weight_stmt(src, False, True)[:, 4], src[:, 16].to(torch.bfloat16))


# ---- refusals that need no device: the argument checks come before any device call -------------------------------------------------------
def test_argument_checks_refuse_before_any_device_call(ops):
    import ctypes as C
    from esvit_amd._lib import lib
    f, off = C.c_void_p(0x1000), C.c_void_p(0x1004)  # never dereferenced
    ARG, UNSUPPORTED = -1, -3

    def fwd(dtype=1, x=f, b1=f, M=17, Cc=96, nn=(None,) * 5):
        return lib.esvit_mlp_fused_fwd(dtype, x, f, f, 1e-6, f, b1, f, f, None, M, Cc, f, *nn, None)

    def train(dtype=1, x=f, b1=f, M=17, Cc=384):
        return lib.esvit_mlp_fused_fwd_train(dtype, x, f, f, 1e-6, f, b1, f, f, None, M, Cc, f, f, f, f, f, f, None)

    def bwd(dtype=1, x=f, b1=f, M=17, Cc=96, tail=(None,) * 5):
        return lib.esvit_mlp_fused_bwd(dtype, x, f, None, None, f, f, 1e-6, f, f, f, b1, M, Cc, f, f, f, f, f, None, *tail)
    for call, bad_c in ((fwd, (160,)), (train, (160, 96)), (bwd, (160, 384))):
        for Cc in bad_c:
            assert call(Cc=Cc) == ARG and lib.esvit_last_error()
        assert call(dtype=0) == ARG and call(M=0) == ARG and call(b1=None) == ARG and call(x=off) == ARG
    full = (f, f, f, f, f)
    for k in range(1, 5):
        assert fwd(nn=full[:k] + (None,) + full[k + 1:]) == ARG
    assert fwd(nn=(off,) + full[1:]) == ARG and fwd(Cc=384, nn=full) == ARG
    assert bwd(tail=(f, None, None, None, None)) == ARG and bwd(Cc=192, tail=full) == ARG
    first = -(-0x7ff00000 // (4 * 384 * 2))
    assert train(M=first) == UNSUPPORTED and not ops.mlp_fused_train_supported(torch.bfloat16, 384, first) and ops.mlp_fused_train_supported(torch.bfloat16, 384, first - 1)
    assert lib.esvit_cast_weight(f, f, 64, 48, 0, 1, None) == ARG and lib.esvit_cast_weight(f, f, 48, 64, 1, 1, None) == ARG and lib.esvit_cast_weight(None, f, 64, 64, 0, 0, None) == ARG
    assert lib.esvit_ln_fold_finish(f, f, f, f, f, 0, 96, f, f, 0, None) == ARG and lib.esvit_ln_fold_finish(None, f, f, f, f, 4, 96, f, f, 0, None) == ARG
    assert lib.esvit_mlp_fused_weight(0, f, f, 160, None) == ARG and lib.esvit_mlp_fused_weight(1, f, f, 384, None) == ARG and lib.esvit_mlp_fused_weight(7, f, f, 96, None) == ARG


# ---- the bounds are not too tight; the second criterion is a condition the emulation itself meets -------------------------------------
@pytest.mark.parametrize("case", MR.CASES, ids=_ids(MR.CASES))
def test_emulation_stays_under_every_bound_in_three_summation_orders(case):
    ref = MR.reference(case)
    MR.check("emulation", case, MR.metrics(case, MR.emulate(case), ref, factor=1.0, floor=False))  # (prints the largest ratio of every output)
    for order in ("matmul", "reversed"):  # against the emulation itself: no floor
        MR.check("emulation_" + order, case, MR.metrics(case, MR.emulate(case, order=order), ref, factor=1.2, floor=False))


# ---- the criteria are not too loose ----------------------------------------------------------------------------------------------------
def _caught(case, mutant):
    return MR.failures(MR.metrics(case, MR.emulate(case, mutant=mutant), MR.reference(case)))


@pytest.mark.parametrize("mutant", MR.MUTANTS)
def test_every_mutant_is_caught_by_its_named_cases(mutant):
    for name in MR.MUTANT_CASES[mutant]:
        bad = _caught(MR.BY_NAME[name], mutant)
        print("MUTANT", mutant, name, bad)
        assert bad, "mutant %s escapes %s" % (mutant, name)


@pytest.mark.parametrize("case", MR.CASES, ids=_ids(MR.CASES))
def test_every_case_catches_a_mutant(case):
    for mutant in MR.CATCH_ALL:
        bad = _caught(case, mutant)
        if bad:
            print("CASE", case["name"], "catches", mutant, bad)
            return
    raise AssertionError("%s catches none of %s" % (case["name"], MR.CATCH_ALL))


def test_mutant_table_is_complete():
    assert set(MR.MUTANT_CASES) == set(MR.MUTANTS) and len(MR.MUTANTS) == 17
    assert all(n in MR.BY_NAME for ns in MR.MUTANT_CASES.values() for n in ns)
