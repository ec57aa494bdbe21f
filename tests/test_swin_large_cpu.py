"""Swin-L without a GPU: the named config is the yaml's SPEC and from_yaml builds the same model; the product's host code with
oracle/ops_ref.py in place of the kernels reproduces the step of the reference's own Swin-L (tests/golden/full_swin_large.pt,
tools/gen_swin_large_golden.py); the library answers the block-count question for the wide LayerNorm rows (2048 < C <= 8192,
C % 1024 == 0) as the restated rule does and still refuses 98, 2052, 2560 and 9216; the fp64 statements of tests/norm_ref.py hold at
the new widths against torch's fp64 autograd; an fp32 emulation in the wide kernels' reduction order stays under the derived bounds of
every case of tests/test_norm_wide_gpu.py, and each of its mutants is caught by the cases named for it (tests/norm_wide_ref.py)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref
from tests import norm_ref as NR
from tests import norm_wide_ref as NW
from tests import swin_large_ref as SL

CPU = torch.device("cpu")
PARAMS = NW.params()

# the MODEL section of experiments/imagenet/swin/swin_large_patch4_window7_224.yaml as the file states it
YAML_MODEL = """
MODEL:
  NAME: swin_transformer
  SPEC:
    PATCH_SIZE: 4
    DIM_EMBED: 192
    DEPTHS: [ 2, 2, 18, 2 ]
    NUM_HEADS: [ 6, 12, 24, 48 ]
    WINDOW_SIZE: 7
    MLP_RATIO: 4
    QKV_BIAS: True
    DROP_RATE: 0
    ATTN_DROP_RATE: 0
    DROP_PATH_RATE: 0.2
    USE_APE: False
    PATCH_NORM: True
TRAIN:
  IMAGE_SIZE: [ 224, 224 ]
"""


@pytest.fixture()
def cpu_ops(monkeypatch, lib_built):
    import esvit_amd.functional as Fn
    import esvit_amd.loss as L
    import esvit_amd.params as P
    for mod in (Fn, L, P):
        monkeypatch.setattr(mod, "ops", ops_ref)
    ops_ref.set_act_dtype(torch.float32)
    P.clear()
    Fn._GEOM.clear()
    yield ops_ref
    ops_ref.set_act_dtype(torch.float32)
    P.clear()
    Fn._GEOM.clear()


# ---- the config ------------------------------------------------------------------------------------------------------------------------
def test_swin_large_config_is_the_yaml_spec(tmp_path, lib_built):
    from esvit_amd import config as CFG
    from esvit_amd import models
    cfg = CFG.model_config("swin_large_w7")
    assert dict(cfg.MODEL.SPEC) == SL.SPEC and cfg.MODEL.NAME == "swin_transformer"
    assert dict(CFG.SWIN_SPECS["swin_large_w7"]) == SL.SPEC
    path = tmp_path / "swin_large_patch4_window7_224.yaml"
    path.write_text(YAML_MODEL)
    ycfg = CFG.from_yaml(str(path))
    assert dict(ycfg.MODEL.SPEC) == SL.SPEC and ycfg.MODEL.NAME == cfg.MODEL.NAME and list(ycfg.TRAIN.IMAGE_SIZE) == list(cfg.TRAIN.IMAGE_SIZE)
    a, b = (models.build_model(c, is_teacher=False, use_dense_prediction=True) for c in (cfg, ycfg))
    layout = lambda m: [(k, tuple(v.shape)) for k, v in m.state_dict().items()]  # noqa: E731
    assert layout(a) == layout(b) and a.num_features == 1536
    norms = {tuple(v.shape)[0] for k, v in a.state_dict().items() if ".norm" in k and k.endswith("weight")} | {a.num_features}
    assert norms == set(SL.LN_WIDTHS)  # 3072: the PatchMerging in front of the last stage


def test_swin_large_composition_matches_reference_golden(cpu_ops):
    """the host code over the fp32 restatement of the kernels vs the reference's own Swin-L: module tree / state_dict layout, loss to
    1e-6, outputs, centres, every gradient norm and the sampled gradients under the bounds of the full-width composition test
    (tests/test_composition_cpu.py)"""
    g = SL.gold()
    student, loss_fn, s_out, t_out, loss = SL.run_case(SL.CASE, CPU)
    SL.check_layout(g, student, s_out)
    d = SL.deltas(g, student, s_out, loss_fn, loss)
    print("OBSERVED", d)
    assert d["abs_err"] < 1e-6, (loss.item(), g["loss"])
    assert d["outputs_rel"] < 1e-4, d
    assert d["worst_grad_norm_rel"] < 2e-3 and d["worst_sampled_grad_rel_l2"] < 5e-3, d
    assert d["center_abs"] < 1e-6, d


# ---- the host rules -----------------------------------------------------------------------------------------------------------------------
def test_block_count_query_answers_the_wide_rule(lib_built):
    from esvit_amd import ops
    for C in NW.WIDTHS:
        assert NW.nv(C) == C // 1024 and 3 <= NW.nv(C) <= 8
        for rows in (1, 5, 170, 1024, 1025, 1029, 40000):
            want = min(rows, 1024)
            assert NW.blocks(rows, C) == want
            assert ops.query(ops.Q_LN_BWD_BLOCKS, rows, C) == want, (rows, C)
    for C in NW.REFUSED:
        assert NW.nv(C) == 0 and NW.blocks(5, C) == 0
        assert ops.query(ops.Q_LN_BWD_BLOCKS, 5, C) == 0, C
    for C, _, _ in NR.WIDTHS:  # the twelve narrow instantiations keep their rule
        for rows in (1, 1029, 40000):
            assert NW.blocks(rows, C) == NR.ln_bwd_blocks(rows, C) == ops.query(ops.Q_LN_BWD_BLOCKS, rows, C)


def test_case_table_covers_what_it_claims():
    names = set(NW.BY_NAME)
    assert {"wln_w%d_r%d" % (C, r) for C in (3072, 5120, 8192) for r in (1, 5, 1029)} <= names
    for C in (3072, 5120, 8192):  # 1024 + 5 rows: the loop is taken twice by blocks 0 .. 4, once by the others
        assert NW.blocks(1029, C) == 1024 and -(-1029 // 1024) == 2
    ri, drows, t2w, period = NW._map_rows(NW.BY_NAME["wln_map_h6_s3"])
    assert drows == 2 * 49 and len(set(ri.tolist())) == 72 and period == 49  # 13 pad slots per sample
    assert [(c["nB"], c["H"], c["W"], c["Cin"], c["pad"]) for c in NW.CASES if c["kind"] == "merge"] == [(1, 2, 2, 768, False), (2, 4, 6, 768, False), (1, 3, 5, 768, True)]
    src = NW.merge_src(1, 3, 5, True)
    assert src.shape == (6, 4) and int((src < 0).sum()) == 24 - 15 and sorted(src[src >= 0].tolist()) == list(range(15))
    assert set(NW.MUTANT_CASES) == set(NW.MUTANTS) and all(n in names for ns in NW.MUTANT_CASES.values() for n in ns)
    with NW.wide_rules():  # the depths handed to norm_ref's formulas
        assert NR.ln_shape(3072) == (64, 7, 1) and NR.ln_shape(8192) == (64, 12, 1) and NR.ln_shape(768) == (64, 3, 4)
        assert NR.fold_depth(5, 3072) == 1 + 1 + 2 + 8 and NR.fold_depth(1029, 3072, True) == 2 + 8 + 2 + 32 + 1
    assert NR.ln_cfg(3072) is None and NR.ln_shape(768) == (64, 3, 4)  # (norm_ref itself is as it was)


# ---- the statement is right at the new widths ---------------------------------------------------------------------------------------------
def _close(a, b, ab):
    return bool(((a - b).abs() <= 1e-12 * ab + 1e-290).all())


@pytest.mark.parametrize("C,rows,eps", [(3072, 3, 1e-6), (5120, 2, 1e-5), (8192, 3, 1e-6)])
def test_layernorm_statement_equals_autograd_at_wide_rows(C, rows, eps):
    x = NR.data(("wag", C, "x"), (rows, C)).double().requires_grad_(True)
    gamma = (1 + NR.data(("wag", C, "g"), (C,), scale=0.2)).double().requires_grad_(True)
    beta = NR.data(("wag", C, "b"), (C,), scale=0.1).double().requires_grad_(True)
    dy, g_in = NR.data(("wag", C, "dy"), (rows, C)).double(), NR.data(("wag", C, "gin"), (rows, C)).double()
    y = F.layer_norm(x, (C,), gamma, beta, eps)
    (y * dy).sum().backward()
    with NW.wide_rules():
        fw = NR.ln_forward(x.detach(), gamma.detach(), beta.detach(), eps, C, torch.float32)
        bw = NR.ln_backward(x.detach(), dy, fw["mean"], fw["rstd"], gamma.detach(), C, g_in=g_in)
    assert _close(fw["y"], y.detach(), fw["ab_y"])
    assert _close(bw["dx"], x.grad + g_in, bw["ab_dx"]) and _close(bw["dgamma"], gamma.grad, bw["ab_dgamma"]) and _close(bw["dbeta"], beta.grad, bw["ab_dbeta"])


@pytest.mark.parametrize("name", [c["name"] for c in NW.CASES if c["kind"] == "merge"])
def test_merge_statement_equals_autograd_of_pad_slice_cat_norm(name):
    """swin_transformer.py PatchMerging: F.pad to even sides, x0 = x[:, 0::2, 0::2], x1 = x[:, 1::2, 0::2], x2 = x[:, 0::2, 1::2],
    x3 = x[:, 1::2, 1::2], cat, LayerNorm -- forward, dx on the true grid, dgamma, dbeta of the statement against fp64 autograd"""
    case = NW.BY_NAME[name]
    nB, H, W, Cin, C = case["nB"], case["H"], case["W"], case["Cin"], case["C"]
    inp = NW.inputs(case, torch.float32)
    x = inp["x"].double().requires_grad_(True)
    gamma, beta = inp["gamma"].double().requires_grad_(True), inp["beta"].double().requires_grad_(True)
    xg = x.view(nB, H, W, Cin)
    if case["pad"]:
        xg = F.pad(xg, (0, 0, 0, W % 2, 0, H % 2))
    cat = torch.cat([xg[:, 0::2, 0::2], xg[:, 1::2, 0::2], xg[:, 0::2, 1::2], xg[:, 1::2, 1::2]], -1).reshape(-1, C)
    assert torch.equal(cat.detach(), NW._gather(x.detach(), NW.merge_src(nB, H, W, case["pad"]), Cin))
    y = F.layer_norm(cat, (C,), gamma, beta, case["eps"])
    (y * inp["dy"].double()).sum().backward()
    ref = NW.statement(case, torch.float32)
    assert _close(ref["y"], y.detach(), ref["ab_y"])
    # the statement's backward takes mean / rstd rounded to fp32, as the kernel does: autograd agrees to that rounding, which moves
    # every xhat of a row by u |mean| rstd whatever its size -- so the scale is the output's largest term, not each element's own
    shift = 1.0 + float((inp["mean"].double().abs() * inp["rstd"].double()).max())
    for k, want in (("dx", x.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
        assert bool(((ref[k] - want).abs() <= 16 * NR.U * shift * ref["ab_" + k].max()).all()), k


# ---- the bounds are not too tight, and not too loose -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dt", PARAMS, ids=NW.ids(PARAMS))
def test_emulation_in_the_wide_kernels_order_stays_under_the_derived_bounds(case, dt):
    m = NW.metrics(case, dt, NW.run(NW.Emulation(), CPU, case, dt, repeat=True))
    NR.check("emulation_wide", case, dt, m)


@pytest.mark.parametrize("mutant", NW.MUTANTS)
def test_every_wide_mutant_is_caught_by_its_named_cases(mutant):
    caught = []
    for name in NW.MUTANT_CASES[mutant]:
        case = NW.BY_NAME[name]
        for dt in NW.DTYPES:
            bad = NR.failures(NW.metrics(case, dt, NW.run(NW.Emulation(mutant), CPU, case, dt)))
            caught.append("%s-%s: %s" % (name, NR.dt_name(dt), ", ".join(bad)))
            assert bad, "mutant %s escapes %s in %s" % (mutant, name, NR.dt_name(dt))
    print("MUTANT", mutant, "caught by", caught)
