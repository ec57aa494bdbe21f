"""The fp64 statement of window attention (tests/window_attn_ref.py) and the cases of tests/test_window_attn_gpu.py, proved without a GPU:
the statement agrees with torch autograd of a dense softmax formulation over the reference-style window partition and mask
(oracle/ops_ref.window_maps / shift_mask), oracle/ops_ref.py passes every case under the bounds, an emulation of the bf16 rounding
points stays under half the bf16 bound, the range cases have the scores and the masked probabilities they claim, the walk figures are
the docstring's, and every mutant of the statement exceeds its bound on every case it changes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref
from tests import window_attn_ref as WR

CPU = torch.device("cpu")
PARAMS = WR.params()


@pytest.fixture(autouse=True)
def _built(lib_built):
    ops_ref.set_act_dtype(torch.float32)
    yield
    ops_ref.set_act_dtype(torch.float32)


# ---- maps, labels, index ---------------------------------------------------------------------------------------------------------------
GRIDS = [(12, 12, 7, 3), (14, 14, 7, 0), (24, 24, 14, 7), (6, 6, 6, 0), (12, 5, 7, 0), (12, 5, 7, 3), (5, 12, 7, 0), (5, 12, 7, 3), (24, 13, 14, 7)]


@pytest.mark.parametrize("H,W,ws,shift", GRIDS)
def test_maps_and_labels_equal_the_partition_of_the_reference_and_the_library(H, W, ws, shift):
    """square and rectangular grids (only squares had ever been passed): the statement's closed form == the roll / pad / partition
    restatement (ops_ref) == the library's host code (ops.window_maps, shift_region_ids, shift_mask)"""
    from esvit_amd import ops
    tok, reg = WR.window_geometry(H, W, ws, shift)
    N = ws * ws
    w2t_ref, t2w_ref = ops_ref.window_maps(H, W, ws, shift)
    w2t, t2w = ops.window_maps(H, W, ws, shift)
    assert np.array_equal(tok.reshape(-1).numpy(), w2t_ref) and np.array_equal(w2t, w2t_ref) and np.array_equal(t2w, t2w_ref)
    assert sorted(tok[tok >= 0].tolist()) == list(range(H * W))  # every token sits in exactly one slot
    if shift:
        assert np.array_equal(reg.reshape(-1).numpy(), ops_ref.shift_region_ids(H, W, ws, shift))
        assert np.array_equal(ops.shift_region_ids(H, W, ws, shift), reg.reshape(-1).numpy())
        mask = torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0).numpy().astype(np.float32)
        assert np.array_equal(mask, ops_ref.shift_mask(H, W, ws, shift)) and np.array_equal(mask, ops.shift_mask(H, W, ws, shift))
    else:
        assert reg is None
        with pytest.raises(RuntimeError, match="shifted windows only"):
            ops.shift_region_ids(H, W, ws, 0)
    assert tok.shape == (w2t.size // N, N)


@pytest.mark.parametrize("ws", [3, 6, 7, 14])
def test_relative_position_index(ws):
    from esvit_amd import ops
    assert np.array_equal(WR.rel_index(ws).numpy(), ops_ref.relative_position_index(ws))
    assert np.array_equal(WR.rel_index(ws).numpy(), ops.relative_position_index(ws))


# ---- the statement == torch autograd of the dense formulation ---------------------------------------------------------------------------
AUTOGRAD_CASES = [c for c in WR.CASES if c["name"] != "walk14_hd64"]


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=[c["name"] for c in AUTOGRAD_CASES])
def test_statement_equals_autograd_of_the_dense_formulation(case):
    g, x = WR.geometry(case), WR.inputs(case, torch.float32)
    ref = WR.reference(case, torch.float32)
    nB, nH, hd, N, nW, L = case["nB"], case["nH"], case["hd"], g["N"], g["nW"], g["L"]
    C = nH * hd
    if case["N"] is None:
        tok = torch.from_numpy(ops_ref.window_maps(case["H"], case["W"], case["ws"], case["shift"])[0]).long()
    else:
        tok = torch.arange(N)
    nb = min(nB, 4)  # the per-slot outputs of the first images; the sums over windows need them all
    for images in (range(nb), range(nB)):
        n = len(images)
        qkv = x["qkv"][:n * L].double().requires_grad_(True)
        qb, table = x["qb"].double().requires_grad_(True), x["table"].double().requires_grad_(True)
        rows = torch.arange(n).view(n, 1) * L + tok.clamp(min=0).view(1, -1)
        pad = (tok < 0).view(1, -1, 1)
        xw = torch.where(pad, qb.view(1, 1, -1), qkv[rows]).view(n, nW, N, 3, nH, hd).permute(3, 0, 1, 4, 2, 5)
        s = (xw[0] * x["scale"]) @ xw[1].transpose(-1, -2) + table[g["index"][:N, :N].reshape(-1)].view(N, N, nH).permute(2, 0, 1)
        if case["shift"]:
            s = s + torch.from_numpy(ops_ref.shift_mask(case["H"], case["W"], case["ws"], case["shift"])).double().view(1, nW, 1, N, N)
        p = F.softmax(s, -1)
        o = p @ xw[2]  # [n, nW, nH, N, hd]
        do = torch.where(pad, torch.zeros(1, dtype=torch.float64), x["dout"][:n * L].double()[rows]).view(n, nW, N, nH, hd).permute(0, 1, 3, 2, 4)
        (o * do).sum().backward()
        close = lambda a, b, ab: bool(((a - b).abs() <= 1e-12 * ab + 1e-290).all())  # noqa: E731
        if n == nB:
            assert close(ref["dtable"], table.grad, ref["ab_dtable"] + 1e-30)
            assert close(ref["dpad"], qb.grad[C:], ref["ab_dpad"] + 1e-30) and float(qb.grad[:C].abs().max()) <= 1e-12 * float(ref["ab_dq"].max())
            if n > nb:
                continue
        sl = slice(0, n * nW)
        live = (~pad).view(1, nW, 1, N, 1).double()
        assert close(ref["attn"][sl], p.detach().reshape(-1, nH, N, N), ref["attn"][sl])
        assert close(ref["out"][sl], (o.detach() * live).reshape(-1, nH, N, hd), ref["ab_out"][sl])
        assert close(ref["lse"][sl], torch.logsumexp(s.detach(), -1).reshape(-1, nH, N), ref["ab_lse"][sl] + 1)
        sub = dict(case, nB=n)
        d3 = WR.to_win(qkv.grad, sub, parts=3)
        for i, k in enumerate(("dq", "dk", "dv")):
            assert close(ref[k][sl], d3[i], ref["ab_" + k][sl] + 1e-30), k


# ---- oracle/ops_ref.py under the bounds; the bf16 rounding points under half of them -----------------------------------------------------------
@pytest.mark.parametrize("case,dt", PARAMS, ids=WR.ids(PARAMS))
def test_ops_ref_passes_and_the_bf16_emulation_stays_under_half(case, dt):
    """the fp32 restatement (fp32 arithmetic on the case's inputs) passes every bound; in bf16 mode the restatement with its rounding
    points -- scale q, P and dS as operands, the stored outputs, as the kernels have them -- stays under half the bound"""
    got = WR.run_attention(ops_ref, CPU, case, dt, cast=torch.float32)
    WR.check("ops_ref_fp32", case, dt, WR.metrics(case, dt, got))
    if dt == torch.bfloat16:
        got = WR.run_attention(ops_ref, CPU, case, dt)
        WR.check("bf16_emulation", case, dt, WR.metrics(case, dt, got), limit=0.5)


def test_ops_ref_takes_the_block_of_the_full_index_on_the_partial_grid():
    case = WR.BY_NAME["partial_grid"]
    g, ref = WR.geometry(case), WR.reference(case, torch.float32)
    N, nH = g["N"], case["nH"]
    slab = ops_ref.dense_to_frag(ref["dbias"].float()).unsqueeze(0)
    full = ops_ref.relpos_bias_bwd(slab, g["index"], N, g["trows"])
    block = ops_ref.relpos_bias_bwd(slab, g["index"][:N, :N].contiguous(), N, g["trows"])
    assert torch.equal(full, block)
    assert WR.ratio(full.double(), ref["dtable"], ref["bd_dtable"]) <= 1.0


# ---- the inputs are what they claim ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dt", [p for p in PARAMS if p[0]["name"].startswith("range")], ids=WR.ids([p for p in PARAMS if p[0]["name"].startswith("range")]))
def test_range_cases_have_large_scores_and_live_masked_keys(case, dt):
    g, x = WR.geometry(case), WR.inputs(case, dt)
    ref = WR.reference(case, dt)
    nB, nW, N, nH = case["nB"], g["nW"], g["N"], case["nH"]
    S = torch.log(ref["attn"]) + ref["lse"].unsqueeze(-1)  # the scores, mask included
    masked = ref["masked"].view(1, nW, 1, N, N).expand(nB, nW, nH, N, N).reshape(-1, nH, N, N)
    pm = torch.where(masked, ref["attn"], torch.zeros_like(ref["attn"]))
    print("range", case["name"], WR.dt_name(dt), "max score %.1f, max masked probability %.3g" % (float(S.max()), float(pm.max())))
    assert float(S.max()) > 89.0              # fp32 exp without the max subtraction overflows
    if case["name"] in WR.RANGE_QK:           # (the bias-dominated variants: the score range only)
        assert _masked_keys_above_the_bound(case, dt)   # -100 and -inf differ by more than the bound
    for k in WR.OUTPUTS:
        assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(ref["bd_" + k]).all()), k


WALK = dict(walk7=((64, 2, 36), (42, 3, 16)), walk7_hd64=((85, 2, 15), (85, 2, 15)), walk7_noshift=((64, 2, 36), (42, 3, 16)),
            walk_small_w6=((42, 3, 16), (42, 3, 16)), walk_small_w3=((42, 3, 16), (42, 3, 16)), walk14=((48, 1, 48), (21, 3, 6)),
            walk14_hd64=((48, 1, 48), (42, 2, 6)), range7_hd32=((12, 1, 12), (12, 1, 12)), range7_hd64=((12, 1, 12), (12, 1, 12)),
            range7_bias=((12, 1, 12), (12, 1, 12)), range14=((8, 1, 8), (8, 1, 8)), range14_bias=((8, 1, 8), (8, 1, 8)),
            partial_grid=((170, 2, 30), (170, 2, 30)))


def test_the_walk_figures_of_the_case_table():
    """(parts, iters, active pairs of the last round) of the docstring table, from the host formulas; the cases named walk* do walk"""
    assert set(WALK) == set(WR.BY_NAME)
    for c in WR.CASES:
        w = WR.walk(c)
        assert (w["fwd"], w["bwd"]) == WALK[c["name"]], (c["name"], w)
        if c["name"].startswith("walk") or c["name"] == "partial_grid":
            assert w["bwd"][1] > 1 and w["bwd"][2] < w["bwd"][0], c["name"]  # several rounds, and an inactive tail in the last
    g = WR.geometry(WR.BY_NAME["walk7"])
    assert bool((g["tok"] < 0).any()) and g["reg"] is not None
    g = WR.geometry(WR.BY_NAME["walk7_noshift"])
    assert not bool((g["tok"] < 0).any()) and g["reg"] is None
    for name, dead_tiles in (("walk_small_w6", 1), ("walk_small_w3", 3)):
        assert (64 - WR.geometry(WR.BY_NAME[name])["N"]) // 16 == dead_tiles


# ---- the cases discriminate: every mutant of the statement exceeds its bound wherever it changes anything --------------------------------
SUMS = ("dbias_last_round", "pad_query_dout", "dpad_part", "index_stride")  # mutants of the sums over windows: every image is needed


def _compared(case):
    return tuple(k for k in WR.OUTPUTS if k != "dbias" and (k != "lse" or WR.geometry(case)["N"] > 64))


def _changed(mut, ref, dt):
    """the elements a mutant changes in a way the case's dtype can hold: by more than half an ulp of the dtype (2^-25 | 2^-9 relative) and
    more than the floor under which fp32 flushes to zero; a smaller change does not exist on the device"""
    diff = torch.where(torch.isfinite(mut), (mut - ref).abs(), torch.full_like(ref, float("inf")))
    return diff > torch.clamp((WR.BF if dt == torch.bfloat16 else WR.U / 2) * ref.abs(), min=WR.FLOOR)


def _evaluate(case, dt, mutant, parts):
    """None: the mutant changes nothing on this case that fp32 can hold; else True / False for caught / survived"""
    g = WR.geometry(case)
    nB, nW = case["nB"], g["nW"]
    ref = WR.reference(case, dt)
    images = None if mutant in SUMS or nB <= 2 else (0, nB - 1)  # (the last image holds the windows of the last round)
    mut = WR.statement(case, dt, mutant, parts, want_bounds=False, images=images)
    wsel = slice(None) if images is None else torch.cat([torch.arange(b * nW, (b + 1) * nW) for b in images])
    applies, caught = False, False
    for k in _compared(case):
        if k in ("dtable", "dpad"):
            if images is not None:
                continue
            a, b, bd = mut[k], ref[k], ref["bd_" + k]
        else:
            a, b, bd = mut[k], ref[k][wsel], ref["bd_" + k][wsel]
        diff = torch.where(torch.isfinite(a), (a - b).abs(), torch.full_like(b, float("inf")))
        if bool(_changed(a, b, dt).any()):
            applies = True
            caught = caught or bool((diff > bd).any())
            print("mutant", mutant, case["name"], WR.dt_name(dt), parts, k, "max diff / bound %.3g" % float((diff / bd).max()))
    return caught if applies else None


def _masked_keys_above_the_bound(case, dt):
    """the input condition of the range cases: some masked key keeps a probability above its bound, so -100 and -inf differ"""
    g, ref = WR.geometry(case), WR.reference(case, dt)
    masked = ref["masked"].view(1, g["nW"], 1, g["N"], g["N"])
    sh = (case["nB"], g["nW"], case["nH"], g["N"], g["N"])
    return bool((masked & (ref["attn"].view(sh) > ref["bd_attn"].view(sh))).any())


def _precondition(case, dt, mutant):
    g = WR.geometry(case)
    if mutant == "mask_inf":
        return g["reg"] is not None and _masked_keys_above_the_bound(case, dt)
    pads, walks = bool((g["tok"] < 0).any()), WR.walk(case)["bwd"][1] > 1
    if mutant == "pad_keys_kept":
        # it adds (NK - N) exp(-row maximum) to the denominators: on the bias-dominated cases every row maximum is tens of units up and
        # the change (1e-6 of a probability) lies under the resolution of bf16 while fp32 holds it; the cases with unit-scale rows stand
        return case["tab"] <= 1.0
    return {"prev_mask": walks and g["reg"] is not None, "prev_map": walks and g["nW"] > 1,
            "pad_kv_zero": pads, "pad_q_unscaled": pads, "pad_query_dout": pads, "dpad_part": pads and walks, "dbias_last_round": walks,
            "index_stride": g["N"] < g["ws"] ** 2, "lse_no_max": g["N"] > 64}.get(mutant, True)


@pytest.mark.parametrize("mutant", WR.MUTANTS)
def test_mutants_are_caught(mutant):
    applied, survived = 0, []
    for case, dt in PARAMS:
        if not _precondition(case, dt, mutant):
            continue
        w = WR.walk(case)
        for parts in sorted({w["bwd"][0], w["fwd"][0]} if mutant.startswith("prev_") else {w["bwd"][0]}):
            caught = _evaluate(case, dt, mutant, parts)
            if caught is None:
                continue
            applied += 1
            if not caught:
                survived.append((case["name"], WR.dt_name(dt), parts))
    assert applied > 0, "mutant %s applies to no case of the table" % mutant
    assert not survived, "mutant %s stays within the bound on %s" % (mutant, survived)
