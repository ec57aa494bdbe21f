"""What tests/test_gemm_gpu.py relies on, proved without a GPU: the fp64 statement of tests/gemm_ref.py against torch.matmul and the
oracle; the exactness of every generated case; that the table reaches every main loop, tile, fast-path condition (both ways), the
multi-item walk of the eight-phase loop and empty split-K slices; that the comparison catches every mutant of the statement; and the
argument checks of esvit_gemm (cross-compiled library, nothing launched)."""
import ctypes

import pytest
import torch

from oracle import ops_ref
from tests import gemm_ref as GR

BF16, F32 = GR.BF16, GR.F32
_PROBS = {}


def prob_of(case, dt):
    key = (case["name"], dt)
    if key not in _PROBS:
        prob = GR.build(case, dt)
        _PROBS[key] = (prob, GR.expected(prob))
    return _PROBS[key]


def all_cases():
    return [(c, dt) for c in GR.table() for dt in c["dts"]]


def small(case):
    return case["M"] * case["N"] * case["K"] * max(case.get("batch", 1), 1) <= 5e7


# ---- the statement against independent restatements ---------------------------------------------------------------------------------------
def _dense(prob, f, rows, cols, nb=1, stride=0, ld=None):
    buf, off = prob["bufs"][prob["desc"][f][0]], prob["desc"][f][1]
    return buf.as_strided((nb, rows, cols), (stride, ld, 1), off).double()


def _operands(prob):
    d = prob["desc"]
    M, N, K, nb = d["M"], d["N"], d["K"], d["batch"]
    a = _dense(prob, "A", K if d["a_kstrided"] else M, M if d["a_kstrided"] else K, nb, d["strideA"], d["lda"])
    b = _dense(prob, "B", K if d["b_kstrided"] else N, N if d["b_kstrided"] else K, nb, d["strideB"], d["ldb"])
    return (a.transpose(1, 2) if d["a_kstrided"] else a), (b if d["b_kstrided"] else b.transpose(1, 2))


def _vec(prob, f, n):
    return prob["bufs"][prob["desc"][f][0]][prob["desc"][f][1]: prob["desc"][f][1] + n].double()


def torch_restatement(prob):
    """torch.matmul in fp64 plus the obvious epilogue, on dense copies of the operands (no row map) -> {output: dense fp64 tensor}"""
    d = prob["desc"]
    M, N, nb = d["M"], d["N"], d["batch"]
    a, b = _operands(prob)
    v = d["alpha"] * torch.matmul(a, b)
    out = {}
    if "colsum" in d:
        out["colsum"] = d["alpha"] * a[0].sum(1)
    if "bias" in d:
        v = v + _vec(prob, "bias", N)
    if d["epilogue"] in (GR.EPI_GELU, GR.EPI_QGELU):
        if "aux" in d:
            out["aux"] = v[0]
        v = torch.nn.functional.gelu(v) if d["epilogue"] == GR.EPI_GELU else v * torch.sigmoid(1.702 * v)
    elif d["epilogue"] in (GR.EPI_GELU_BWD, GR.EPI_QGELU_BWD):
        x = _dense(prob, "aux", M, N, 1, 0, d["ldaux"]).requires_grad_(True)
        y = torch.nn.functional.gelu(x) if d["epilogue"] == GR.EPI_GELU_BWD else x * torch.sigmoid(1.702 * x)
        v = v * torch.autograd.grad(y.sum(), x)[0]
    if "rowscale" in d:
        rs = _vec(prob, "rowscale", -(-M // d["rows_per_sample"]))
        v = v * rs[torch.arange(M) // d["rows_per_sample"]].view(1, M, 1)
    cin = _dense(prob, "C", M, N, nb, d["strideC"], d["ldc"])
    if "residual" in d:
        v = v + (cin if d["residual"] == d["C"] else _dense(prob, "residual", M, N, 1, 0, d["ldr"]))
    if d.get("splitk", 0) > 1 and d.get("accumulate"):
        v = v + cin
    out["C"] = v
    return out


def _written_dense(prob, exp, name, rows, cols, nb=1, stride=0, ld=None):
    """the statement's values as a dense tensor (NaN where it writes nothing)"""
    _, idx, val, _, _ = exp[name]
    flat = torch.full((prob["bufs"][name].numel(),), float("nan"), dtype=torch.float64)
    flat[idx] = val
    return flat.as_strided((nb, rows, cols), (stride, ld, 1), prob["desc"][name][1])


def test_reference_equals_torch_matmul_and_the_obvious_epilogue():
    n = 0
    for case, dt in all_cases():
        if case.get("rowmap") or not small(case):
            continue
        prob, exp = prob_of(case, dt)
        d = prob["desc"]
        want = torch_restatement(prob)
        got = _written_dense(prob, exp, "C", d["M"], d["N"], d["batch"], d["strideC"], d["ldc"])
        if prob["act"]:
            assert torch.allclose(got, want["C"], rtol=1e-12, atol=1e-13), case["name"]
        else:
            assert torch.equal(got, want["C"]), case["name"]
        if "aux" in exp:
            assert torch.equal(_written_dense(prob, exp, "aux", d["M"], d["N"], 1, 0, d["ldaux"])[0], want["aux"]), case["name"]
        if "colsum" in exp:
            assert torch.equal(exp["colsum"][2], want["colsum"]), case["name"]
        n += 1
    assert n > 800


def test_reference_equals_the_oracle_wrappers():
    """oracle/ops_ref.linear_fwd / linear_dgrad / linear_wgrad / batched_nt on every case they can express (fp32 arithmetic: exact on
    these inputs before the activation function)"""
    seen = dict(fwd=0, dgrad=0, wgrad=0, bnt=0, rowmap=0)
    for case, dt in all_cases():
        if not small(case) or case.get("splitk", 0) > 1 or case.get("alpha", 1.0) != 1.0:
            continue
        prob, exp = prob_of(case, dt)
        d = prob["desc"]
        M, N, K, nb, lay = d["M"], d["N"], d["K"], d["batch"], case["lay"]
        opa, opb = _operands(prob)
        of32 = bool(d["out_f32"])
        tol = dict(rtol=1e-5, atol=1e-5) if prob["act"] else dict(rtol=0, atol=0)
        if nb > 1:
            if lay != "nt" or dt != F32:
                continue
            got = ops_ref.batched_nt(opa.float().contiguous(), opb.transpose(1, 2).float().contiguous(), N)
            want = _written_dense(prob, exp, "C", M, N, nb, d["strideC"], d["ldc"])
            assert torch.equal(got.double(), want), case["name"]
            seen["bnt"] += 1
        elif lay == "nt" and case.get("residual") != "C":
            x, w = opa[0].to(dt), opb[0].t().contiguous().to(dt)
            rmap = None
            out_rows = M
            if "rowmap" in d:
                rmap = prob["bufs"]["rowmap"][4: 4 + d["rowmap_period"]]
                out_rows = (M // d["rowmap_period"]) * d["rowmap_tokens"]
            gelu = d["epilogue"] in (GR.EPI_GELU, GR.EPI_QGELU)
            r = ops_ref.linear_fwd(
                x, w, _vec(prob, "bias", N).float() if "bias" in d else None, gelu=gelu, want_preact=gelu and "aux" in d,
                residual=_dense(prob, "residual", out_rows, N, 1, 0, d["ldr"])[0].float() if "residual" in d else None, rowmap=rmap,
                rowmap_tokens=d.get("rowmap_tokens", 0), out_rows=out_rows if rmap is not None else None,
                rowscale=_vec(prob, "rowscale", -(-out_rows // d["rows_per_sample"])).float() if "rowscale" in d else None,
                rows_per_sample=d.get("rows_per_sample", 0), out_f32=of32, quick=d["epilogue"] == GR.EPI_QGELU)
            y, pre = r if isinstance(r, tuple) else (r, None)
            want = _written_dense(prob, exp, "C", out_rows, N, 1, 0, d["ldc"])[0]
            w_ok = ~torch.isnan(want)
            wr = GR.round_to(torch.nan_to_num(want), F32 if of32 else dt).double()
            assert torch.allclose(y.double()[w_ok], wr[w_ok], **(tol if of32 or dt == F32 else dict(rtol=2.0 ** -7, atol=1e-5) if prob["act"] else tol)), case["name"]
            if pre is not None:
                assert torch.equal(pre.double(), GR.round_to(exp["aux"][2], dt).double().view(M, N)), case["name"]
            seen["rowmap" if rmap is not None else "fwd"] += 1
        elif lay == "dg" and "bias" not in d:
            bwd = d["epilogue"] in (GR.EPI_GELU_BWD, GR.EPI_QGELU_BWD)
            y = ops_ref.linear_dgrad(opa[0].to(dt), opb[0].contiguous().to(dt), gelu_preact=_dense(prob, "aux", M, N, 1, 0, d["ldaux"])[0].to(dt) if bwd else None,
                                     out_f32=True, quick=d["epilogue"] == GR.EPI_QGELU_BWD)
            want = _written_dense(prob, exp, "C", M, N, 1, 0, d["ldc"])[0]
            assert torch.allclose(y.double(), want, **tol), case["name"]
            seen["dgrad"] += 1
        elif lay == "wg" and case.get("residual") in (None, "C"):
            out = _dense(prob, "C", M, N, 1, 0, d["ldc"])[0].float().contiguous() if case.get("residual") == "C" else None
            r = ops_ref.linear_wgrad(opa[0].t().contiguous().to(dt), opb[0].contiguous().to(dt), out=out, accumulate=out is not None, want_bias="colsum" in d)
            dw, db = r if isinstance(r, tuple) else (r, None)
            assert torch.equal(dw.double(), _written_dense(prob, exp, "C", M, N, 1, 0, d["ldc"])[0]), case["name"]
            if db is not None:
                assert torch.equal(db.double(), exp["colsum"][2]), case["name"]
            seen["wgrad"] += 1
    assert min(seen.values()) > 0 and seen["fwd"] > 100 and seen["wgrad"] > 100 and seen["dgrad"] > 50, seen


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------
def test_every_case_is_exact_in_fp32():
    worst = 0.0
    for case, dt in all_cases():
        worst = max(worst, GR.check_exact(prob_of(case, dt)[0]))
    assert worst < 2 ** 24 / 16   # (four bits to spare)


def test_inputs_are_representable_in_their_storage_type():
    for case, dt in all_cases():
        prob, _ = prob_of(case, dt)
        for f in ("A", "B", "aux"):
            if f in prob["desc"] and f not in prob["outs"]:
                b = prob["bufs"][f]
                assert b.dtype == dt
        assert prob["bufs"]["C"].dtype == (F32 if case.get("out_f32") else dt)


def test_bf16_outputs_hold_unrepresentable_values_and_exact_ties():
    """longer reductions: most exact values lie between bf16 neighbours, and some exactly half way (257 -> 256: round to even)"""
    ties = long_cases = 0
    for case, dt in all_cases():
        prob, exp = prob_of(case, dt)
        if prob["outs"]["C"] != BF16 or prob["act"] or not small(case):
            continue
        val = exp["C"][2]
        r = val.float().bfloat16().double()
        unrep = r != val
        if case["K"] >= 128 and not case.get("rowscale"):   # (a rowscale of 0 stores a quarter of the rows as zeros)
            long_cases += 1
            # whole units in [256, 512): every odd one lies between neighbours; from 512 on three of four
            # (2.2 units per k: K = 128 straddles 256, K = 192 lies in [256, 512), K = 256 mostly beyond 512)
            floor = 0.6 if case["K"] >= 256 else 0.45 if case["K"] >= 192 else 0.3
            assert float(unrep.double().mean()) > floor, (case["name"], float(unrep.double().mean()))
        # a tie: the value is exactly half way between its two bf16 neighbours
        lo = (val.float().view(torch.int32) & -65536).view(torch.float32).double()
        hi = (((val.float().view(torch.int32) & -65536) + 65536)).view(torch.float32).double()
        tie = unrep & ((val - lo) == (hi - val))
        ties += int(tie.sum())
        if bool(tie.any()):   # and RNE resolves it to the even mantissa
            assert bool(((r[tie].float().bfloat16().view(torch.int16) & 1) == 0).all())
    assert long_cases > 100 and ties > 1000, (long_cases, ties)
    assert float(torch.tensor(257.0).bfloat16()) == 256.0 and float(GR.round_to(torch.tensor([257.0, 259.0], dtype=torch.float64), BF16)[1]) == 260.0


# ---- which loop runs: esvit_gemm_select on every case --------------------------------------------------------------------------------------
def _fake_desc(prob, **over):
    """the case's descriptor with plausible, never dereferenced addresses (16-byte aligned buffer bases)"""
    from esvit_amd import _lib
    d = _lib.GemmDesc()
    ad = GR.addresses(prob)
    for f, v in prob["desc"].items():
        setattr(d, f, ad[f] if isinstance(v, tuple) else v)
    for f, v in over.items():
        setattr(d, f, v)
    return d


def _select(d, dt):
    from esvit_amd import _lib
    tm, tn, slots = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    k = _lib.lib.esvit_gemm_select(_lib.BF16 if dt == BF16 else _lib.F32, ctypes.byref(d), ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(slots))
    return (k, tm.value, tn.value)


def test_every_case_resolves_to_the_loop_and_tile_the_table_claims(lib_built):
    seen = set()
    for case, dt in all_cases():
        prob, _ = prob_of(case, dt)
        got = _select(_fake_desc(prob), dt)
        assert got == GR.resolves_to(case, dt), (case["name"], dt, got)
        if case["kern"] != GR.AUTO and dt == BF16:
            assert got[0] == case["kern"]   # a forced loop is never replaced
        seen.add((got, case["lay"]) if got[0] in (GR.DMA8, GR.P8) else got)
    want = {(GR.REGSTAGE, 128, 64), (GR.REGSTAGE, 128, 96), (GR.REGSTAGE, 128, 128), (GR.DMA4, 128, 64), (GR.DMA4, 128, 96), (GR.DMA4, 128, 128),
            (GR.DMA4W, 128, 192), (GR.DMA4W, 128, 96), ((GR.DMA8, 256, 256), "nt"), ((GR.DMA8, 256, 256), "dg"),
            ((GR.P8, 256, 256), "nt"), ((GR.P8, 256, 256), "dg"), ((GR.P8, 256, 256), "wg")}
    assert want <= seen, want - seen


def test_refused_loops_are_refused_not_replaced(lib_built):
    from esvit_amd import _lib
    for r in GR.REFUSED:
        case = GR._case("refused", "x", r["lay"], r["M"], r["N"], r["K"], r["kern"], (r["dt"],), **({"rowmap": r["rowmap"]} if "rowmap" in r else {}))
        prob = GR.build(case, BF16)   # (the descriptor of the bf16 build carries the forced loop)
        d = _fake_desc(prob)
        if r.get("validate"):
            d.lda = d.ldb = 320   # (legal pitches: the refusal is about M)
            rc = _lib.lib.esvit_gemm(_lib.BF16, ctypes.byref(d), None)
            assert rc == -1 and "k-strided A" in _lib.lib.esvit_last_error().decode(), r["why"]
        else:
            assert _select(d, r["dt"])[0] == -1, r["why"]
    # the hook FORCE_GEMM_KERNEL falls back to AUTO without saying so; an explicit kernel= does not
    from esvit_amd import ops
    old = ops.FORCE_GEMM_KERNEL
    try:
        ops.FORCE_GEMM_KERNEL = GR.P8
        assert ops._gemm_desc(dict(M=296, N=328, K=200, lda=200, ldb=200, ldc=328)).kernel == GR.AUTO
        assert ops._gemm_desc(dict(M=296, N=328, K=200, lda=200, ldb=200, ldc=328, kernel=GR.P8)).kernel == GR.P8
    finally:
        ops.FORCE_GEMM_KERNEL = old


# ---- the fast-path predicates, transcribed -------------------------------------------------------------------------------------------------
def dma_fast(d, ad, z, interior):
    """gemm_epilogue_bf16 (gemm_kernels.h:589-635): the straight-line epilogue of the LDS-DMA kernels is taken when ..."""
    al16 = lambda f: ad[f] % 16 == 0
    if d.get("splitk", 0) > 1:   # :594
        return interior and d["N"] % 4 == 0 and al16("partial")
    fast = ("rowmap" not in d and interior and d["ldc"] % 8 == 0 and al16("C") and (d["strideC"] * z) % 8 == 0 and
            ("bias" not in d or al16("bias")))                                                            # :599-600
    if d["epilogue"] in (GR.EPI_GELU, GR.EPI_QGELU):                                                      # :602-604
        return fast and "residual" not in d and "rowscale" not in d and not d["out_f32"] and ("aux" not in d or (d["ldaux"] % 8 == 0 and al16("aux")))
    if d["epilogue"] in (GR.EPI_GELU_BWD, GR.EPI_QGELU_BWD):                                              # :605-607
        return fast and "residual" not in d and "rowscale" not in d and d["ldaux"] % 8 == 0 and al16("aux")
    if "residual" in d:                                                                                   # :608-610
        return fast and d["ldr"] % 4 == 0 and al16("residual")
    return fast and "rowscale" not in d                                                                   # :612


def p8_fast(d, ad, lay):
    """p8_epi_matches (gemm_p8.hip:255-271) over the epilogue kinds instantiated for the layout (esvit_gemm_p8_launch, :595-599)"""
    al16 = lambda f: ad[f] % 16 == 0
    if d.get("splitk", 0) > 1:
        return d["N"] % 4 == 0 and al16("partial")                                                       # :258
    if not (d["ldc"] % 8 == 0 and al16("C") and d["strideC"] % 8 == 0 and ("bias" not in d or al16("bias"))):   # :259
        return False
    gelu, gelu_bwd = d["epilogue"] in (GR.EPI_GELU, GR.EPI_QGELU), d["epilogue"] in (GR.EPI_GELU_BWD, GR.EPI_QGELU_BWD)
    res, rs, f32 = "residual" in d, "rowscale" in d, bool(d["out_f32"])
    kinds = dict(
        bf16=not gelu and not gelu_bwd and not res and not rs and not f32,                                # :263
        f32=not gelu and not gelu_bwd and not res and not rs and f32,                                     # :265
        gelu=gelu and not res and not rs and not f32 and ("aux" not in d or (d["ldaux"] % 8 == 0 and al16("aux"))),   # :266
        res=not gelu and not gelu_bwd and res and f32 and d["ldr"] % 4 == 0 and al16("residual"),         # :267
        gelu_bwd=gelu_bwd and "bias" not in d and not res and not rs and not f32 and d["ldaux"] % 8 == 0 and al16("aux"))   # :268
    have = dict(nt=("bf16", "gelu", "res", "f32"), dg=("bf16", "gelu_bwd", "f32"), wg=("f32", "res"))[lay]
    return any(kinds[k] for k in have)


def test_every_fast_path_condition_is_negated_once_and_satisfied_once():
    """on bf16 launches with whole interior tiles: each alignment term of the two predicates is the ONLY false one in some case (the
    general epilogue runs because of it) and all hold in another (the straight-line epilogue runs)"""
    alone, all_true = set(), set()
    fast_seen = {(k, f): 0 for k in ("dma", "p8") for f in (True, False)}
    for case, dt in all_cases():
        if dt != BF16 or not GR.has_interior_tile(case, dt):
            continue
        prob, _ = prob_of(case, dt)
        terms = GR.fast_terms(prob)
        false = [t for t, ok in terms.items() if not ok]
        fam = "p8" if GR.resolves_to(case, dt)[0] == GR.P8 else "dma"
        if len(false) == 1:
            alone.add((fam, false[0]))
        if not false:
            all_true.update((fam, t) for t in terms)
        d, ad = prob["desc"], GR.addresses(prob)
        z = 1 if d["batch"] > 1 else 0
        fast = p8_fast(d, ad, case["lay"]) if fam == "p8" else dma_fast(d, ad, z, True)
        fast_seen[(fam, fast)] += 1
        if false:
            assert not fast, (case["name"], false)
        if case.get("defeat") == GR.ALL_OFF and d.get("splitk", 0) <= 1:
            assert not fast and len(false) >= 2, case["name"]
    terms = ("c_ptr", "ldc", "bias_ptr", "aux_ptr", "ldaux", "res_ptr", "ldr", "stridec", "partial_ptr", "n4")
    for fam in ("dma", "p8"):
        for t in terms:
            assert (fam, t) in alone, (fam, t, "never the only false term")
            assert (fam, t) in all_true, (fam, t, "never satisfied with all others")
    assert min(fast_seen.values()) >= 20, fast_seen


def test_the_multi_item_and_empty_slice_cases_are_what_they_claim(lib_built):
    multi = [c for c in GR.table() if c["family"] == "multi"]
    assert len(multi) == 5
    for c in multi:
        assert c["kern"] == GR.P8 and GR.p8_items(c) > 256 and c["K"] % 64 == 0
    # no other forced eight-phase case walks a second item: this family is the only cover of stream_next_item across items
    assert max(GR.p8_items(c) for c in GR.table() if c["kern"] == GR.P8 and c["family"] != "multi") <= 256
    s66 = [c for c in multi if c.get("splitk")]
    assert len(s66) == 2
    for c in s66:
        nkt = c["K"] // 64
        per = -(-nkt // c["splitk"])
        assert (nkt, per) == (70, 2) and GR.empty_slices(c["K"], c["splitk"], 64) and c["splitk"] - -(-nkt // per) == 31
    empty = {}
    for c in GR.table():
        if c.get("splitk", 0) > 1:
            for dt in c["dts"]:
                bk = 64 if dt == BF16 else 32
                if GR.empty_slices(c["K"], c["splitk"], bk):
                    kern = GR.resolves_to(c, dt)[0]
                    empty[(kern, c["lay"])] = empty.get((kern, c["lay"]), 0) + 1
    for key in ((GR.REGSTAGE, "dg"), (GR.REGSTAGE, "wg"), (GR.DMA4, "dg"), (GR.DMA4, "wg"), (GR.DMA4, "nt"), (GR.DMA4W, "wg"), (GR.DMA4W, "dg"), (GR.DMA8, "dg"),
                (GR.P8, "dg"), (GR.P8, "wg"), (GR.P8, "nt")):
        assert empty.get(key, 0) > 0, key
    # what the wrapper produces in the product: 8256 rows, a 96 x 96 weight
    from esvit_amd import ops
    sk = ops._pick_splitk(8256, 96, 96, 1, 512)
    assert sk == 16 and GR.empty_slices(8256, sk, 64)


def test_the_window_row_map_is_the_one_the_library_builds(lib_built):
    from esvit_amd import ops
    rmap, tokens = GR.rowmap_of("win")
    assert tokens == 36 and rmap.numel() == 49 and int((rmap < 0).sum()) == 13
    assert torch.equal(rmap, torch.from_numpy(ops.window_maps(6, 6, 7, 3)[0]))
    hand, tokens = GR.rowmap_of("hand")
    assert sorted(set(range(tokens)) - set(hand.tolist())) == [1, 4, 5]


# ---- mutants --------------------------------------------------------------------------------------------------------------------------
def _sample(items, n=60):
    step = max(1, len(items) // n)
    return items[::step]


@pytest.mark.parametrize("mutant,applies", GR.MUTANTS, ids=[m for m, _ in GR.MUTANTS])
def test_the_comparison_catches_the_mutant(mutant, applies):
    """a kernel with this mistake fails the comparison the GPU test makes, on the table as it stands"""
    cases = [(c, dt) for c, dt in all_cases() if applies(c) and small(c)]
    if mutant == "trunc":
        cases = [(c, dt) for c, dt in cases if dt == BF16 and not c.get("out_f32") and c.get("epi", 0) == 0 and c["K"] >= 128]
    if mutant == "last_slice":
        cases = [(c, dt) for c, dt in cases if dt == BF16]   # (slices of 64-deep k-tiles)
    assert len(cases) >= 8, (mutant, len(cases))
    for case, dt in _sample(cases):
        prob, exp = prob_of(case, dt)
        assert not GR.verify(prob, GR.render(prob, None), exp), case["name"]
        assert GR.verify(prob, GR.render(prob, mutant), exp), (mutant, case["name"], GR.dt_name(dt))


def test_the_comparison_catches_a_store_outside_the_written_set():
    """one element past a ragged edge, in a pad column, a guard row, a row the row map does not target, or the workspace's guard"""
    case = next(c for c in GR.table() if c["family"] == "rowmap" and "hand-res-rs-f32-dense" in c["name"])
    prob, exp = prob_of(case, BF16)
    clean = GR.render(prob, None)
    assert not GR.verify(prob, clean, exp)
    d = prob["desc"]
    base, ld = d["C"][1], d["ldc"]
    for where in (base + d["N"], base - 1, base + 1 * ld, base + 4 * ld + 3, clean["C"].numel() - 1):   # token rows 1 and 4 are untargeted
        got = dict(clean, C=clean["C"].clone())
        got["C"][where] = 1.0
        assert GR.verify(prob, got, exp), where
    case = next(c for c in GR.table() if c["family"] == "splitk" and c.get("colsum"))
    prob, exp = prob_of(case, BF16)
    clean = GR.render(prob, None)
    for name in ("partial", "colsum_partial", "colsum"):
        for where in (0, clean[name].numel() - 1):
            got = dict(clean)
            got[name] = clean[name].clone()
            got[name][where] = 0.0
            assert GR.verify(prob, got, exp), (name, where)
    # an unwritten plane of the workspace (an empty slice skipped instead of zeroed) shows as NaN in the sum
    got = dict(clean, partial=prob["bufs"]["partial"].clone())
    assert GR.verify(prob, got, exp)


# ---- argument checks come before any device call ----------------------------------------------------------------------------------------
REJECTIONS = [
    ("null operand", dict(A=None)), ("bad shape", dict(M=0)), ("bad dtype", dict(dtype=7)), ("lda/ldb", dict(lda=60)),
    ("K=60 must be", dict(K=60)), ("(k-strided A)", dict(a_kstrided=1, b_kstrided=1, M=124)), ("(k-strided B)", dict(b_kstrided=1, N=124, ldc=124)),
    ("16-byte aligned", dict(A=0x10008)), ("not used on the path", dict(a_kstrided=1)),
    ("split-K needs", dict(splitk=2)), ("split-K needs", dict(splitk=2, partial=0x50000, batch=2)), ("split-K needs", dict(splitk=2, partial=0x50000, ldc=136)),
    ("no fused epilogue", dict(splitk=2, partial=0x50000, bias=0x60000)), ("no fused epilogue", dict(splitk=2, partial=0x50000, epilogue=1)),
    ("no fused epilogue", dict(splitk=2, partial=0x50000, rowscale=0x60000, rows_per_sample=8)),
    ("bad rowmap geometry", dict(rowmap=0x60000)), ("rowscale needs", dict(rowscale=0x60000)), ("GELU' needs aux", dict(epilogue=2)),
    ("bad epilogue", dict(epilogue=9)), ("needs colsum_partial", dict(splitk=2, partial=0x50000, colsum=0x60000)),
    ("colsum is not batched", dict(colsum=0x60000, batch=2)), ("weight-gradient layout only", dict(colsum=0x60000)),
    ("weight-gradient layout only", dict(colsum=0x60000, b_kstrided=1)), ("colstat comes with rowstat", dict(colstat=0x60000)),
    ("plain bf16 forward epilogue only", dict(rowstat=0x60000, bias=0x70000)), ("plain bf16 forward epilogue only", dict(rowstat=0x60000, alpha=2.0)),
    ("whole 128 x 128 tiles", dict(rowstat=0x60000, M=64)),
    ("colstat lives in", dict(rowstat=0x60000, colstat=0x70000, M=256, N=256, ldc=256, kernel=GR.P8)),
    ("row statistics exist in", dict(rowstat=0x60000, kernel=GR.DMA8)),
    ("bad kernel selector", dict(kernel=9)), ("eight-phase loop needs", dict(kernel=GR.P8, K=72, lda=72, ldb=72)),
    ("eight-phase loop needs", dict(kernel=GR.P8, rowmap=0x60000, rowmap_period=4, rowmap_tokens=4)),
    ("fp32 runs on the register-staged", dict(dtype=1, kernel=GR.DMA4)), ("fp32 parity mode", dict(kernel=GR.REGSTAGE)),
    ("8-wave tile does not exist", dict(kernel=GR.DMA8, a_kstrided=1, b_kstrided=1)),
]


@pytest.mark.parametrize("msg,over", REJECTIONS, ids=["%02d-%s" % (i, m.replace(" ", "_")) for i, (m, _) in enumerate(REJECTIONS)])
def test_argument_checks_come_before_any_device_call(lib_built, msg, over):
    """one case per ESVIT_CHECK_ARG of validate and check_selector (gemm.hip): fake addresses, ESVIT_ERR_ARG, nothing launched"""
    from esvit_amd import _lib
    over = dict(over)
    dtype = over.pop("dtype", None)
    dtype = _lib.BF16 if dtype is None else (_lib.F32 if dtype == 1 else dtype)
    d = _lib.GemmDesc(A=0x10000, B=0x20000, C=0x30000, M=128, N=128, K=64, lda=64, ldb=64, ldc=128, batch=1, alpha=1.0)
    for f, v in over.items():
        setattr(d, f, v)
    rc = _lib.lib.esvit_gemm(dtype, ctypes.byref(d), None)
    got = _lib.lib.esvit_last_error().decode()
    assert rc == -1 and msg in got, (rc, got)
