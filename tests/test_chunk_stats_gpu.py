"""-m gpu: the statistics mode of the sliding-chunk kernels (esvit_amd/csrc/chunk_attn.hip: chunk_stats_local, chunk_stats_global_part /
_combine, chunk_stats_rows; ws | ESVIT_ATTN_SLIDING_CHUNK | ESVIT_ATTN_CHUNK_STATS) behind ops.chunk_attn_stats and esvit_amd.analysis
on an MsViT, on the MI355X, against the fp64 statement of tests/chunk_stats_ref.py: EVERY element of the entropy and of the listed rows
under the bounds its docstring derives, over the case table of tests/chunk_attn_ref.py.  tests/test_chunk_stats_cpu.py proves the
statement, the bounds and the mutants they catch without a GPU.  Every err / bound ratio goes to golden_utils.record_parity; the device
run is committed as profiles/chunk_stats_parity_observed.jsonl, a record only."""
import math

import pytest
import torch

from tests import attn_stats_ref as AR
from tests import chunk_attn_ref as CR
from tests import chunk_stats_ref as R
from tests import golden_utils as GU

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
GUARD = 64  # rows around what the kernels read and behind what they write
CASE_IDS = [c["name"] for c in CR.CASES]


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _between_nan_rows(qkv):
    """the token rows between GUARD rows of NaN on either side (a read outside the rows poisons the result)"""
    buf = torch.full((qkv.shape[0] + 2 * GUARD, qkv.shape[1]), float("nan"), dtype=qkv.dtype, device=DEV)
    buf[GUARD:GUARD + qkv.shape[0]] = qkv.to(DEV)
    return buf[GUARD:GUARD + qkv.shape[0]]


def _run(ops, qkv, case, scale, qs):
    """one call into NaN-filled destinations with GUARD rows behind them -> (entropy buffer [B + 1...], rows buffer)"""
    B, nH, L = case["B"], case["nH"], case["L"]
    ent, rows = _nan(B + 1, nH, L), _nan(B + 1, nH, len(qs), L)
    e, r = ops.chunk_attn_stats(qkv, B, L, nH, scale, CR.layout(case, DEV), queries=qs, ent_out=ent[:B], rows_out=rows[:B])
    torch.cuda.synchronize()
    assert e.data_ptr() == ent.data_ptr() and r.data_ptr() == rows.data_ptr()
    return ent, rows


def _note(tag, m):
    GU.record_parity(test="chunk_stats", where="mi355x", **tag, **m)
    print("OBSERVED", tag, m)


def _check(tag, m, note=True):
    if note:
        _note(tag, m)
    bad = ["%s = %.4g" % (k, v) for k, v in m.items() if (k.startswith("equal") and v != 1.0) or (k.startswith("ratio") and not v <= 1.0)]
    assert not bad, (tag, bad)


@pytest.mark.parametrize("case", CR.CASES, ids=CASE_IDS)
def test_stats_under_the_bounds(ops, case):
    """entropy and listed rows (every global, the first and the last local token, a chunk-corner token, an interior one and its
    duplicate) per element; rows exactly 0 wherever the mask forbids (the planted 700 of the stress cases is such a key); NaN-filled
    destinations whose guard image stays NaN, inputs between NaN rows; two launches, equal bits; ops.chunk_attn_stats without
    destinations returns the same bits; without a list it returns no rows and the same entropies"""
    ref, _, qs = R.case_reference(case)
    x = CR.inputs(case, BF16)
    B, nH, hd, L, nglo = case["B"], case["nH"], case["hd"], case["L"], case["nglo"]
    assert ops.chunk_attn_stats_supported(BF16, hd, CR.W, nglo)
    qkv = _between_nan_rows(x["qkv"])
    e1, r1 = _run(ops, qkv, case, x["scale"], qs)
    e2, r2 = _run(ops, qkv, case, x["scale"], qs)
    e3, r3 = ops.chunk_attn_stats(qkv, B, L, nH, x["scale"], CR.layout(case, DEV), queries=torch.tensor(qs))
    e4, none = ops.chunk_attn_stats(qkv, B, L, nH, x["scale"], CR.layout(case, DEV))
    torch.cuda.synchronize()
    ent, rows = e1[:B].cpu().double(), r1[:B].cpu().double()
    forbidden = ~ref["mask"][qs]
    m = dict(ratio_ent=CR.ratio(ent, ref["ent"], ref["bd_ent"]), ratio_rows=CR.ratio(rows, ref["rows"], ref["bd_rows"]),
             ratio_ent_derived=CR.ratio(ent, ref["ent"], ref["bd_ent_derived"]), ratio_rows_derived=CR.ratio(rows, ref["rows"], ref["bd_rows_derived"]))
    for k in ("ratio_ent_derived", "ratio_rows_derived"):  # (for the record: the asserted bounds carry the device-function allowance)
        m["observed_" + k[6:]] = m.pop(k)
    m["equal_finite"] = float(bool(torch.isfinite(e1[:B]).all()) and bool(torch.isfinite(r1[:B]).all()))
    m["equal_masked_zero"] = float(bool((rows[..., forbidden] == 0).all()))
    m["equal_guard"] = float(_all_nan(e1[B:]) and _all_nan(r1[B:]))
    m["equal_repeat"] = float(torch.equal(_bits(e1[:B]), _bits(e2[:B])) and torch.equal(_bits(r1[:B]), _bits(r2[:B])))
    m["equal_plain_call"] = float(torch.equal(_bits(e3), _bits(e1[:B])) and torch.equal(_bits(r3), _bits(r1[:B])) and none is None
                                  and torch.equal(_bits(e4), _bits(e1[:B])))
    m["equal_duplicate"] = float(torch.equal(_bits(r1[:B, :, -1]), _bits(r1[:B, :, -2])))
    m["ratio_row_sum"] = float(((rows.sum(-1) - 1).abs() / (ref["bd_rows"].sum(-1))).max())
    _check(dict(entry="stats", case=case["name"]), m)


@pytest.mark.parametrize("case", CR.CASES, ids=CASE_IDS)
def test_zero_queries_give_the_log_of_the_visible_keys(ops, case):
    """q = 0: every score is 0, every row uniform over the keys it sees, H = ln(visible keys) to the bound of the statement on these
    inputs -- a dead neighbourhood slot or a padded column that enters the sum moves it by ln(448 / visible)"""
    x = CR.inputs(case, BF16)
    B, nH, hd, L, nglo, nx, ny = case["B"], case["nH"], case["hd"], case["L"], case["nglo"], case["nx"], case["ny"]
    qkv0 = x["qkv"].clone()
    qkv0[:, :nH * hd] = 0
    ref, _ = R.bounds(qkv0, B, nH, hd, nglo, nx, ny, x["scale"])
    visible = ref["mask"].sum(-1).double()
    assert (ref["ent"] - torch.log(visible)).abs().max().item() <= 1e-12
    ent, none = ops.chunk_attn_stats(_between_nan_rows(qkv0), B, L, nH, x["scale"], CR.layout(case, DEV))
    torch.cuda.synchronize()
    m = dict(ratio_ent=CR.ratio(ent.cpu().double(), torch.log(visible).expand(B, nH, L), ref["bd_ent"]), equal_no_rows=float(none is None),
             observed_bound_max=float(ref["bd_ent"].max()))
    assert (ref["bd_ent"] < torch.log((visible + 1) / visible)).all()  # (every bound is below what ONE entering slot would move the row by)
    _check(dict(entry="zero_q", case=case["name"]), m)


def _direct(ops, case, qkv, scale, qidx, ent, rows, nq=None, hd=None):
    nq = qidx.numel() if nq is None else nq
    tab, nglo, rowtok = CR.layout(case, DEV)
    ws = ops.workspace(ops.query(ops.Q_CHUNK_ATTN_WS, case["B"] * case["nH"], case["L"], 0), DEV, slot=3)
    rc = ops.lib.esvit_window_attn_fwd(ops.BF16, ops._p(qkv), None, ops._p(tab), case["L"], None, CR.W | ops.ATTN_SLIDING_CHUNK | ops.ATTN_CHUNK_STATS,
                                       ops._p(ws), None, case["nx"], case["B"], case["ny"] | (nq << 16), case["nH"], case["hd"] if hd is None else hd,
                                       float(scale), ops._p(qidx), ops._p(rows), ops._p(ent), ops._stream())
    torch.cuda.synchronize()
    return rc


def test_out_of_range_index_is_skipped_and_refused_calls_write_nothing(ops):
    """through the C entry (ops.chunk_attn_stats refuses such a list on the host): a listed index outside [0, L) leaves its row NaN, the
    rows beside it and the entropies are the bits of the call without it; a refused call leaves every destination NaN"""
    case = CR.BY_NAME["ragged"]
    ref, _, qs = R.case_reference(case)
    x = CR.inputs(case, BF16)
    B, nH, L = case["B"], case["nH"], case["L"]
    qkv = _between_nan_rows(x["qkv"])
    good, _ = _run(ops, qkv, case, x["scale"], qs)
    want_rows = _run(ops, qkv, case, x["scale"], qs)[1]
    lst = [qs[0], L, qs[1], -1, 2 ** 31 - 1, qs[2]]
    qidx = torch.tensor(lst, dtype=torch.int32, device=DEV)
    ent, rows = _nan(B + 1, nH, L), _nan(B + 1, nH, len(lst), L)
    with pytest.raises(ValueError, match=r"\[0, 121\)"):
        ops.chunk_attn_stats(qkv, B, L, nH, x["scale"], CR.layout(case, DEV), queries=lst)
    assert _direct(ops, case, qkv, x["scale"], qidx, ent, rows) == 0
    assert torch.equal(_bits(ent[:B]), _bits(good[:B])) and _all_nan(ent[B:]) and _all_nan(rows[B:])
    for j, src in ((0, 0), (2, 1), (5, 2)):
        assert torch.equal(_bits(rows[:B, :, j]), _bits(want_rows[:B, :, src]))
    for j in (1, 3, 4):
        assert _all_nan(rows[:B, :, j])
    # refused calls: ESVIT_ERR_ARG, nothing written
    ent, rows = _nan(B + 1, nH, L), _nan(B + 1, nH, len(lst), L)
    assert _direct(ops, case, qkv, x["scale"], qidx, ent, rows, hd=40) == -1 and b"head_dim 40" in ops.lib.esvit_last_error()
    assert _direct(ops, case, qkv, x["scale"], qidx, ent, None) == -1 and b"without the rows output" in ops.lib.esvit_last_error()
    assert _direct(ops, case, qkv, x["scale"], None, ent, rows, nq=3) == -1 and b"without the list" in ops.lib.esvit_last_error()
    assert _direct(ops, case, qkv, x["scale"], qidx, ent, rows, nq=0) == -1 and b"must be NULL" in ops.lib.esvit_last_error()
    assert _all_nan(ent) and _all_nan(rows)


def test_memory_stays_below_one_head_of_scores(ops):
    """vil_small's stage-1 shape at 448^2 (L = 12545, 3 heads of 32), B = 2: the peak allocation of ops.chunk_attn_stats above its live
    inputs stays below the bytes of ONE head's fp32 L x L matrix (629 MB; the dense route holds B nH of them in bf16 and its fp32 P on
    top).  A condition, not a measurement: the mode's own outputs are (1 + nq) L floats per (image, head)"""
    B, nH, hd, nglo, nx, ny = 2, 3, 32, 1, 112, 112
    L = nglo + nx * ny
    case = dict(nx=nx, ny=ny, nglo=nglo)
    qkv = (torch.randn(B * L, 3 * nH * hd, generator=torch.Generator().manual_seed(3))).to(BF16).to(DEV)
    lay = (CR.table(case).to(DEV), nglo, CR.W * ny)
    qs = R.default_queries(nglo, nx, ny)
    ops.chunk_attn_stats(qkv[:B * 50], B, 50, nH, hd ** -0.5, (CR.table(dict(nx=7, ny=7, nglo=1)).to(DEV), 1, 49), queries=[0])  # (the shared scratch exists)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ent, rows = ops.chunk_attn_stats(qkv, B, L, nH, hd ** -0.5, lay, queries=qs)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    one_head = 4 * L * L
    outputs = 4 * B * nH * (1 + len(qs)) * L
    GU.record_parity(test="chunk_stats", where="mi355x", entry="memory", shape=[B, L, nH, hd], peak_above_inputs_MB=peak / 1e6, one_head_MB=one_head / 1e6,
                     outputs_MB=outputs / 1e6)
    assert ent.shape == (B, nH, L) and rows.shape == (B, nH, len(qs), L) and torch.isfinite(ent).all() and torch.isfinite(rows).all()
    assert ((rows.sum(-1) - 1).abs() <= 1e-3).all() and (ent > 0).all() and (ent[:, :, nglo:] <= math.log(442.0) + 1e-3).all()
    assert peak < one_head, (peak, one_head)


# ---- model level: a nano MsViT in bf16 mode ----------------------------------------------------------------------------------------
def _dense_allowance(qkv, B, nH, hd, nglo, nx, ny, qs):
    """what the dense route (scores and P rounded to bf16 by the batched GEMMs and the row softmax) may differ from fp64 by, as
    tests/test_attn_stats_gpu.py takes it: its score error is dg = 2^-9 max_k |s_k| per row over the keys the row sees (the exact
    form e^(2 dg) - 1 is kept), rows off by (e^(2 dg) - 1 + 2^-9) p + 2^-23, the entropy by 2 dg max(1, ln n) + 2^-9 (ln n + 1), n the
    keys the row sees"""
    L = nglo + nx * ny
    q, k = R.heads64(qkv, B, nH, hd, L)
    mask = R.mask_of(nglo, nx, ny)
    smax = torch.where(mask, (hd ** -0.5 * (q @ k.transpose(-1, -2))).abs(), 0.0).amax(-1)
    dg = 2.0 ** -9 * smax
    lnn = torch.log(mask.sum(-1).double()).view(1, 1, L)
    return 2 * dg * lnn.clamp(min=1.0) + 2.0 ** -9 * (lnn + 1), torch.expm1(2 * dg[:, :, qs]).unsqueeze(-1) + 2.0 ** -9


def test_msvit_analysis_on_both_routes(lib_built, monkeypatch):
    """attention_entropy and vil_attention_rows of the nano MsViT (112 x 80 images: ragged 28 x 20 and 14 x 10 grids, head_dim 48 and
    32) in bf16 mode: the fused route against the fp64 statement on the blocks' own qkv under its bounds; the fall-back route (P of the
    dense route reduced in torch) against the fused one at the sum of both routes' bounds.  The full-attention pairs are held to the
    flash statistics' own bound, 2 delta max(1, ln N) with delta = 1e-3 (1 + |lse|) (tests/test_attn_stats_gpu.py).

    The fall-back runs the dense route in fp32 (functional.vil_attention_stats): with the dense route in bf16 its rows reached 1.21 /
    1.16 of the summed bound in the two sliding-chunk pairs, because round-to-nearest to bf16's 8 significant bits errs by up to 2^-8
    relative in the stored scores and the stored P alike, where the allowance as tests/test_attn_stats_gpu.py writes it counts 2^-9
    (there the flash route's own 2e-3 (1 + |lse|) beside it hides the factor of two; the fused bound here is 1e-5 of p).  The
    allowance stays as it was set."""
    import esvit_amd
    from esvit_amd import analysis as A
    from esvit_amd import ops
    from tests.test_chunk_stats_cpu import block_inputs, nano_msvit
    assert torch.cuda.is_available(), "these tests need the MI355X"
    esvit_amd.set_precision("bf16")
    try:
        m = nano_msvit(((112, 80),)).to(DEV)
        B = 2
        x = torch.randn(B, 3, 112, 80, generator=torch.Generator().manual_seed(11)).to(DEV)
        grids = m.feature_grid(112, 80)
        pts = [(0, 0), (111, 79), (57, 30), 0, (57, 30)]
        strides = (4, 8)
        calls = {"n": 0}
        real = ops.chunk_attn_stats

        def counted(*a, **kw):
            calls["n"] += 1
            return real(*a, **kw)
        monkeypatch.setattr(ops, "chunk_attn_stats", counted)
        ent = A.attention_entropy(m, x, unit="nats")
        rows = A.vil_attention_rows(m, x, pts, blocks=[0, 1])
        assert calls["n"] == 4  # (two sliding-chunk pairs, twice: the kernels ran)
        monkeypatch.setattr(ops, "chunk_attn_stats_supported", lambda *a: False)
        ent_d = A.attention_entropy(m, x, unit="nats")
        rows_d = A.vil_attention_rows(m, x, pts, blocks=[0, 1])
        assert calls["n"] == 4  # (the fall-back did not)
        torch.cuda.synchronize()
        blocks = block_inputs(m, x, ops)
        assert len(ent) == len(blocks) == 4
        noted = []  # (every pair's figures are printed and recorded before the first assertion)
        for i, (qkv, nH, hd, (nglo, nx, ny), sparse) in enumerate(blocks):
            assert qkv.dtype == BF16 and ent[i].shape == (B, nH, nglo + nx * ny)
            if not sparse:
                e64, _, lse64 = AR.stats64(qkv.cpu(), B, nglo + nx * ny, nH, hd, hd ** -0.5)
                tol = 2e-3 * (1 + lse64.abs()) * max(1.0, math.log(nglo + nx * ny))
                noted.append((dict(entry="msvit_full", block=i), dict(ratio_ent=float(((ent[i].cpu().double() - e64).abs() / tol).max()))))
                continue
            qs = [p if isinstance(p, int) else nglo + (p[0] // strides[i]) * ny + p[1] // strides[i] for p in pts]
            ref, _ = R.bounds(qkv, B, nH, hd, nglo, nx, ny, hd ** -0.5, qs)
            got_rows = torch.cat([rows[i][1], rows[i][0].flatten(-2)], -1).cpu().double()
            dense_rows = torch.cat([rows_d[i][1], rows_d[i][0].flatten(-2)], -1).cpu().double()
            de, dr = _dense_allowance(qkv, B, nH, hd, nglo, nx, ny, qs)
            mm = dict(ratio_ent=CR.ratio(ent[i].cpu().double(), ref["ent"], ref["bd_ent"]), ratio_rows=CR.ratio(got_rows, ref["rows"], ref["bd_rows"]),
                      ratio_ent_vs_dense=CR.ratio(ent_d[i].cpu().double(), ent[i].cpu().double(), ref["bd_ent"] + de),
                      ratio_rows_vs_dense=CR.ratio(dense_rows, got_rows, ref["bd_rows"] + dr * ref["rows"] + 2.0 ** -23),
                      equal_masked_zero=float(bool((got_rows[..., ~ref["mask"][qs]] == 0).all()) and bool((dense_rows[..., ~ref["mask"][qs]] == 0).all())),
                      ratio_row_sum=float(((got_rows.sum(-1) - 1).abs() / ref["bd_rows"].sum(-1)).max()))
            noted.append((dict(entry="msvit_sparse", block=i), mm))
        for tag, mm in noted:
            _note(tag, mm)
        for tag, mm in noted:
            _check(tag, mm, note=False)
    finally:
        esvit_amd.set_precision("fp32")
