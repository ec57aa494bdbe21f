"""-m gpu: the window-statistics kernels (csrc/window_attn.hip attn_stats4, window_attn_big.hip attn_big_stats; ws |
ESVIT_ATTN_WINDOW_STATS behind ops.window_attn_stats) and the Swin side of esvit_amd.analysis on the MI355X, against the fp64 statement
of tests/window_attn_ref.py on its case table.  tests/window_stats_ref.py derives the bounds (its docstring): a listed row under bd_attn
of its elements; the entropy under sum_k (|ln P_k| + 1) bd_attn_k + twice (NK + 4) u sum_k P_k |s_k - m| + 2^-100, and inside
[0, ln N + bound].  tests/test_window_stats_cpu.py holds the fp32 restatement to the same bounds without a GPU.

The two routes of attention_entropy are compared at the sum of both routes' bounds: the fused route's bd_ent, and for the maps route
the first-order term of its own P (the forward's probability variant, under the same bd_attn) plus the fp32 reduction torch makes of
it, (N + 4) u H.  Observed error / bound ratios go to profiles/window_stats_parity_observed.jsonl, with the maps route's entropy error
against the same fp64 beside them for context (nothing is asserted on that figure), and the two peak allocations of the memory test."""
import ctypes as C
import json
import math
import os

import pytest
import torch

from tests import golden_utils as GU
from tests import window_attn_ref as WR
from tests import window_stats_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "window_stats_parity_observed.jsonl")
DEV = torch.device("cuda:0")
BF = torch.bfloat16
MOAT = 64  # floats of sentinel before and after every output


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


def _record(rec):
    print(json.dumps(rec))
    old = []
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            old = [json.loads(l) for l in f if l.strip()]
    old = [r for r in old if (r["test"], r["case"], r["dtype"]) != (rec["test"], rec["case"], rec["dtype"])]
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "w") as f:
        for r in old + [rec]:
            f.write(json.dumps(r) + "\n")


def _moated(shape):
    n = math.prod(shape)
    buf = torch.full((n + 2 * MOAT,), SR.SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[MOAT:MOAT + n].view(shape)


def _moat_ok(buf):
    return bool((buf[:MOAT] == SR.SENTINEL).all()) and bool((buf[-MOAT:] == SR.SENTINEL).all())


def _call(ops, case, dt, slots, table=True, bias_frag=None):
    """one launch: the qkv of the call between NaN rows, both outputs in sentinel moats -> (ent, rows, moats intact and outputs written)"""
    g, x = WR.geometry(case), WR.inputs(case, dt)
    nH, nB, N, nW, L = case["nH"], case["nB"], g["N"], g["nW"], g["L"]
    rows_n, C3 = nB * L, 3 * nH * case["hd"]
    qbuf = torch.full((rows_n + 2 * WR.GUARD, C3), float("nan"), dtype=dt, device=DEV)
    qbuf[WR.GUARD:WR.GUARD + rows_n] = x["qkv"].to(DEV)
    geom = SR.geom_of(case, DEV)
    ebuf, ent = _moated((nB * nW, nH, N))
    rbuf, rows = _moated((nB, nH, len(slots), N))
    e, r = ops.window_attn_stats(qbuf[WR.GUARD:WR.GUARD + rows_n], x["qb"].to(DEV), geom.win2tok, L, x["table"].to(DEV) if table else None, g["ws"],
                                 geom.region_ids, nW, N, nH, x["scale"], slots=slots, bias_frag=bias_frag, ent_out=ent, rows_out=rows)
    assert e.data_ptr() == ent.data_ptr() and r.data_ptr() == rows.data_ptr()
    ok = _moat_ok(ebuf) and _moat_ok(rbuf) and bool((ent != SR.SENTINEL).all()) and bool((rows != SR.SENTINEL).all())
    return ent, rows, ok


def _params(prefixes):
    ps = [p for p in WR.params() if p[0]["name"].startswith(prefixes)]
    return [pytest.param(c, dt, id="%s-%s" % (c["name"], WR.dt_name(dt))) for c, dt in ps]


def _run_case(ops, case, dt):
    g, x = WR.geometry(case), WR.inputs(case, dt)
    N, nW, nH = g["N"], g["nW"], case["nH"]
    assert ops.window_attn_stats_supported(dt, N, case["hd"])
    ref = SR.reference(case, dt)
    slots = ref["slots"]
    ent, rows, ok = _call(ops, case, dt, slots)
    m = SR.metrics(case, dt, ent, rows)
    m["equal_moat_and_written"] = float(ok)
    ent2, rows2, ok2 = _call(ops, case, dt, torch.tensor(slots, device=DEV))
    m["equal_repeat"] = float(ok2 and torch.equal(ent, ent2) and torch.equal(rows, rows2))
    m["equal_duplicate"] = float(torch.equal(rows[:, :, 4], rows[:, :, 5]))
    # rel_table = NULL after a filling call into the caller's fragment, the shared scratch poisoned in between
    frag = ops.new_bias_frag(nH, N, DEV)
    _call(ops, case, dt, slots, bias_frag=frag)
    ops.workspace(2 * nH * ops.attn_frag_elems(N), DEV, slot=2).fill_(float("nan"))
    ent3, rows3, ok3 = _call(ops, case, dt, slots, table=False, bias_frag=frag)
    m["equal_prefilled"] = float(ok3 and torch.equal(ent, ent3) and torch.equal(rows, rows3))
    # without a list: the same entropies, no rows
    geom = SR.geom_of(case, DEV)
    e4, none = ops.window_attn_stats(x["qkv"].to(DEV), x["qb"].to(DEV), geom.win2tok, g["L"], x["table"].to(DEV), g["ws"], geom.region_ids, nW, N, nH,
                                     x["scale"])
    m["equal_no_list"] = float(none is None and torch.equal(e4, ent))
    # context: the maps route (the probability variant of the forward, reduced in torch) against the same fp64
    attn = ops.window_attn_fwd(x["qkv"].to(DEV), x["qb"].to(DEV), geom.win2tok, g["L"], x["table"].to(DEV), g["ws"], geom.region_ids, nW, N, nH, x["scale"],
                               want_attn=True)[2]
    maps_ent = torch.special.entr(attn.float()).sum(-1).cpu().double()
    ctx = dict(maps_entropy_ratio=WR.ratio(maps_ent, ref["ent"], ref["bd_ent"]), maps_entropy_abs=float((maps_ent - ref["ent"]).abs().max()),
               entropy_abs=float((ent.cpu().double() - ref["ent"]).abs().max()),
               rows_equal_maps=float(torch.equal(rows.cpu(), SR.rows_of(attn.cpu(), case, slots))))
    _record(dict(test="kernel", case=case["name"], dtype=WR.dt_name(dt), **m, **ctx))
    WR.check("window_stats", case, dt, m)


@pytest.mark.parametrize("case,dt", _params("walk"))
def test_walk_cases(ops, case, dt):
    """wave pairs walking several windows with the mask on, pads and an inactive tail in the last round; dead key tiles; the 224-slot kernels"""
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params("range"))
def test_range_cases(ops, case, dt):
    """scores beyond 89, masked keys that keep probability, bias-dominated scores"""
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params("partial_grid"))
def test_partial_grid(ops, case, dt):
    """N = 37 of a 7 x 7 grid"""
    _run_case(ops, case, dt)


def test_refused_calls_leave_the_outputs_untouched(ops):
    """an unsupported shape through the wrapper, a bad slot through the wrapper's range check, and the flag beside another through the
    entry itself: sentinel-filled outputs stay as they were"""
    from esvit_amd import _lib
    lib = _lib.lib
    case = WR.BY_NAME["range14"]
    g, x = WR.geometry(case), WR.inputs(case, torch.float32)
    N, nW, nB, L = g["N"], g["nW"], case["nB"], g["L"]
    geom = SR.geom_of(case, DEV)
    qkv = x["qkv"].to(DEV)  # [nB L, 3 * 6 * 32] read as 3 heads of 64: fp32 at head_dim 64 on 196 slots does not exist
    ebuf, ent = _moated((nB * nW, 3, N))
    rbuf, rows = _moated((nB, 3, 2, N))
    table = torch.zeros(x["table"].shape[0], 3, device=DEV)
    assert not ops.window_attn_stats_supported(torch.float32, N, 64)
    with pytest.raises(RuntimeError, match="196 tokens at head_dim 64"):
        ops.window_attn_stats(qkv, x["qb"].to(DEV), geom.win2tok, L, table, g["ws"], geom.region_ids, nW, N, 3, 0.125, slots=[0, 5], ent_out=ent,
                              rows_out=rows)
    with pytest.raises(ValueError, match=r"\[0, %d\)" % (nW * N)):
        ops.window_attn_stats(qkv, x["qb"].to(DEV), geom.win2tok, L, x["table"].to(DEV), g["ws"], geom.region_ids, nW, N, 6, x["scale"],
                              slots=[0, nW * N], ent_out=_moated((nB * nW, 6, N))[1], rows_out=_moated((nB, 6, 2, N))[1])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    frag = ops.new_bias_frag(6, N, DEV)
    lst = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    qb, tab = x["qb"].to(DEV), x["table"].to(DEV)
    for ws, nq, out, lse in ((g["ws"] | ops.ATTN_WINDOW_STATS | ops.ATTN_SPLIT_DBIAS, 2, p(lst), p(rows)),
                             (g["ws"] | ops.ATTN_WINDOW_STATS, 2, None, p(rows)),
                             (g["ws"] | ops.ATTN_WINDOW_STATS, 0, None, p(rows))):
        rc = lib.esvit_window_attn_fwd(ops.F32, p(qkv), p(qb), p(geom.win2tok), L, p(tab), ws, p(frag), p(geom.region_ids), nW, nB, N | (nq << 16), 6, 32,
                                       x["scale"], out, lse, p(ent), None)
        assert rc == -1, lib.esvit_last_error()
    torch.cuda.synchronize()
    assert bool((ebuf == SR.SENTINEL).all()) and bool((rbuf == SR.SENTINEL).all())


# ---- esvit_amd.analysis on nano Swins ------------------------------------------------------------------------------------------------
@pytest.fixture()
def route():
    from esvit_amd import analysis as A
    old = A.SWIN_STATS

    def set_(r):
        A.SWIN_STATS = r
    yield set_
    A.SWIN_STATS = old


def _nano(window):
    from tests.test_composition_cpu import build_nano
    m = build_nano(window=window)
    GU.fill_state_dict(m.state_dict(), 0)
    return m.to(DEV).eval()


def _blocks(m):
    return [(li, blk) for li, layer in enumerate(m.layers) for blk in layer.blocks]


def _block_statements(m, x):
    """the fp64 statement of every block on that block's own qkv (recomputed with the library, as swin_block_attention does)"""
    import esvit_amd.functional as Fn
    from esvit_amd.models.swin_transformer import _grid, _hw_of
    o = Fn.ops_module()
    out = []
    with torch.no_grad():
        t, hw = m._tokens(x), m._image_grid(x)
        for layer in m.layers:
            for blk in layer.blocks:
                nB, L, Cc = t.shape
                H, W = _grid(L, hw)
                geom = Fn.geometry(H, W, blk.window_size, blk.shift_size, t.device)
                g1, b1, table, Wqkv, bqkv = blk._params()[:5]
                qkv = o.linear_fwd(o.layernorm_fwd(t.contiguous().view(nB * L, Cc), g1, b1, Fn.LN_EPS)[0], Fn._weight(Wqkv), bqkv)
                assert qkv.dtype == BF
                st = SR.block_statement(qkv, bqkv, table, geom.win2tok, geom.region_ids, nB, L, blk.num_heads, geom.ws, (Cc // blk.num_heads) ** -0.5, BF)
                st["geom"] = geom
                out.append(st)
                t, _ = blk(t, hw=hw)
            t = layer._down(t, hw)
            hw = _hw_of(layer, hw)
    return out


@pytest.mark.parametrize("size", [224, 96])
@pytest.mark.parametrize("window", [7, 14])
def test_nano_swin_routes_agree_and_rows_are_the_maps(lib_built, route, window, size):
    """bf16 nano Swins at W = 7 and W = 14 on 224^2 and 96^2 batches: "fused" entropies against "maps" within the sum of both routes'
    bounds (and each against fp64 within its own), swin_attention_rows against the maps under bd_attn twice (each route once), its rows
    + pad_mass = 1 and exact zeros outside the window, AttentionEntropyMeter under both routes within the same bound"""
    import esvit_amd
    from esvit_amd import analysis as A
    esvit_amd.set_precision("bf16")
    try:
        m = _nano(window)
        x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(size + window)).to(DEV)
        sts = _block_statements(m, x)
        route("maps")
        e_maps = A.attention_entropy(m, x, unit="nats")
        meter_maps = A.AttentionEntropyMeter("nats").update(m, x).compute()
        with torch.no_grad():
            maps = m.forward_selfattention(x, n=2)
        route("fused")
        e_fused = A.attention_entropy(m, x, unit="nats")
        meter_fused = A.AttentionEntropyMeter("nats").update(m, x).compute()
        assert len(e_fused) == len(e_maps) == len(sts) == 8
        worst = dict(fused=0.0, maps=0.0, routes=0.0, meter=0.0, rows=0.0, row_sum=0.0)
        for i, st in enumerate(sts):
            N = st["geom"].N
            bd_maps = st["first_order"] + (N + 4) * WR.U * st["ent"] + WR.FLOOR
            ef, em = e_fused[i].cpu().double(), e_maps[i].cpu().double()
            assert ef.shape == em.shape == st["ent"].shape and bool((ef >= 0).all()) and bool((ef <= math.log(N) + st["bd_ent"]).all())
            worst["fused"] = max(worst["fused"], float(((ef - st["ent"]).abs() / st["bd_ent"]).max()))
            worst["maps"] = max(worst["maps"], float(((em - st["ent"]).abs() / bd_maps).max()))
            worst["routes"] = max(worst["routes"], float(((ef - em).abs() / (st["bd_ent"] + bd_maps)).max()))
            both = (st["bd_ent"] + bd_maps).mean(-1).mean(0)  # the meter's mean over slots and windows of the per-slot bound
            worst["meter"] = max(worst["meter"], float(((meter_fused[i] - meter_maps[i]).abs().cpu() / both).max()))
        # rows of three points in a shifted block of stage 0, a block of stage 1 and the last block, against the maps
        points = [(0, 0), (size - 1, size - 1), (size // 2 + 3, size // 3)]
        chosen = [1, 3, -1]
        res = A.swin_attention_rows(m, x, points, chosen)
        grids = m.feature_grid(size, size)
        blocks = _blocks(m)
        for (rows, pad_mass), b in zip(res, chosen):
            b %= 8
            li, blk = blocks[b]
            st, geom = sts[b], sts[b]["geom"]
            N, nW, nH = geom.N, geom.nW, blk.num_heads
            gh, gw = grids[li]
            s = m.patch_embed.patch_size[0] << li
            assert rows.shape == (2, nH, 3, gh, gw) and pad_mass.shape == (2, nH, 3)
            flat = rows.flatten(-2).cpu().double()
            pm = maps[b].view(2, nW, nH, N, N).cpu().double()
            bd = st["bd_attn"].view(2, nW, nH, N, N)
            for n, (y, xx) in enumerate(points):
                slot = int(geom.tok2win[(y // s) * gw + xx // s])
                w, i = slot // N, slot % N
                tok = st["tok"][w]
                live = tok >= 0
                inside = torch.zeros(gh * gw, dtype=torch.bool)
                inside[tok[live]] = True
                assert bool((flat[:, :, n, ~inside] == 0).all())
                err = (flat[:, :, n][:, :, tok[live]] - pm[:, w, :, i][:, :, live]).abs()
                worst["rows"] = max(worst["rows"], float((err / (2 * bd[:, w, :, i][:, :, live])).max()))
                total = flat[:, :, n].sum(-1) + pad_mass[:, :, n].cpu().double()
                worst["row_sum"] = max(worst["row_sum"], float(((total - 1).abs() / (bd[:, w, :, i].sum(-1) + N * WR.U)).max()))
        _record(dict(test="nano_swin", case="w%d_%d" % (window, size), dtype="bf16", **{"ratio_" + k: v for k, v in worst.items()}))
        assert all(v <= 1.0 for v in worst.values()), worst
    finally:
        esvit_amd.set_precision("fp32")


def test_fused_route_stays_below_one_map_tensor(lib_built, route):
    """a nano-width W = 14 Swin, 224^2, B = 4: the peak allocation above the live inputs of the fused route stays below the byte size of
    ONE block's stage-0 map tensor [B nW, nH, N, N] in fp32 (computed from the shape: 4 * 16 windows, 1 head, 196^2 floats = 9.8 MB);
    the maps route keeps every block's at once.  Both peaks are recorded."""
    import esvit_amd
    from esvit_amd import analysis as A
    esvit_amd.set_precision("bf16")
    try:
        m = _nano(14)
        x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(4)).to(DEV)
        blk = m.layers[0].blocks[0]
        one_map = 4 * (56 // 14) ** 2 * blk.num_heads * 196 * 196 * 4
        peaks = {}
        for r in ("fused", "maps"):
            route(r)
            A.attention_entropy(m, x)  # (weights cast, the library's shared scratch sized before the measurement)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ent = A.attention_entropy(m, x)
            torch.cuda.synchronize()
            peaks[r] = torch.cuda.max_memory_allocated() - base
            assert len(ent) == 8 and all(bool(torch.isfinite(e).all()) for e in ent)
            del ent
    finally:
        esvit_amd.set_precision("fp32")
    _record(dict(test="memory", case="w14_224_b4", dtype="bf16", fused_peak_above_inputs_MB=peaks["fused"] / 1e6,
                 maps_peak_above_inputs_MB=peaks["maps"] / 1e6, one_stage0_map_MB=one_map / 1e6))
    assert peaks["fused"] < one_map, (peaks, one_map)
