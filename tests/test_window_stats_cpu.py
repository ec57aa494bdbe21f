"""-m "not gpu": the window-statistics mode (ws | ESVIT_ATTN_WINDOW_STATS of esvit_window_attn_fwd: entropy of every row of the window
softmax, probability rows of listed slots) and the Swin side of esvit_amd.analysis without a GPU -- the argument checks of the C entry,
the host's range check, the fall-back route of functional.window_attention_stats over oracle/ops_ref.py against the fp64 statement on
every case of tests/window_attn_ref.py under the bounds the GPU test uses (tests/window_stats_ref.py derives them), three mutants of
the reduction, and attention_entropy / swin_attention_rows / AttentionEntropyMeter on the nano Swin."""
import ctypes as C
import os

import pytest
import torch

from oracle import ops_ref
from tests import golden_utils as GU
from tests import window_attn_ref as WR
from tests import window_stats_ref as SR
from tests.test_composition_cpu import build_nano, cpu_ops  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def test_window_stats_mode_is_refused_where_it_must_be(lib_built):
    """one rejection per argument check of the mode, ESVIT_ERR_ARG before any launch (a launch on this GPU-less host would come back as
    ESVIT_ERR_HIP), the cause in esvit_last_error(); then the host's range check of the slot list"""
    from esvit_amd import _lib, ops
    lib = _lib.lib
    fake = C.c_void_p(0x1000)  # never dereferenced: the argument checks come first
    WS, G, S, K, D = ops.ATTN_WINDOW_STATS, ops.ATTN_GLOBAL, ops.ATTN_STATS, ops.ATTN_SLIDING_CHUNK, ops.ATTN_SPLIT_DBIAS

    def fwd(dtype=ops.BF16, hd=32, ws=7 | WS, N=49, nq=0, out=None, lse=None, attn=fake, bias=fake, w2t=fake, frag=fake):
        rc = lib.esvit_window_attn_fwd(dtype, fake, bias, w2t, 144, None, ws, frag, None, 4, 2, N | (nq << 16), 3, hd, 0.17, out, lse, attn, None)
        return rc, lib.esvit_last_error()

    def bwd(ws):
        rc = lib.esvit_window_attn_bwd(ops.BF16, fake, fake, fake, 144, fake, fake, fake, None, ws, fake, None, 4, 2, 49, 3, 32, 0.17, fake,
                                       fake, fake, None)
        return rc, lib.esvit_last_error()
    for got, cause in ((bwd(7 | WS), b"esvit_window_attn_fwd only"),                       # the flag in the backward entry
                       (bwd(14 | WS | D), b"esvit_window_attn_fwd only"),
                       (fwd(ws=7 | WS | K), b"together with ESVIT_ATTN_SLIDING_CHUNK"),    # together with each other mode flag
                       (fwd(ws=7 | WS | G), b"together with ESVIT_ATTN_GLOBAL"),
                       (fwd(ws=WS | G | S), b"together with ESVIT_ATTN_GLOBAL"),
                       (fwd(ws=7 | WS | S), b"together with ESVIT_ATTN_STATS"),
                       (fwd(ws=14 | WS | D, N=196), b"together with ESVIT_ATTN_SPLIT_DBIAS"),
                       (fwd(out=fake), b"out must be NULL"),                               # each must-be-NULL argument
                       (fwd(lse=fake), b"lse must be NULL"),
                       (fwd(attn=None), b"attn_out"),                                      # a missing output
                       (fwd(nq=3, out=fake), b"without the rows output"),
                       (fwd(nq=3, lse=fake), b"without the list"),                         # nq without a list
                       (fwd(dtype=7), b"bad dtype"),                                       # unsupported (dtype, N, hd)
                       (fwd(hd=48), b"head_dim 48"),
                       (fwd(dtype=ops.F32, hd=64, ws=14 | WS, N=196), b"196 tokens at head_dim 64"),
                       (fwd(ws=15 | WS, N=225), b"225 tokens"),
                       (fwd(ws=7 | WS, N=50), b"bad args"),
                       (fwd(ws=WS), b"bad args"),                                          # the flag without a window side
                       (fwd(bias=None), b"bad args"),
                       (fwd(w2t=None), b"bad args"),
                       (fwd(frag=None), b"bias_frag_ws")):
        assert got[0] == -1 and cause in got[1], (got, cause)
    # what existed is refused as before, with its own messages
    rc = lib.esvit_window_attn_fwd(ops.BF16, fake, None, fake, 785, None, S | 7, None, None, 3, 2, 785, 3, 64, 0.125, None, None, fake, None)
    assert rc == -1 and b"only together with ESVIT_ATTN_GLOBAL" in lib.esvit_last_error()
    assert ops.window_attn_stats_supported(torch.bfloat16, 49, 32) and ops.window_attn_stats_supported(torch.float32, 37, 64)
    assert ops.window_attn_stats_supported(torch.float32, 196, 32) and ops.window_attn_stats_supported(torch.bfloat16, 196, 64)
    assert not ops.window_attn_stats_supported(torch.float32, 196, 64) and not ops.window_attn_stats_supported(torch.bfloat16, 225, 32)
    assert not ops.window_attn_stats_supported(torch.bfloat16, 49, 48) and not ops.window_attn_stats_supported(torch.float16, 49, 32)
    # the slot list is checked on the host, before the library is called (which cannot read the array)
    qkv = torch.zeros(2 * 144, 3 * 96, dtype=torch.bfloat16)
    w2t = torch.zeros(4 * 49, dtype=torch.int32)
    for bad in ([0, 196], [-1], torch.tensor([5, 1000])):
        with pytest.raises(ValueError, match=r"\[0, 196\)"):
            ops.window_attn_stats(qkv, torch.zeros(288), w2t, 144, torch.zeros(169, 3), 7, None, 4, 49, 3, 0.17, slots=bad)


def test_header_constant_equals_ops_constant(lib_built):
    from esvit_amd import ops
    hdr = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "#define ESVIT_ATTN_WINDOW_STATS 0x%08x\n" % ops.ATTN_WINDOW_STATS in hdr
    others = (ops.ATTN_GLOBAL, ops.ATTN_SLIDING_CHUNK, ops.ATTN_STATS, ops.ATTN_SPLIT_DBIAS)
    for name, f in zip(("GLOBAL", "SLIDING_CHUNK", "STATS", "SPLIT_DBIAS"), others):
        assert "#define ESVIT_ATTN_%s 0x%x" % (name, f) in hdr or "#define ESVIT_ATTN_%s 0x%08x" % (name, f) in hdr
        assert ops.ATTN_WINDOW_STATS & f == 0
    assert 224 < ops.ATTN_WINDOW_STATS < 2 ** 31 and ops.ATTN_WINDOW_STATS & 0xffffff == 0  # a window side and N | nq << 16 fit beside it


def _fallback(case, dt, slots):
    """functional.window_attention_stats on oracle/ops_ref (no window_attn_stats there): bf16-valued fp32 inputs, maps reduced in torch"""
    import esvit_amd.functional as Fn
    assert not hasattr(ops_ref, "window_attn_stats")
    g, x = WR.geometry(case), WR.inputs(case, dt)
    old, old_slice = ops_ref.act_dtype(), Fn._STATS_SLICE_ELEMS
    ops_ref.set_act_dtype(torch.float32)
    try:
        Fn._STATS_SLICE_ELEMS = 3 * g["nW"] * case["nH"] * g["N"] ** 2  # three images per slice: several slices, a ragged last one
        return Fn.window_attention_stats(ops_ref, x["qkv"].float(), x["qb"], SR.geom_of(case, CPU), g["L"], x["table"], case["nH"], x["scale"],
                                         slots)
    finally:
        ops_ref.set_act_dtype(old)
        Fn._STATS_SLICE_ELEMS = old_slice


@pytest.mark.parametrize("case,dt", WR.params(), ids=WR.ids(WR.params()))
def test_fallback_route_stays_inside_the_gpu_bounds(case, dt):
    """the fp32 restatement against the fp64 statement on every case, under the bounds of tests/window_stats_ref.py: they are achievable"""
    ref = SR.reference(case, dt)
    ent, rows = _fallback(case, dt, ref["slots"])
    g = WR.geometry(case)
    assert ent.shape == (case["nB"] * g["nW"], case["nH"], g["N"]) and rows.shape == (case["nB"], case["nH"], len(ref["slots"]), g["N"])
    assert ent.dtype == rows.dtype == torch.float32 and torch.equal(rows[:, :, 4], rows[:, :, 5])
    m = SR.metrics(case, dt, ent, rows)
    WR.check("window_stats_fallback", case, dt, m)
    e2, none = _fallback(case, dt, None)
    assert none is None and torch.equal(e2, ent)


# mutant -> the cases named for it (each must push some figure over its bound there)
MUTANT_CASES = {
    "pad_keys_out": ("walk7", "walk14", "walk7_hd64"),                      # windows with zero-pad key slots
    "mask_ignored": ("range7_hd32", "range7_bias", "range14", "walk7"),     # shifted windows: masked keys
    "neighbour_window": ("walk7", "walk7_noshift", "walk14", "range7_hd64"),  # more than one window per image
}


@pytest.mark.parametrize("which", SR.MUTANTS)
def test_mutants_of_the_reduction_are_caught(which):
    for name in MUTANT_CASES[which]:
        case = WR.BY_NAME[name]
        for dt in case["dts"]:
            ent, rows = SR.mutant(case, dt, which)
            m = SR.metrics(case, dt, ent, rows)
            assert WR.failures(m), (which, name, WR.dt_name(dt), m)
    # the same restatement without the mistake is the reference itself
    case = WR.BY_NAME["walk7"]
    ref = SR.reference(case, torch.float32)
    assert not WR.failures(SR.metrics(case, torch.float32, ref["ent"], ref["rows"]))


def test_block_statement_is_the_statement_of_the_case_table():
    """window_stats_ref.block_statement (the fp64 statement for a model's block, used by the GPU test) on the inputs of a case: the
    probabilities and the derived bound of window_attn_ref.statement"""
    case = WR.BY_NAME["range7_hd32"]
    for dt in WR.DTYPES:
        g, x, want = WR.geometry(case), WR.inputs(case, dt), WR.statement(case, dt)
        got = SR.block_statement(x["qkv"], x["qb"], x["table"], g["tok"].reshape(-1), g["reg"].reshape(-1), case["nB"], g["L"], case["nH"], g["ws"],
                                 x["scale"], dt)
        assert (got["attn"] - want["attn"]).abs().max().item() <= 1e-13
        assert ((got["bd_attn"] - want["bd_attn"]).abs() <= 1e-9 * want["bd_attn"]).all()
        assert torch.equal(got["pad"], g["tok"] < 0)


def test_slot_lists_reach_the_corners(lib_built):
    """every case lists the first and last slot of the first and last window and a slot alone in its 16-slot tile, twice"""
    for case in WR.CASES:
        g, s = WR.geometry(case), SR.slot_list(case)
        assert s[:4] == [0, g["N"] - 1, (g["nW"] - 1) * g["N"], g["nW"] * g["N"] - 1] and s[4] == s[5] and 0 <= s[4] < g["nW"] * g["N"]
        print(case["name"], s, SR.lonely_tile_live(case))
        if g["N"] % 16 == 1:  # 7 x 7: slot 48 is the only slot of tile 3
            assert SR.lonely_tile_live(case) == 1, case["name"]


# ---- esvit_amd.analysis on the nano Swin -----------------------------------------------------------------------------------------
def _nano():
    m = build_nano()
    GU.fill_state_dict(m.state_dict(), 0)
    return m.eval()


def _images(B, H, W, seed):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


@pytest.fixture()
def route():
    from esvit_amd import analysis as A
    old = A.SWIN_STATS

    def set_(r):
        A.SWIN_STATS = r
    yield set_
    A.SWIN_STATS = old


def _hand_rows(m, x, points, b):
    """the rows of block b cut out of forward_selfattention's maps and scattered with Fn.geometry's win2tok, slot by slot"""
    import esvit_amd.functional as Fn
    with torch.no_grad():
        maps = m.forward_selfattention(x, n=2)
    blocks = [(li, blk) for li, layer in enumerate(m.layers) for blk in layer.blocks]
    li, blk = blocks[b]
    gh, gw = m.feature_grid(x.shape[2], x.shape[3])[li]
    s = m.patch_embed.patch_size[0] << li
    geom = Fn.geometry(gh, gw, blk.window_size, blk.shift_size, x.device)
    N, nW = geom.N, geom.nW
    w2t = geom.win2tok.long().tolist()
    p = maps[b].view(x.shape[0], nW, blk.num_heads, N, N)
    rows = torch.zeros(x.shape[0], blk.num_heads, len(points), gh * gw)
    pad = torch.zeros(x.shape[0], blk.num_heads, len(points))
    inside = torch.zeros(len(points), gh * gw, dtype=torch.bool)
    for n, (y, xx) in enumerate(points):
        slot = w2t.index((y // s) * gw + xx // s)
        w, i = slot // N, slot % N
        for j in range(N):
            t = w2t[w * N + j]
            if t >= 0:
                rows[:, :, n, t] = p[:, w, :, i, j]
                inside[n, t] = True
            else:
                pad[:, :, n] += p[:, w, :, i, j]
    return rows.view(x.shape[0], blk.num_heads, len(points), gh, gw), pad, inside.view(len(points), gh, gw)


@pytest.mark.parametrize("H,W", [(96, 96), (96, 64)])
def test_nano_swin_fused_equals_maps_and_rows_equal_the_cut_maps(cpu_ops, route, H, W):  # noqa: F811
    """a 96^2 batch (pads, shifted blocks with the 4-region mask) and a rectangular one.  Both routes are the fall-back here (ops_ref has
    no statistics entry): entropies exactly equal; swin_attention_rows exactly the rows cut by hand out of the maps, zero outside the
    window exactly, rows + pad_mass = 1 within 1e-6"""
    from esvit_amd import analysis as A
    m = _nano()
    x = _images(2, H, W, 5)
    route("maps")
    want = A.attention_entropy(m, x)
    want_q = A.attention_entropy(m, x, queries=[0, 48, 7], unit="nats")
    meter_maps = A.AttentionEntropyMeter().update(m, x).compute()
    route("fused")
    got = A.attention_entropy(m, x)
    got_q = A.attention_entropy(m, x, queries=[0, 48, 7], unit="nats")
    meter_fused = A.AttentionEntropyMeter().update(m, x).compute()
    assert len(got) == len(want) == sum(GU.NANO["depths"])
    for a, b in zip(got + got_q + meter_fused, want + want_q + meter_maps):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    points = [(0, 0), (H - 1, W - 1), (40, 57 if W > 64 else 20)]
    blocks = [5, 0, -1, 3]
    for r in ("maps", "fused"):  # (swin_attention_rows does not depend on the switch)
        route(r)
        res = A.swin_attention_rows(m, x, points, blocks)
        assert len(res) == 4
        for (rows, pad), b in zip(res, blocks):
            hr, hp, inside = _hand_rows(m, x, points, b % 8)
            assert rows.shape == hr.shape and rows.dtype == torch.float32 and pad.shape == hp.shape
            assert torch.equal(rows, hr)
            assert (pad - hp).abs().max().item() <= 1e-6
            assert ((rows.sum((-1, -2)) + pad - 1).abs() <= 1e-6).all()
            assert bool((rows[:, :, ~inside] == 0).all()) and bool((rows >= 0).all())
            masks = A.attention_mass_masks(rows.flatten(-2))
            assert masks.shape == rows.flatten(-2).shape
    last = A.swin_attention_rows(m, x, points)
    assert len(last) == 1 and torch.equal(last[0][0], res[2][0])


def test_swin_attention_rows_lists_and_errors(cpu_ops, route):  # noqa: F811
    from esvit_amd import analysis as A
    m = _nano()
    xs = [_images(1, 96, 96, 1), _images(2, 64, 96, 2)]
    pts = [(10, 10), (63, 95)]
    both = A.swin_attention_rows(m, xs, pts, blocks=[-1, 2])
    assert isinstance(both, list) and len(both) == 2
    for x, res in zip(xs, both):
        single = A.swin_attention_rows(m, x, pts, blocks=[-1, 2])
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(res, single))
        grids = m.feature_grid(x.shape[2], x.shape[3])
        assert res[0][0].shape[-2:] == grids[3] and res[1][0].shape[-2:] == grids[1] and res[0][0].shape[0] == x.shape[0]
    route("fused")
    ents = A.attention_entropy(m, xs)
    assert len(ents) == 2 and all(len(e) == 8 for e in ents)
    x = xs[0]
    with pytest.raises(ValueError, match="outside"):
        A.swin_attention_rows(m, x, [(96, 0)])
    with pytest.raises(ValueError, match="outside"):
        A.swin_attention_rows(m, x, [(0, -1)], blocks=[0])
    with pytest.raises(ValueError, match="block indices"):
        A.swin_attention_rows(m, x, pts, blocks=[8])
    with pytest.raises(ValueError, match="at least one point"):
        A.swin_attention_rows(m, x, [])
    with pytest.raises(TypeError, match="SwinTransformer"):
        A.swin_attention_rows(torch.nn.Linear(2, 2), x, pts)
    with pytest.raises(TypeError, match="VisionTransformer"):
        A.attention_rows(m, x, [0])
    route("both")
    with pytest.raises(ValueError, match="maps or fused"):
        A.attention_entropy(m, x)


# ---- routing, with a recording stand-in for the ops module -----------------------------------------------------------------------
class _Rec:
    """oracle.ops_ref with every call recorded by name (and the want_attn keyword of window_attn_fwd)"""

    def __init__(self, calls, with_stats=False):
        self._calls = calls
        if with_stats:
            self.window_attn_stats_supported = lambda dtype, N, hd: True
            self.window_attn_stats = self._stats

    def _stats(self, qkv, qkv_bias, win2tok, L, rel_table, ws, region_ids, nW, N, nH, scale, slots=None):
        self._calls.append(("window_attn_stats", None))
        return torch.zeros(qkv.shape[0] // L * nW, nH, N), None

    def __getattr__(self, name):
        attr = getattr(ops_ref, name)
        if not callable(attr) or name in ("act_dtype", "set_act_dtype"):
            return attr

        def call(*a, **k):
            self._calls.append((name, k.get("want_attn")))
            return attr(*a, **k)
        return call


def _with_rec(monkeypatch, with_stats=False):
    import esvit_amd.functional as Fn
    import esvit_amd.loss as L
    import esvit_amd.params as P
    calls = []
    stub = _Rec(calls, with_stats)
    for mod in (Fn, L, P):
        monkeypatch.setattr(mod, "ops", stub)
    ops_ref.set_act_dtype(torch.float32)
    P.clear()
    Fn._GEOM.clear()
    return calls


def test_default_route_issues_the_calls_of_today(monkeypatch, lib_built, route):
    """"maps" (the default): exactly the library calls of forward_selfattention(n=2), nothing else; "fused" on an ops module with the
    entry: one statistics call per block and no probability variant of the forward at all"""
    import esvit_amd.functional as Fn
    import esvit_amd.params as P
    from esvit_amd import analysis as A
    assert os.environ.get("ESVIT_SWIN_ATTN_STATS", "maps") != "maps" or A.SWIN_STATS == "maps"
    try:
        calls = _with_rec(monkeypatch)
        m = _nano()
        x = _images(1, 96, 96, 3)
        route("maps")
        with torch.no_grad():
            m.forward_selfattention(x, n=2)  # (the weights are cast and cached by the first pass)
        del calls[:]
        A.attention_entropy(m, x)
        got = list(calls)
        del calls[:]
        with torch.no_grad():
            m.forward_selfattention(x, n=2)
        assert got == list(calls) and sum(1 for n, w in got if n == "window_attn_fwd" and w) == 8
        assert not any(n == "window_attn_stats" for n, _ in got)
        calls = _with_rec(monkeypatch, with_stats=True)
        route("fused")
        ent = A.attention_entropy(m, x)
        assert len(ent) == 8 and sum(1 for n, _ in calls if n == "window_attn_stats") == 8
        assert not any(n == "window_attn_fwd" and w for n, w in calls)
    finally:
        P.clear()
        Fn._GEOM.clear()
