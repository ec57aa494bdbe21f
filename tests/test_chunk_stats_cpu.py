"""-m "not gpu": the attention statistics of Vision Longformer's sliding-chunk softmax (entropy of every row, probability rows of listed
queries; the mode ESVIT_ATTN_SLIDING_CHUNK | ESVIT_ATTN_CHUNK_STATS of esvit_window_attn_fwd) and esvit_amd.analysis on an MsViT without
a GPU -- the fp64 statement of tests/chunk_stats_ref.py against the one of tests/chunk_attn_ref.py, the combine's range-merge recurrence
in fp64, the bounds against the fp32 restatement and the mutants they catch, the argument checks of the C entry, the fall-back of
functional.vil_attention_stats on an ops module without the entry, and the public functions on the torch restatement of every kernel."""
import ctypes as C
import math
import os

import pytest
import torch

from oracle import ops_ref
from tests import attn_stats_ref as AR
from tests import chunk_attn_ref as CR
from tests import chunk_stats_ref as R
from tests import golden_utils as GU
from tests.test_composition_cpu import cpu_ops  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
CASE_IDS = [c["name"] for c in CR.CASES]
NANO_ARCH = 'l1,h1,d48,n1,s1,g1,p4,f7_l2,h3,d96,n1,s1,g1,p2,f7_l3,h3,d192,n1,s0,g1,p2,f7_l4,h6,d384,n1,s0,g0,p2,f7'  # vil_tiny with n9 -> n1


def _rel_equal(a, b, tol=1e-12):
    return bool(((a - b).abs() <= tol * b.abs()).all())


@pytest.mark.parametrize("case", CR.CASES, ids=CASE_IDS)
def test_statement_equals_the_forward_statement(case):
    """P and its derived bound are those of chunk_attn_ref.statement(case, bf16, "fused") to 1e-12 relative; the entropy is
    sum entr(P) to 1e-12; every listed row is a row of P"""
    x = CR.inputs(case, BF16)
    qs = R.default_queries(case["nglo"], case["nx"], case["ny"])
    got = R.stats64(x["qkv"], case["B"], case["nH"], case["hd"], case["nglo"], case["nx"], case["ny"], x["scale"], qs)
    ref = CR.statement(case, BF16, "fused")
    assert torch.equal(got["mask"], ref["mask"])
    assert _rel_equal(got["attn"], ref["attn"]) and _rel_equal(got["bd_attn"], ref["bd_attn"])
    want = torch.special.entr(ref["attn"]).sum(-1)
    assert (got["ent"] - want).abs().max().item() <= 1e-12 * (1 + want.abs().max().item())
    assert torch.equal(got["rows"], got["attn"][:, :, qs]) and (got["rows"][..., ~got["mask"][qs]] == 0).all()
    assert len(qs) == case["nglo"] + 5 and qs[-1] == qs[-2] and all(0 <= t < case["L"] for t in qs)
    assert (got["bd_ent"] > 0).all() and (got["bd_rows"] > 0).all()


@pytest.mark.parametrize("L", [2, 23, 512, 513, 1025])
def test_range_merge_recurrence_equals_direct_entropy(L):
    """the combine's recurrence over 512-key ranges against sum -p ln p in fp64, to 1e-12: random rows, a one-hot row (H = 0 exactly, no
    NaN: every other range's weight underflows), a maximum in the last range (one token at L = 513, 1025), uniform rows (H = ln of the
    visible keys), and the two mutants of the recurrence, which miss by far"""
    g = torch.Generator().manual_seed(L)
    s = 4 * torch.randn(6, L, generator=g, dtype=torch.float64)
    allowed = torch.ones(6, L, dtype=torch.bool)
    s[1, L - 1] = s[1].max() + 9.0
    s[2, :] = 0.0
    s[2, L // 2] = 2000.0
    s[3, 0] = s[3].max() + 30.0
    s[4, :] = 1.25
    s[5, :] = -3.5
    allowed[5] = torch.rand(L, generator=g) < 0.5
    allowed[5, ::CR.GSPLIT] = True  # (every range keeps a key, as every range of the kernel has one)
    sf = s.masked_fill(~allowed, float("-inf"))
    want = torch.special.entr(torch.softmax(sf, -1)).sum(-1)
    got = R.merge_ranges64(s, allowed)
    assert torch.isfinite(got).all()
    assert (got - want).abs().max().item() <= 1e-12
    assert got[2].item() == 0.0
    assert abs(got[4].item() - math.log(L)) <= 1e-12 and abs(got[5].item() - math.log(int(allowed[5].sum()))) <= 1e-12
    if L > CR.GSPLIT:
        for mutant in ("combine_no_shift", "no_rescale"):
            assert (R.merge_ranges64(s, allowed, mutant) - want).abs().max().item() > 1e-3, mutant


@pytest.mark.parametrize("case", CR.CASES, ids=CASE_IDS)
def test_fp32_restatement_sits_under_every_bound(case):
    ref, (ent32, rows32), qs = R.case_reference(case)
    m = dict(ratio_ent=CR.ratio(ent32, ref["ent"], ref["bd_ent"]), ratio_rows=CR.ratio(rows32, ref["rows"], ref["bd_rows"]),
             derived_ent=CR.ratio(ent32, ref["ent"], ref["bd_ent_derived"]), derived_rows=CR.ratio(rows32, ref["rows"], ref["bd_rows_derived"]))
    print("OBSERVED", case["name"], m)
    assert max(m.values()) <= 1.0, m  # (under the final bounds and under the derived ones alone)
    assert (rows32[..., ~ref["mask"][qs]] == 0).all()


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_leaves_its_bound(mutant):
    cases, what = R.MUTANTS[mutant]
    for name in cases:
        case = CR.BY_NAME[name]
        ref, _, qs = R.case_reference(case)
        x = CR.inputs(case, BF16)
        got = R.stats64(x["qkv"], case["B"], case["nH"], case["hd"], case["nglo"], case["nx"], case["ny"], x["scale"], qs, mutant=mutant, want_bounds=False)
        worst = max(CR.ratio(got["ent"], ref["ent"], ref["bd_ent"]), CR.ratio(got["rows"], ref["rows"], ref["bd_rows"]))
        print("OBSERVED", mutant, name, worst)
        assert worst >= 2.0, (mutant, what, name, worst)


def test_stats_mode_is_refused_where_it_must_be(lib_built):
    """one rejection per argument check of the mode, ESVIT_ERR_ARG before any launch (a launch on this GPU-less host would come back as
    ESVIT_ERR_HIP), the cause in esvit_last_error(); the rejections older tests pin keep their messages"""
    from esvit_amd import _lib, ops
    lib = _lib.lib
    fake = C.c_void_p(0x1000)  # never dereferenced: the argument checks come first
    K, T = ops.ATTN_SLIDING_CHUNK, ops.ATTN_CHUNK_STATS
    G, S, WS, SD = ops.ATTN_GLOBAL, ops.ATTN_STATS, ops.ATTN_WINDOW_STATS, ops.ATTN_SPLIT_DBIAS
    nx = ny = 14

    def fwd(dtype=ops.BF16, hd=32, nglo=1, ws=7 | K | T, nq=2, out=fake, rows=fake, attn=fake, bias=None, table=None, region=None, tab=fake, frag=fake, N=None):
        L = nglo + nx * ny
        rc = lib.esvit_window_attn_fwd(dtype, fake, bias, tab, L, table, ws, frag, region, nx, 2, ny | (nq << 16) if N is None else N, 2, hd, 0.125,
                                       out, rows, attn, None)
        return rc, lib.esvit_last_error()

    def bwd(ws):
        rc = lib.esvit_window_attn_bwd(ops.BF16, fake, None, fake, 197, fake, fake, fake, None, ws, fake, None, nx, 2, ny, 2, 32, 0.125, fake, None, None, None)
        return rc, lib.esvit_last_error()
    for got, cause in ((fwd(ws=7 | T), b"ESVIT_ATTN_SLIDING_CHUNK is missing"),              # the flag without the sliding-chunk flag
                       (fwd(ws=T), b"ESVIT_ATTN_SLIDING_CHUNK is missing"),
                       (bwd(7 | K | T), b"esvit_window_attn_fwd only"),                       # in the backward entry
                       (bwd(7 | T), b"esvit_window_attn_fwd only"),
                       (fwd(ws=7 | K | T | G), b"ESVIT_ATTN_CHUNK_STATS together with ESVIT_ATTN_GLOBAL"),
                       (fwd(ws=7 | K | T | S), b"ESVIT_ATTN_CHUNK_STATS together with ESVIT_ATTN_STATS"),
                       (fwd(ws=7 | K | T | WS), b"ESVIT_ATTN_CHUNK_STATS together with ESVIT_ATTN_WINDOW_STATS"),
                       (fwd(ws=7 | K | T | SD), b"ESVIT_ATTN_CHUNK_STATS together with ESVIT_ATTN_SPLIT_DBIAS"),
                       (fwd(out=None), b"without the list"),                                   # nq > 0 without the list / the rows
                       (fwd(rows=None), b"without the rows output"),
                       (fwd(nq=0), b"out must be NULL"),                                       # nq = 0 with either
                       (fwd(nq=0, out=None), b"lse must be NULL"),
                       (fwd(attn=None), b"attn_out"),
                       (fwd(dtype=ops.F32), b"bf16"),
                       (fwd(hd=40), b"head_dim 40"),
                       (fwd(ws=8 | K | T), b"chunk side"),
                       (fwd(nglo=8), b"global tokens"),
                       (fwd(bias=fake), b"pass NULL"),
                       (fwd(table=fake), b"pass NULL"),
                       (fwd(region=fake), b"pass NULL"),
                       (fwd(tab=None), b"are required"),
                       (fwd(frag=None), b"are required"),
                       (fwd(N=0), b"must be positive")):
        assert got[0] == -1 and cause in got[1], (got, cause)
    # the rejections existing tests pin still give their old messages
    def old(entry, ws, L=785, nW=1, N=785):
        if entry == "fwd":
            rc = lib.esvit_window_attn_fwd(ops.BF16, fake, None, fake, L, None, ws, None, None, nW, 2, N, 3, 64, 0.125, None, None, fake, None)
        else:
            rc = lib.esvit_window_attn_bwd(ops.BF16, fake, None, None, L, fake, fake, fake, None, ws, fake, None, nW, 2, N, 3, 64, 0.125, fake, None, None, None)
        return rc, lib.esvit_last_error()
    for got, cause in ((old("fwd", G | S | K), b"both mode flags"), (old("bwd", G | S | K), b"both mode flags"), (old("fwd", G | K), b"both mode flags"),
                       (old("fwd", 7 | WS | K), b"together with ESVIT_ATTN_SLIDING_CHUNK"),
                       (old("fwd", S), b"only together with ESVIT_ATTN_GLOBAL"), (old("fwd", S | 7), b"only together with ESVIT_ATTN_GLOBAL"),
                       (old("bwd", S | 7), b"only together with ESVIT_ATTN_GLOBAL")):
        assert got[0] == -1 and cause in got[1], (got, cause)
    # the plain sliding-chunk forward still refuses attn_out
    rc = lib.esvit_window_attn_fwd(ops.BF16, fake, None, fake, 197, None, 7 | K, fake, None, nx, 2, ny, 2, 32, 0.125, fake, fake, fake, None)
    assert rc == -1 and b"attn_out is not available" in lib.esvit_last_error()
    assert all(ops.chunk_attn_stats_supported(BF16, hd, 7, g) for hd in (32, 48, 64) for g in (0, 1, 7))
    assert not ops.chunk_attn_stats_supported(torch.float32, 32, 7, 1) and not ops.chunk_attn_stats_supported(BF16, 40, 7, 1)
    assert not ops.chunk_attn_stats_supported(BF16, 32, 7, 8) and not ops.chunk_attn_stats_supported(BF16, 32, 8, 1)
    # the query list is checked on the host, before the library is called (which cannot read the array)
    qkv = torch.zeros(2 * 5, 3 * 64, dtype=BF16)
    lay = (torch.tensor([-1, 0, 0, 0, 0], dtype=torch.int32), 1, 14)
    for bad in ([0, 5], [-1], torch.tensor([1, 7])):
        with pytest.raises(ValueError, match=r"chunk_attn_stats.*\[0, 5\)"):
            ops.chunk_attn_stats(qkv, 2, 5, 2, 0.2, lay, queries=bad)


def test_header_constant_equals_ops_constant(lib_built):
    from esvit_amd import ops
    hdr = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "#define ESVIT_ATTN_CHUNK_STATS 0x%08x\n" % ops.ATTN_CHUNK_STATS in hdr and ops.ATTN_CHUNK_STATS == 0x02000000
    others = (ops.ATTN_GLOBAL, ops.ATTN_SLIDING_CHUNK, ops.ATTN_STATS, ops.ATTN_WINDOW_STATS, ops.ATTN_SPLIT_DBIAS)
    assert all(ops.ATTN_CHUNK_STATS & f == 0 for f in others) and 65535 < ops.ATTN_CHUNK_STATS < 2 ** 31
    # the forward's scratch holds the per-range partials of the mode: 24 of its 528 floats per (image, head, range)
    for L in (2, 512, 513, 12545):
        assert ops.query(ops.Q_CHUNK_ATTN_WS, 6, L, 0) >= 6 * -(-L // 512) * 24


def test_functional_falls_back_on_an_ops_module_without_the_entry():
    """oracle/ops_ref has no chunk_attn_stats: functional.vil_attention_stats reduces P of its vit_attn_fwd(chunk=), a slice of the batch
    at a time (forced to one image per slice here), and agrees with the fp64 statement.  fp32 softmax of N <= 230 terms: the entropy to
    1e-4 absolute, the rows to 1e-4 relative + 1e-7 (the figures of test_attn_stats_cpu.py for the same softmax)."""
    import esvit_amd.functional as Fn
    assert not hasattr(ops_ref, "chunk_attn_stats")
    B, nH, hd, nglo, nx, ny = 3, 2, 32, 1, 15, 8
    N, Cc, scale = nglo + nx * ny, nH * hd, hd ** -0.5
    qkv = torch.randn(B * N, 3 * Cc, generator=torch.Generator().manual_seed(5))
    queries = R.default_queries(nglo, nx, ny)
    lay = (CR.table(dict(nx=nx, ny=ny, nglo=nglo)), nglo, CR.W * ny, CR.W)
    ops_ref.set_act_dtype(torch.float32)
    old = Fn._STATS_SLICE_ELEMS
    try:
        Fn._STATS_SLICE_ELEMS = nH * N * N  # one image per slice
        ent, rows = Fn.vil_attention_stats(ops_ref, qkv, B, N, nH, scale, lay, queries)
        ent2, none = Fn.vil_attention_stats(ops_ref, qkv, B, N, nH, scale, lay[:3])
    finally:
        Fn._STATS_SLICE_ELEMS = old
    ref = R.stats64(qkv, B, nH, hd, nglo, nx, ny, scale, queries, want_bounds=False)
    assert none is None and torch.equal(ent, ent2) and ent.shape == (B, nH, N) and rows.shape == (B, nH, len(queries), N)
    assert (ent.double() - ref["ent"]).abs().max().item() <= 1e-4
    assert ((rows.double() - ref["rows"]).abs() <= 1e-4 * ref["rows"] + 1e-7).all()
    assert (rows[..., ~ref["mask"][queries]] == 0).all() and torch.equal(rows[:, :, -1], rows[:, :, -2])
    with pytest.raises(ValueError, match=r"vil_attention_stats.*\[0, 121\)"):
        Fn.vil_attention_stats(ops_ref, qkv, B, N, nH, scale, lay, [121])


# ---- the public functions on a nano MsViT ------------------------------------------------------------------------------------------
def rect_positions(model, shapes):
    """MsViT's PatchEmbed resamples its position table to square grids only.  For the rectangular images of these tests every stage gets
    the table of the crop's own grid: the leading nx x ny block of the stage's separable embedding (a test arrangement; the attention and
    everything measured here do not depend on where the table comes from)"""
    for li, layer in enumerate(model._layers()):
        pe = layer[0]
        grids = {g[0] + g[1] * g[2]: g for g in (model.feature_grid(H, W)[li] for H, W in shapes)}

        def pos(ntok, pe=pe, grids=grids):
            _, nx, ny = grids[ntok]
            g = torch.cat([pe.x_pos_embed[:, :nx].unsqueeze(2).expand(-1, -1, ny, -1), pe.y_pos_embed[:, :ny].unsqueeze(1).expand(-1, nx, -1, -1)], dim=-1)
            return torch.cat([pe.cls_pos_embed, g.flatten(start_dim=1, end_dim=2)], dim=1)
        pe.position_embedding = pos


def nano_msvit(shapes, seed=0):
    import esvit_amd
    from esvit_amd import config as CFG
    m = esvit_amd.build_model(CFG.vil_config("vil_tiny", arch=NANO_ARCH, DROP_PATH=0.0), use_dense_prediction=True)
    GU.fill_state_dict(m.state_dict(), seed)
    rect_positions(m, shapes)
    return m.eval()


def block_inputs(model, images, o):
    """the model walked as MsViT._stage walks it -> per (AttnBlock, MlpBlock) pair (qkv, nH, hd, (nglo, nx, ny), sparse): the blocks' own
    recomputed qkv.  Advances as the analysis pass does: it asks for the fused chunk route and the flash forward (where the ops module
    has them), so that both see the same block inputs"""
    import esvit_amd.functional as Fn
    from esvit_amd.models.vision_longformer import Long2DSCSelfAttention, _pair_params
    out = []
    with torch.no_grad(), Fn._long_attention("flash"):
        nB, _, H, W = images.shape
        src, nchw = images, True
        for layer, cfg in zip(model._layers(), model.layer_cfgs):
            x, nx, ny = layer[0](src, nB, H, W, nchw)
            sparse = isinstance(layer[1].attn, Long2DSCSelfAttention)
            chunk = (model._chunk_table(cfg['g'], nx, ny, cfg['f'], x.device), cfg['g'], cfg['f'] * ny, cfg['f']) if sparse else None
            for b in range(1, len(layer), 2):
                prm = _pair_params(layer[b], layer[b + 1])
                qkv = Fn._vil_block_qkv(o, x, cfg['h'], prm)[0]
                out.append((qkv, cfg['h'], cfg['d'] // cfg['h'], (cfg['g'], nx, ny), sparse))
                x = Fn.vil_block(x, cfg['h'], None, chunk, prm)
            src, H, W, nchw = x[:, cfg['g']:].contiguous(), nx, ny, False
    return out


def maps64(blocks, B, queries_of=None):
    """fp64 (entropy in nats [B, nH, N], rows of queries_of(pair) or None, mask or None) per pair from its qkv"""
    out = []
    for i, (qkv, nH, hd, (nglo, nx, ny), sparse) in enumerate(blocks):
        q = None if queries_of is None else queries_of(i)
        if sparse:
            r = R.stats64(qkv, B, nH, hd, nglo, nx, ny, hd ** -0.5, q, want_bounds=False)
            out.append((r["ent"], r.get("rows"), r["mask"]))
        else:
            ent, rows, _ = AR.stats64(qkv, B, nglo + nx * ny, nH, hd, hd ** -0.5, q)
            out.append((ent, rows, None))
    return out


def test_analysis_on_the_nano_msvit_equals_its_fp64_maps(cpu_ops):  # noqa: F811
    """attention_entropy / vil_attention_rows / vil_tokens_to_grid / feature_grid of the nano MsViT on 112 x 80 images (grids 28 x 20 and
    14 x 10 in the sliding-chunk stages: ragged chunk grids in both) in fp32 mode against fp64 maps built from the blocks' own qkv"""
    from esvit_amd import analysis as A
    shapes = ((112, 80), (64, 128))
    m = nano_msvit(shapes)
    B = 2
    x = torch.randn(B, 3, 112, 80, generator=torch.Generator().manual_seed(11))
    grids = m.feature_grid(112, 80)
    assert grids == [(1, 28, 20), (1, 14, 10), (1, 7, 5), (0, 3, 2)] and m.feature_grid(224, 224)[0] == (1, 56, 56)
    blocks = block_inputs(m, x, cpu_ops)
    assert len(blocks) == m.depth == 4 and [b[4] for b in blocks] == [True, True, False, False]
    want = maps64(blocks, B)
    ent = A.attention_entropy(m, x)
    assert isinstance(ent, list) and len(ent) == 4
    for e, (w, _, _), (nglo, nx, ny), nH in zip(ent, want, grids, (1, 3, 3, 6)):
        assert e.shape == (B, nH, nglo + nx * ny) and e.dtype == torch.float32
        assert (e.double() - w / math.log(2.0)).abs().max().item() <= 1e-4 / math.log(2.0)
    nats = A.attention_entropy(m, x, queries=[0, 5, 0], unit="nats")
    for e, (w, _, _) in zip(nats, want):
        assert e.shape[2] == 3 and (e.double() - w[..., [0, 5, 0]]).abs().max().item() <= 1e-4
    with pytest.raises(ValueError, match=r"\[0, 6\)"):  # checked per block: the last stage has six tokens
        A.attention_entropy(m, x, queries=[6])
    with pytest.raises(ValueError, match="bits or nats"):
        A.attention_entropy(m, x, unit="dits")
    with pytest.raises(TypeError, match="VisionTransformer and SwinTransformer.*MsViT"):
        A.attention_entropy(torch.nn.Linear(2, 2), x)
    # a list of two batch shapes
    x2 = torch.randn(1, 3, 64, 128, generator=torch.Generator().manual_seed(12))
    both = A.attention_entropy(m, [x, x2])
    assert len(both) == 2 and all(torch.equal(a, b) for a, b in zip(both[0], ent))
    w2 = maps64(block_inputs(m, x2, cpu_ops), 1)
    for e, (w, _, _), (nglo, nx, ny) in zip(both[1], w2, m.feature_grid(64, 128)):
        assert e.shape[2] == nglo + nx * ny and (e.double() - w / math.log(2.0)).abs().max().item() <= 1e-4 / math.log(2.0)
    # rows: pixel points and a global query, negative block indices
    pts = [(0, 0), (111, 79), (57, 30), 0, (57, 30)]
    strides = (4, 8, 16, 32)

    def tokens(i):
        nglo, nx, ny = grids[i]
        return [p if isinstance(p, int) else nglo + (p[0] // strides[i]) * ny + p[1] // strides[i] for p in pts]
    wantr = maps64(blocks, B, lambda i: tokens(i) if i < 3 else None)  # (the last point lies outside the 3 x 2 grid of stage 4)
    got = A.vil_attention_rows(m, x, pts, blocks=[1, -4, 2])
    assert len(got) == 3
    for (rows, glob), i in zip(got, (1, 0, 2)):
        nglo, nx, ny = grids[i]
        w, mask = wantr[i][1], wantr[i][2]
        assert rows.shape == (B, blocks[i][1], 5, nx, ny) and glob.shape == (B, blocks[i][1], 5, nglo) and rows.dtype == torch.float32
        flat = torch.cat([glob, rows.flatten(-2)], -1)
        assert ((flat.double() - w).abs() <= 1e-4 * w + 1e-7).all()
        assert ((rows.sum((-1, -2)) + glob.sum(-1)).double() - 1).abs().max().item() <= 1e-6
        if mask is not None:
            assert (flat[..., ~mask[tokens(i)]] == 0).all()
            assert i != 0 or (~mask[tokens(i)]).any()  # (4 x 3 chunks in stage 1: keys outside the neighbourhood exist; 2 x 2 in stage 2)
        g2, l2 = A.vil_tokens_to_grid(flat, nglo, nx, ny)
        assert torch.equal(g2, rows) and torch.equal(l2, glob)
        masks = A.attention_mass_masks(rows.flatten(-2))
        assert masks.shape == (B, blocks[i][1], 5, nx * ny) and masks.any(-1).all()
    last = A.vil_attention_rows(m, x, [(40, 40)])  # default: the last pair, which has no global token
    assert len(last) == 1 and last[0][0].shape == (B, 6, 1, 3, 2) and last[0][1].shape == (B, 6, 1, 0)
    grid, glob = A.vil_tokens_to_grid(ent[0], *grids[0])
    assert grid.shape == (B, 1, 28, 20) and glob.shape == (B, 1, 1) and torch.equal(grid.flatten(-2), ent[0][..., 1:])
    with pytest.raises(ValueError, match="vil_tokens_to_grid"):
        A.vil_tokens_to_grid(ent[0], 1, 28, 21)
    with pytest.raises(ValueError, match="outside the 28 x 20 token grid of stage 0"):
        A.vil_attention_rows(m, x, [(0, 80)], blocks=[0])
    with pytest.raises(ValueError, match="outside"):
        A.vil_attention_rows(m, x, [(-1, 0)], blocks=[0])
    with pytest.raises(ValueError, match="no global token 0"):  # stage 4 has none
        A.vil_attention_rows(m, x, [0])
    with pytest.raises(ValueError, match="no global token 1"):
        A.vil_attention_rows(m, x, [1], blocks=[0])
    with pytest.raises(ValueError, match="block indices"):
        A.vil_attention_rows(m, x, [(0, 0)], blocks=[4])
    with pytest.raises(ValueError, match="at least one point"):
        A.vil_attention_rows(m, x, [])
    with pytest.raises(TypeError, match="MsViT"):
        A.vil_attention_rows(torch.nn.Linear(2, 2), x, [(0, 0)])
    with pytest.raises(TypeError, match="VisionTransformer"):  # attention_rows stays ViT-only, swin_attention_rows Swin-only
        A.attention_rows(m, x, [0])
    with pytest.raises(TypeError, match="SwinTransformer"):
        A.swin_attention_rows(m, x, [(0, 0)])


def test_entropy_meter_on_the_nano_msvit(cpu_ops):  # noqa: F811
    """batches of unequal size and of two shapes == the per-image mean of the mean-over-queries entropy, per block pair and head"""
    from esvit_amd import analysis as A
    shapes = ((112, 80), (64, 128))
    m = nano_msvit(shapes)
    x = torch.randn(5, 3, 112, 80, generator=torch.Generator().manual_seed(21))
    x2 = torch.randn(2, 3, 64, 128, generator=torch.Generator().manual_seed(22))
    q = range(6)
    meter = A.AttentionEntropyMeter()
    for a, b in ((0, 1), (1, 4), (4, 5)):
        meter.update(m, x[a:b], queries=q)
    meter.update(m, [x2], queries=q)
    got = meter.compute()
    e1, e2 = A.attention_entropy(m, x, queries=q), A.attention_entropy(m, x2, queries=q)
    assert isinstance(got, list) and len(got) == 4 and meter.images == 7
    for g, a, b, nH in zip(got, e1, e2, (1, 3, 3, 6)):
        want = (a.double().mean(-1).sum(0) + b.double().mean(-1).sum(0)) / 7
        assert g.shape == (nH,) and g.dtype == torch.float64 and (g - want).abs().max().item() <= 1e-6
