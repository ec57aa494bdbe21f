"""-m gpu: the attention statistics kernels (csrc/flash_attn.hip: stats_entropy, stats_rows; ws = ESVIT_ATTN_GLOBAL | ESVIT_ATTN_STATS) and
esvit_amd.analysis on the MI355X, against fp64 of the same bf16 inputs (tests/attn_stats_ref.py).

The bounds (derived here, not fitted).  The existing flash test grants the fp32 scores of these kernels an error that moves the
log-sum-exp by delta = 1e-3 (1 + |lse64|) per row; take that as the bound on every score of the row, |s_k - s64_k| <= delta.
  rows     ln p_k = s_k - lse, and lse moves by at most delta when every score does: |d ln p_k| <= 2 delta, so to first order
           |p_k - p64_k| <= 2 delta p64_k, plus one fp32 ulp of 1 (2^-23) for the rounding of the stored value and of its normaliser.
  row sum  summing that over k: |sum_k p_k - 1| <= 2 delta + 2^-23 (the floor is not multiplied by N: stricter than the sum would allow).
  entropy  dH = -sum_k p_k (ln p_k + H) ds_k (the mean of ds drops out because sum_k p_k (ln p_k + H) = 0), and
           sum_k p_k |ln p_k + H| <= 2 H <= 2 ln N: |H - H64| <= 2 delta max(1, ln N).
  lse      |lse - lse64| <= delta, the flash test's own bound.
Observed fractions of each bound go to profiles/attn_stats_parity.jsonl, with the batched-GEMM route's error against the same fp64 for
context (nothing is asserted on it: it rounds the scores to bf16 before the softmax)."""
import json
import math
import os
from functools import partial

import pytest
import torch

from tests import attn_stats_ref as R
from tests import golden_utils as GU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "attn_stats_parity.jsonl")
BF = torch.bfloat16
BLOCK = R.BLOCK
ULP1 = 2.0 ** -23


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    return ops


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF).to(dev)


def _record(rec):
    print(json.dumps(rec))
    old = []
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            old = [json.loads(l) for l in f if l.strip()]
    old = [r for r in old if (r["test"], r["shape"]) != (rec["test"], rec["shape"])]
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "w") as f:
        for r in old + [rec]:
            f.write(json.dumps(r) + "\n")


def _queries(N):
    q = [t for t in (0, 15, 16, 63, 64, N - 1) if 0 <= t < N]
    q = sorted(set(q))
    return q + [q[len(q) // 2]]  # plus one duplicate


def _fractions(ent, rows, lse, ent64, rows64, lse64, N, queries):
    """observed error / derived bound, the largest over all elements -> dict (<= 1 passes)"""
    delta = 1e-3 * (1 + lse64.abs())                                    # [B, nH, N]
    dq = delta[:, :, queries].unsqueeze(-1)                             # [B, nH, nq, 1]
    rows = rows.double()
    return dict(entropy=((ent.double() - ent64).abs() / (2 * delta * max(1.0, math.log(N)))).max().item(),
                rows=((rows - rows64).abs() / (2 * dq * rows64 + ULP1)).max().item(),
                row_sum=((rows.sum(-1) - 1).abs() / (2 * dq.squeeze(-1) + ULP1)).max().item(),
                lse=((lse.double() - lse64).abs() / delta).max().item())


def _gemm_route_errors(ops, qkv, B, N, nH, scale, ent64, rows64, queries):
    """the batched-GEMM route's P (scores and P rounded to bf16) against the same fp64, for the record"""
    _, att = ops.vit_attn_fwd(qkv, B, N, nH, scale)
    p = att[-1]
    p = p.reshape(B, nH, p.shape[-2], p.shape[-1])[:, :, :N, :N].double()
    return dict(gemm_entropy_abs=(torch.special.entr(p).sum(-1) - ent64).abs().max().item(),
                gemm_rows_abs=(p[:, :, queries] - rows64).abs().max().item())


def _check(ops, test, qkv, shape, scale):
    B, N, nH, hd = shape
    queries = _queries(N)
    ent, rows, lse = ops.global_attn_stats(qkv, B, N, nH, scale, queries=queries, want_lse=True)
    assert ent.shape == (B, nH, N) and rows.shape == (B, nH, len(queries), N) and lse.shape == (B, nH, N)
    assert ent.dtype == rows.dtype == lse.dtype == torch.float32
    assert torch.isfinite(ent).all() and torch.isfinite(rows).all() and torch.isfinite(lse).all()
    assert (ent >= 0).all() and (rows >= 0).all()
    ent64, rows64, lse64 = R.stats64(qkv, B, N, nH, hd, scale, queries)
    frac = _fractions(ent, rows, lse, ent64, rows64, lse64, N, queries)
    rec = dict(test=test, shape=list(shape), **{"frac_of_bound_" + k: v for k, v in frac.items()},
               entropy_abs=(ent.double() - ent64).abs().max().item(), rows_abs=(rows.double() - rows64).abs().max().item(),
               **_gemm_route_errors(ops, qkv, B, N, nH, scale, ent64, rows64, queries))
    _record(rec)
    for k, v in frac.items():
        assert v <= 1.0, (k, rec)
    return ent, rows, lse


# (B, N, nH, hd): every boundary of the 64-token blocking, both head dims
SHAPES = [(2, 1, 2, 32), (2, 17, 3, 64), (2, 64, 3, 64), (2, 65, 3, 32), (2, 129, 2, 64), (3, 257, 1, 32), (1, 785, 3, 64)]


@pytest.mark.parametrize("shape", SHAPES)
def test_stats_match_fp64(ops, shape):
    """randn inputs: entropy, rows, row sums and lse within the bounds derived in the module docstring"""
    B, N, nH, hd = shape
    assert ops.global_attn_stats_supported(BF, hd)
    qkv = _rand((B * N, 3 * nH * hd), _dev(), 3 + sum(shape))
    ent, rows, _ = _check(ops, "parity", qkv, shape, hd ** -0.5)
    if N == 1:  # a single-token image: H = 0 and p = 1 exactly
        assert (ent == 0).all() and (rows == 1).all()


def planted(shape, dev):
    """the inputs of test_online_softmax_under_stress: qkv = 4 randn and, for four listed queries, one key whose row is 3x the query's
    row, so that the row maximum sits in the first key block, the last full block, the tail (one token at N = 65, 129, 257) and on the
    diagonal -> (qkv, [(query, key)])"""
    B, N, nH, hd = shape
    C = nH * hd
    nfull = N // BLOCK
    assert N % BLOCK != 0 and nfull >= 1
    qkv = _rand((B * N, 3 * C), dev, 50 + N, scale=4.0)
    pairs = [(15, 5),                               # (query, key): the maximum in the first key block
             (16, (nfull - 1) * BLOCK + 8),         # in the last full block
             (0, N - 1),                            # in the tail block
             (63, 63)]                              # on the diagonal
    assert len({k for _, k in pairs}) == 4
    for b in range(B):
        for q, k in pairs:
            qkv[b * N + k, C:2 * C] = 3 * qkv[b * N + q, :C]
    return qkv, pairs


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] > BLOCK and s[1] % BLOCK])
def test_stats_under_stress(ops, shape):
    """logits spread over ~ 16 and planted maxima early, late, in the tail and on the diagonal: the running maximum moves and u is
    rescaled; the same bounds (delta grows with |lse64|, as the flash test's does)"""
    B, N, nH, hd = shape
    scale = hd ** -0.5
    qkv, pairs = planted(shape, _dev())
    s = R.scores64(qkv, B, N, nH, hd, scale)
    for q, k in pairs:  # the planted keys do hold their query's maximum
        assert (s[:, :, q].argmax(-1) == k).all(), (q, k)
    _check(ops, "stress", qkv, shape, scale)


def test_images_and_heads_do_not_mix_and_the_moat_stays(ops, monkeypatch):
    """another image 1 leaves image 0's outputs bit-equal; another k of head 1 leaves heads 0 and 2 bit-equal; a NaN moat around
    attn_out and lse is intact (the outputs are carved out of larger NaN-filled buffers)"""
    dev = _dev()
    B, N, nH, hd = 2, 257, 3, 64
    C, scale, GUARD = nH * hd, hd ** -0.5, 512
    queries = _queries(N)
    qkv = _rand((B * N, 3 * C), dev, 21)
    bufs = []
    real_empty = torch.empty

    def moated(shape, **kw):
        if kw.get("dtype") != torch.float32:
            return real_empty(shape, **kw)
        n = math.prod(shape)
        buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=kw["device"])
        bufs.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def run(x):
        del bufs[:]
        monkeypatch.setattr(torch, "empty", moated)
        try:
            out = ops.global_attn_stats(x, B, N, nH, scale, queries=queries, want_lse=True)
        finally:
            monkeypatch.setattr(torch, "empty", real_empty)
        torch.cuda.synchronize()
        assert len(bufs) == 2  # attn_out (entropy | rows) and lse
        for buf, n in bufs:
            assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all() and torch.isfinite(buf[GUARD:GUARD + n]).all()
        return out
    e0, r0, l0 = run(qkv)
    x1 = qkv.clone()
    x1[N:] = _rand((N, 3 * C), dev, 23)
    e1, r1, l1 = run(x1)
    assert torch.equal(e1[0], e0[0]) and torch.equal(r1[0], r0[0]) and torch.equal(l1[0], l0[0])
    assert not torch.equal(e1[1], e0[1]) and not torch.equal(r1[1], r0[1])
    x2 = qkv.clone()
    x2[:, C + hd:C + 2 * hd] = _rand((B * N, hd), dev, 24)  # other k columns of head 1
    e2, r2, l2 = run(x2)
    for h in (0, 2):
        assert torch.equal(e2[:, h], e0[:, h]) and torch.equal(r2[:, h], r0[:, h]) and torch.equal(l2[:, h], l0[:, h])
    assert (e2[:, 1] != e0[:, 1]).all()


def test_query_list_duplicates_and_repeated_launches(ops):
    """the entropy with and without a query list is bit-equal; a duplicated query gives two bit-equal rows; ten launches give
    identical bits; 17 and 33 listed queries fill a second and a third 16-query tile"""
    dev = _dev()
    B, N, nH, hd = 2, 129, 2, 64
    scale = hd ** -0.5
    qkv = _rand((B * N, 3 * nH * hd), dev, 31)
    queries = _queries(N)
    first = ops.global_attn_stats(qkv, B, N, nH, scale, queries=queries, want_lse=True)
    dup = [i for i, q in enumerate(queries) if queries.count(q) == 2]
    assert len(dup) == 2 and torch.equal(first[1][:, :, dup[0]], first[1][:, :, dup[1]])
    e_only, none, no_lse = ops.global_attn_stats(qkv, B, N, nH, scale)
    assert none is None and no_lse is None and torch.equal(e_only, first[0])
    empty = ops.global_attn_stats(qkv, B, N, nH, scale, queries=[])
    assert empty[1].shape == (B, nH, 0, N) and torch.equal(empty[0], first[0])
    for _ in range(9):
        again = ops.global_attn_stats(qkv, B, N, nH, scale, queries=torch.tensor(queries, device=dev), want_lse=True)
        assert all(torch.equal(a, b) for a, b in zip(again, first))
    for nq in (17, 33):
        many = [(7 * i) % N for i in range(nq)]
        rows = ops.global_attn_stats(qkv, B, N, nH, scale, queries=many)[1]
        for j, q in enumerate(many):
            if q in queries:
                assert torch.equal(rows[:, :, j], first[1][:, :, queries.index(q)])
        assert ((rows.double().sum(-1) - 1).abs() < 1e-5).all()


def _vit(dev, embed, heads, patch, img, seed=0):
    from esvit_amd.models import vision_transformer as V
    m = V.VisionTransformer(img_size=[img], patch_size=patch, embed_dim=embed, depth=2, num_heads=heads, mlp_ratio=4, qkv_bias=True,
                            norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), drop_path_rate=0.0)
    GU.fill_state_dict(m.state_dict(), seed)
    return m.to(dev).eval()


def test_memory_stays_far_below_one_score_tensor(lib_built):
    """attention_entropy of a 2-block ViT at N = 1601 (320^2 at patch 8), B = 1, nH = 6: the peak allocation above the live inputs stays
    under a quarter of ONE fp32 score tensor (nH N^2 4 B / 4 = 15.4 MB; forward_selfattention holds at least one per block)"""
    import esvit_amd
    from esvit_amd import analysis as A
    dev = _dev()
    esvit_amd.set_precision("bf16")
    try:
        m = _vit(dev, 192, 6, 8, 320)
        x = torch.randn(1, 3, 320, 320, generator=torch.Generator().manual_seed(4)).to(dev)
        A.attention_entropy(m, x)  # (weights cast, the library's shared scratch sized for these GEMMs before the measurement)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ent = A.attention_entropy(m, x)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    finally:
        esvit_amd.set_precision("fp32")
    one_score_tensor = 6 * 1601 * 1601 * 4
    print(json.dumps(dict(test="memory", shape=[1, 1601, 6, 32], peak_above_inputs_MB=peak / 1e6, one_score_tensor_MB=one_score_tensor / 1e6)))
    assert ent.shape == (2, 1, 6, 1601) and torch.isfinite(ent).all()
    assert peak < one_score_tensor / 4, (peak, one_score_tensor / 4)


@pytest.mark.parametrize("img,N", [(64, 65), (128, 257)])
def test_vit_analysis_matches_fp64_and_the_attention_maps(lib_built, img, N):
    """a 2-block patch-8 ViT of deit_tiny's width (192, 3 heads of 64) in bf16.  attention_entropy / attention_rows against the fp64
    statement on the same blocks' qkv (recomputed with the same kernels: the bounds of the module docstring), and against
    forward_selfattention(n=2), whose route rounds the unscaled scores and P to bf16 (relative 2^-9 each): its score error is
    delta_g = 2^-9 max_k |s64_k| per row (not small: the exact form e^(2 delta_g) - 1 is kept for it), so its rows are off by
    (e^(2 delta_g) - 1 + 2^-9) p64 and its entropy by
    2 delta_g max(1, ln N) + 2^-9 (ln N + 1)  (dH = -sum dp (ln p + 1) with |dp| <= 2^-9 p).  The two routes are compared at the sum of
    both routes' bounds."""
    import esvit_amd
    import esvit_amd.functional as Fn
    from esvit_amd import analysis as A
    dev = _dev()
    esvit_amd.set_precision("bf16")
    try:
        m = _vit(dev, 192, 3, 8, img)
        nH, hd = 3, 64
        x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(img)).to(dev)
        queries = _queries(N)
        ent = A.attention_entropy(m, x, unit="nats")
        bits = A.attention_entropy(m, x, queries=queries)
        rows = A.attention_rows(m, x, queries, blocks=[0, 1])
        assert ent.shape == (2, 2, nH, N) and rows.shape == (2, 2, nH, len(queries), N)
        assert torch.allclose(bits, ent[..., queries] / math.log(2.0), rtol=1e-6, atol=0)
        assert torch.equal(A.attention_rows(m, x, queries)[0], rows[1])
        # (the analysis advances through the blocks on the flash forward beyond 224 tokens: so do the maps and this pass, so that all
        # three see the same block inputs; the maps themselves are the batched-GEMM route's P whatever the route of the advance)
        with torch.no_grad(), Fn._long_attention("flash"):
            maps = m.forward_selfattention(x, n=2)
            t = m._tokens(x)
            o = Fn.ops_module()
            for i, blk in enumerate(m.blocks):
                g1, b1, Wqkv, bqkv = blk._params()[:4]
                qkv = o.linear_fwd(o.layernorm_fwd(t.contiguous().view(2 * N, 192), g1, b1, Fn.LN_EPS)[0], Fn._weight(Wqkv), bqkv)
                assert qkv.dtype == BF
                ent64, rows64, lse64 = R.stats64(qkv, 2, N, nH, hd, hd ** -0.5, queries)
                frac = _fractions(ent[i], rows[i], lse64, ent64, rows64, lse64, N, queries)
                smax = R.scores64(qkv, 2, N, nH, hd, hd ** -0.5).abs().max(-1).values
                delta, dg = 1e-3 * (1 + lse64.abs()), 2.0 ** -9 * smax
                lnN = max(1.0, math.log(N))
                p = maps[i].double()
                ent_tol = 2 * (delta + dg) * lnN + 2.0 ** -9 * (math.log(N) + 1)
                dq, dgq = delta[:, :, queries].unsqueeze(-1), dg[:, :, queries].unsqueeze(-1)
                row_tol = (2 * dq + torch.expm1(2 * dgq) + 2.0 ** -9) * rows64 + ULP1
                vs_maps = dict(entropy=((ent[i].double() - torch.special.entr(p).sum(-1)).abs() / ent_tol).max().item(),
                               rows=((rows[i].double() - p[:, :, queries]).abs() / row_tol).max().item())
                _record(dict(test="vit_block%d" % i, shape=[2, N, nH, hd], **{"frac_of_bound_" + k: v for k, v in frac.items() if k != "lse"},
                             **{"frac_of_maps_bound_" + k: v for k, v in vs_maps.items()}))
                assert frac["entropy"] <= 1 and frac["rows"] <= 1 and frac["row_sum"] <= 1, frac
                assert vs_maps["entropy"] <= 1 and vs_maps["rows"] <= 1, vs_maps
                t = blk(t)
    finally:
        esvit_amd.set_precision("fp32")


def test_swin_entropy_is_the_reduction_of_its_own_maps(lib_built):
    import esvit_amd
    from esvit_amd import analysis as A
    from tests.test_composition_cpu import build_nano
    dev = _dev()
    esvit_amd.set_precision("bf16")
    try:
        m = build_nano()
        GU.fill_state_dict(m.state_dict(), 0)
        m = m.to(dev).eval()
        x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(9)).to(dev)
        ent = A.attention_entropy(m, x, queries=range(49))
        with torch.no_grad():
            maps = m.forward_selfattention(x, n=2)
        assert len(ent) == len(maps) == sum(GU.NANO["depths"])
        for e, p in zip(ent, maps):
            assert e.shape == p.shape[:3] and torch.equal(e, torch.special.entr(p.float()).sum(-1) / math.log(2.0))
        per = A.AttentionEntropyMeter().update(m, x).compute()
        assert [tuple(t.shape) for t in per] == [(p.shape[1],) for p in maps]
        with pytest.raises(TypeError, match="VisionTransformer"):
            A.attention_rows(m, x, [0])
    finally:
        esvit_amd.set_precision("fp32")


@pytest.mark.parametrize("grid", [(7, 7), (14, 14)])
@pytest.mark.parametrize("kind", ["mirror", "random", "ties"])
def test_correspondence_scores_on_the_device(lib_built, kind, grid):
    """the library's l2-norm and batched GEMM against the per-image restatement in fp64: similarities at the fp32 GEMM bound (C = 24
    products of unit-norm rows, each factor rounded once: (C + 2) 2^-24 < 2e-6 of a cosine <= 1; 1e-5 granted as on the CPU), accuracy and
    distance on every input kind (they are functions of the matches and the ranking of the `top` rows: a wrong first arg-max index or
    an unstable ranking on the tie inputs, whose similarities are exactly 0 or 1, changes them)"""
    from esvit_amd import analysis as A
    from tests.test_attn_stats_cpu import _corr_inputs
    dev = _dev()
    gh, gw = grid
    T, cell = gh * gw, 16
    fea1, fea2 = _corr_inputs(kind, gh, gw)
    for flipped, top in ((True, 10), (False, 3)):
        if kind == "mirror" and not flipped:
            continue
        acc, err, sims = A.correspondence_scores(fea1.to(dev), fea2.to(dev), grid, cell, top=top, flipped=flipped)
        for b in range(3):
            racc, rerr, rsims, _ = R.correspondence_ref(fea1[b], fea2[b], grid, cell, top=top, flipped=flipped)
            assert (sims[b].double().cpu() - torch.tensor(rsims)).abs().max().item() <= 1e-5
            assert abs(acc[b].item() - racc) <= 1e-6 and abs(err[b].item() - rerr) <= 1e-4 * (1 + rerr), (kind, b, acc[b], racc, err[b], rerr)
            if kind == "mirror":
                assert acc[b].item() == 1.0 and err[b].item() == 0.0
            if kind == "ties":
                assert torch.equal(sims[b].cpu(), torch.ones(T))
