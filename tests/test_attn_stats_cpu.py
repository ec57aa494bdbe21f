"""-m "not gpu": the attention statistics (entropy of every softmax row, probability rows of listed queries; the mode
ESVIT_ATTN_GLOBAL | ESVIT_ATTN_STATS of esvit_window_attn_fwd) and esvit_amd.analysis without a GPU -- the online recurrence of the
entropy kernel in fp64, the argument checks of the C entry, the fall-back of functional.vit_attention_stats on an ops module without
the entry, and the public functions on the torch restatement of every kernel."""
import ctypes as C
import math
import os

import pytest
import torch

from oracle import ops_ref
from tests import attn_stats_ref as R
from tests import golden_utils as GU
from tests.test_composition_cpu import cpu_ops  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N", [1, 17, 64, 65, 129, 257])
def test_blocked_recurrence_equals_direct_entropy(N):
    """the u recurrence over 64-key blocks against sum -p ln p in fp64, to 1e-12: random rows, a row whose maximum sits in the last
    block (every earlier block is rescaled when it arrives), and a one-hot row (H = 0 exactly, no NaN)"""
    g = torch.Generator().manual_seed(N)
    s = 4 * torch.randn(6, N, generator=g, dtype=torch.float64)
    s[1, N - 1] = s[1].max() + 9.0   # the maximum in the last block (N = 65, 129, 257: the one-token tail)
    s[2, :] = 0.0
    s[2, N // 2] = 2000.0            # one-hot after the softmax: every other e^(s - m) underflows to 0
    s[3, 0] = s[3].max() + 30.0      # the maximum in the first block
    s[4, :] = 1.25                   # uniform: H = ln N
    ent, _, lse = R.stats_of_scores64(s)
    got, got_lse = R.blocked_entropy64(s)
    assert torch.isfinite(got).all()
    assert (got - ent).abs().max().item() <= 1e-12, (got - ent).abs().max().item()
    assert (got_lse - lse).abs().max().item() <= 1e-12 * (1 + lse.abs().max().item())
    assert got[2].item() == 0.0 and ent[2].item() == 0.0
    assert abs(got[4].item() - math.log(N)) <= 1e-12


def test_stats_mode_is_refused_where_it_must_be(lib_built):
    """one rejection per argument check of the mode, ESVIT_ERR_ARG before any launch (a launch on this GPU-less host would come back as
    ESVIT_ERR_HIP), the cause in esvit_last_error()"""
    from esvit_amd import _lib, ops
    lib = _lib.lib
    fake = C.c_void_p(0x1000)  # never dereferenced: the argument checks come first
    G, S, K = ops.ATTN_GLOBAL, ops.ATTN_STATS, ops.ATTN_SLIDING_CHUNK

    def fwd(dtype=ops.BF16, hd=64, L=785, ws=G | S, out=None, attn=fake, nW=3, q=fake, bias=None, frag=None):
        rc = lib.esvit_window_attn_fwd(dtype, fake, bias, q, L, None, ws, frag, None, nW, 2, L, 3, hd, 0.125, out, None, attn, None)
        return rc, lib.esvit_last_error()

    def bwd(ws):
        rc = lib.esvit_window_attn_bwd(ops.BF16, fake, None, None, 785, fake, fake, fake, None, ws, fake, None, 1, 2, 785, 3, 64, 0.125, fake,
                                       None, None, None)
        return rc, lib.esvit_last_error()
    for got, cause in ((fwd(ws=S), b"only together with ESVIT_ATTN_GLOBAL"),        # the stats flag without the global flag
                       (fwd(ws=S | 7), b"only together with ESVIT_ATTN_GLOBAL"),    # ... on a window side
                       (bwd(G | S), b"esvit_window_attn_fwd only"),                 # in the backward entry
                       (bwd(S | 7), b"only together with ESVIT_ATTN_GLOBAL"),
                       (fwd(ws=G | S | K), b"both mode flags"),                     # together with the sliding-chunk flag
                       (bwd(G | S | K), b"both mode flags"),
                       (fwd(ws=G | S | 7), b"mode flags alone"),
                       (fwd(out=fake), b"out must be NULL"),
                       (fwd(attn=None), b"attn_out"),
                       (fwd(nW=0), b"nW=0"),
                       (fwd(dtype=ops.F32), b"bf16"),
                       (fwd(hd=48), b"head_dim 48"),
                       (fwd(q=None), b"win2tok"),                                   # listed queries without the list
                       (fwd(bias=fake), b"pass NULL"),
                       (fwd(frag=fake), b"pass NULL"),
                       (fwd(L=0), b"L=0")):
        assert got[0] == -1 and cause in got[1], (got, cause)
    # the plain global mode keeps its own checks: attn_out is still refused there
    rc = lib.esvit_window_attn_fwd(ops.BF16, fake, None, None, 785, None, G, None, None, 1, 2, 785, 3, 64, 0.125, fake, fake, fake, None)
    assert rc == -1 and b"attn_out is not available" in lib.esvit_last_error()
    assert ops.global_attn_stats_supported(torch.bfloat16, 32) and ops.global_attn_stats_supported(torch.bfloat16, 64)
    assert not ops.global_attn_stats_supported(torch.float32, 64) and not ops.global_attn_stats_supported(torch.bfloat16, 48)
    # the query list is checked on the host, before the library is called (which cannot read the array)
    qkv = torch.zeros(2 * 5, 3 * 64, dtype=torch.bfloat16)
    for bad in ([0, 5], [-1], torch.tensor([1, 7])):
        with pytest.raises(ValueError, match=r"\[0, 5\)"):
            ops.global_attn_stats(qkv, 2, 5, 2, 0.2, queries=bad)


def test_header_constants_equal_ops_constants(lib_built):
    from esvit_amd import ops
    hdr = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "#define ESVIT_ATTN_STATS 0x%08x\n" % ops.ATTN_STATS in hdr
    assert "#define ESVIT_ATTN_GLOBAL 0x%x" % ops.ATTN_GLOBAL in hdr
    others = (ops.ATTN_GLOBAL, ops.ATTN_SLIDING_CHUNK, 0x10000000)  # (ESVIT_ATTN_SPLIT_DBIAS)
    assert "#define ESVIT_ATTN_SPLIT_DBIAS 0x%x" % others[2] in hdr
    assert all(ops.ATTN_STATS & f == 0 for f in others) and 224 < ops.ATTN_STATS < 2 ** 31


def test_functional_falls_back_on_an_ops_module_without_the_entry():
    """oracle/ops_ref has no global_attn_stats: functional.vit_attention_stats reduces P of its vit_attn_fwd, a slice of the batch at a
    time (forced to one image per slice here), and agrees with the fp64 statement.  fp32 softmax of N <= 230 terms: the entropy to
    1e-4 absolute, the rows to 1e-4 relative + 1e-7."""
    import esvit_amd.functional as Fn
    assert not hasattr(ops_ref, "global_attn_stats")
    B, N, nH, hd = 3, 230, 2, 32
    Cc, scale = nH * hd, hd ** -0.5
    qkv = torch.randn(B * N, 3 * Cc, generator=torch.Generator().manual_seed(5))
    queries = [0, 15, 229, 15]
    ops_ref.set_act_dtype(torch.float32)
    old = Fn._STATS_SLICE_ELEMS
    try:
        Fn._STATS_SLICE_ELEMS = nH * N * N  # one image per slice
        ent, rows = Fn.vit_attention_stats(ops_ref, qkv, B, N, nH, scale, queries)
        ent2, none = Fn.vit_attention_stats(ops_ref, qkv, B, N, nH, scale)
    finally:
        Fn._STATS_SLICE_ELEMS = old
    ent64, rows64, _ = R.stats64(qkv, B, N, nH, hd, scale, queries)
    assert none is None and torch.equal(ent, ent2) and ent.shape == (B, nH, N) and rows.shape == (B, nH, 4, N)
    assert (ent.double() - ent64).abs().max().item() <= 1e-4
    assert ((rows.double() - rows64).abs() <= 1e-4 * rows64 + 1e-7).all()
    assert torch.equal(rows[:, :, 1], rows[:, :, 3])
    with pytest.raises(ValueError, match=r"\[0, 230\)"):
        Fn.vit_attention_stats(ops_ref, qkv, B, N, nH, scale, [230])


def _nano_vit():
    from tests.test_vit_cpu import build_nano_vit
    m = build_nano_vit()
    GU.fill_state_dict(m.state_dict(), 0)
    return m.eval()


def _images(B, size, seed):
    return torch.randn(B, 3, size, size, generator=torch.Generator().manual_seed(seed))


def test_analysis_on_the_nano_vit_equals_its_attention_maps(cpu_ops):  # noqa: F811
    """attention_entropy / attention_rows of the nano ViT (17 tokens at 64^2, 5 at 32^2) in fp32 mode against the entropy and the rows of
    forward_selfattention(n=2)'s maps: the same probabilities by the same route here, so 1e-6"""
    from esvit_amd import analysis as A
    m = _nano_vit()
    for size, N in ((64, 17), (32, 5)):
        x = _images(3, size, 11)
        with torch.no_grad():
            maps = torch.stack(m.forward_selfattention(x, n=2)).double()
        assert maps.shape == (2, 3, 2, N, N)
        want_bits = torch.special.entr(maps).sum(-1) / math.log(2.0)
        ent = A.attention_entropy(m, x)
        assert ent.shape == (2, 3, 2, N) and ent.dtype == torch.float32
        assert (ent.double() - want_bits).abs().max().item() <= 1e-6
        nats = A.attention_entropy(m, x, queries=[0, N - 1, 0], unit="nats")
        assert nats.shape == (2, 3, 2, 3)
        assert (nats.double() - torch.special.entr(maps).sum(-1)[..., [0, N - 1, 0]]).abs().max().item() <= 1e-6
        q = [0, 3, N - 1, 3]
        rows = A.attention_rows(m, x, q)
        assert rows.shape == (1, 3, 2, 4, N) and rows.dtype == torch.float32
        assert (rows[0].double() - maps[1][:, :, q]).abs().max().item() <= 1e-6
        rows = A.attention_rows(m, x, q, blocks=[1, 0, -1])
        assert rows.shape == (3, 3, 2, 4, N)
        assert (rows.double() - maps[[1, 0, 1]][:, :, :, q]).abs().max().item() <= 1e-6
    with pytest.raises(ValueError, match="bits or nats"):
        A.attention_entropy(m, x, unit="dits")
    with pytest.raises(ValueError, match=r"\[0, 5\)"):
        A.attention_entropy(m, x, queries=[5])
    with pytest.raises(TypeError, match="VisionTransformer and SwinTransformer"):
        A.attention_entropy(torch.nn.Linear(2, 2), x)
    with pytest.raises(TypeError, match="VisionTransformer"):
        A.attention_rows(torch.nn.Linear(2, 2), x, [0])


def test_attention_mass_masks_equal_a_per_row_loop():
    """the reference's steps on one row at a time (ascending sort, normalise, cumulative sum, keep cumsum > 1 - threshold, un-sort)"""
    from esvit_amd import analysis as A
    g = torch.Generator().manual_seed(2)
    rows = torch.softmax(3 * torch.randn(2, 3, 4, 50, generator=g), -1)
    rows[0, 0, 0] = 0
    rows[0, 0, 0, 7] = 1.0  # a one-hot row keeps that entry only
    for th in (0.6, 0.9):
        got = A.attention_mass_masks(rows, th)
        assert got.dtype == torch.bool and got.shape == rows.shape
        for r, gr in zip(rows.reshape(-1, 50), got.reshape(-1, 50)):
            val, idx = torch.sort(r)
            val = val / val.sum()
            keep = torch.cumsum(val, 0) > (1 - th)
            want = keep[torch.argsort(idx)]
            assert torch.equal(gr, want)
        assert got[0, 0, 0].nonzero().flatten().tolist() == [7]
        kept = (rows * got).sum(-1)
        assert (kept >= th - 1e-5).all()


def test_entropy_meter_equals_the_mean_at_once_and_the_running_mean(cpu_ops):  # noqa: F811
    from esvit_amd import analysis as A
    m = _nano_vit()
    x = _images(6, 64, 21)
    q = range(9)
    # three batches of unequal size == all six images at once
    meter = A.AttentionEntropyMeter()
    for a, b in ((0, 1), (1, 4), (4, 6)):
        meter.update(m, x[a:b], queries=q)
    got = meter.compute()
    want = A.attention_entropy(m, x, queries=q).double().mean(-1).mean(1)
    assert got.shape == (2, 2) and got.dtype == torch.float64
    assert (got - want).abs().max().item() <= 1e-6
    # batch 1 through an iterable of (images, target): the reference's running mean of the mean over the queries of -p log2 p
    meter = A.AttentionEntropyMeter().update_from(m, [(x[i:i + 1], torch.zeros(1)) for i in range(6)], queries=q)
    avg, count = [None, None], 0.0
    for i in range(6):
        with torch.no_grad():
            maps = m.forward_selfattention(x[i:i + 1], n=2)
        count += 1.0
        for blk, attn in enumerate(maps):
            acc = 0
            for query in q:
                p = attn[0, :, query, :].double()
                acc = acc + (-p * torch.log2(p)).sum(-1)
            acc = acc / len(q)
            avg[blk] = acc if count < 2 else (acc + (count - 1.0) * avg[blk]) / count
    assert (meter.compute() - torch.stack(avg)).abs().max().item() <= 1e-6
    with pytest.raises(RuntimeError, match="no update"):
        A.AttentionEntropyMeter().compute()


def _corr_inputs(kind, gh, gw, B=3, C=24, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * gh)
    T = gh * gw
    fea1 = torch.randn(B, T, C, generator=g)
    if kind == "mirror":
        fea2 = fea1.view(B, gh, gw, C).flip(2).reshape(B, T, C).clone()
    elif kind == "random":
        fea2 = torch.randn(B, T, C, generator=g)
    else:  # "ties": one-hot features -> similarities exactly 0 or 1; every token of view 1 finds several exact maxima, all rows tie
        assert C >= 4
        fea1 = torch.nn.functional.one_hot(torch.randint(0, 4, (B, T), generator=g), C).float()
        fea2 = torch.nn.functional.one_hot(torch.randint(0, 4, (B, T), generator=g), C).float()
    return fea1, fea2


@pytest.mark.parametrize("grid", [(7, 7), (14, 14)])
@pytest.mark.parametrize("kind", ["mirror", "random", "ties"])
def test_correspondence_scores_equal_the_per_image_restatement(cpu_ops, kind, grid):  # noqa: F811
    """(i) the exact mirror -> accuracy 1, distance 0; (ii) random features; (iii) exact ties (similarities are 0 or 1 exactly: first
    arg-max index, stable ranking).  Similarities to the fp32 rounding of a cosine (1e-5); the matches and the ranking through accuracy
    and distance over the `top` rows, which are functions of both (the random inputs have no near-ties among their row maxima)."""
    from esvit_amd import analysis as A
    gh, gw = grid
    T, cell = gh * gw, 16
    fea1, fea2 = _corr_inputs(kind, gh, gw)
    for flipped, top in ((True, 10), (False, 3), (True, T + 5)):
        if kind == "mirror" and not flipped:
            continue  # (every best similarity is 1 up to rounding there: the ranking is a matter of the last bit, the distances are not 0)
        acc, err, sims = A.correspondence_scores(fea1, fea2, grid, cell, top=top, flipped=flipped)
        assert acc.shape == (3,) and err.shape == (3,) and sims.shape == (3, T)
        for b in range(3):
            racc, rerr, rsims, _ = R.correspondence_ref(fea1[b], fea2[b], grid, cell, top=top, flipped=flipped)
            assert (sims[b].double() - torch.tensor(rsims)).abs().max().item() <= 1e-5
            assert abs(acc[b].item() - racc) <= 1e-6 and abs(err[b].item() - rerr) <= 1e-4 * (1 + rerr), (kind, b, acc[b], racc, err[b], rerr)
            if kind == "mirror" and flipped:
                assert acc[b].item() == 1.0 and err[b].item() == 0.0
            if kind == "ties":
                assert set(rsims) == {1.0} and torch.equal(sims[b], torch.ones(T))
