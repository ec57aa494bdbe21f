"""-m gpu: the fused sliding-chunk attention kernels (csrc/chunk_attn.hip, the sliding-chunk mode of esvit_window_attn_fwd / _bwd)
against the restatement of the dense route (oracle/ops_ref.vit_attn_fwd / _bwd with the chunk mask), exact neighbourhood properties,
the memory bound that is the point of the kernels, and the Vision Longformer models with CHUNK_ATTENTION = "fused"."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import golden_utils as GU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "chunk_attn_parity.jsonl")
BF = torch.bfloat16


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mods(lib_built):
    from esvit_amd import ops
    from oracle import ops_ref
    return ops, ops_ref


def _rand(shape, dev, seed, dt=BF, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dt)


def _table(nglo, nx, ny, w, dev):
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return torch.from_numpy(np.concatenate([np.full(nglo, -1), ((ix // w) << 16 | (iy // w)).reshape(-1)]).astype(np.int32)).to(dev)


def _rel(got, ref):
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert math.isfinite(err), "non-finite output"
    return err / (ref.abs().max().item() + 1e-12)


# the four cases of tests/test_kernels_gpu.py::test_sliding_chunk_attention, then the 96^2 crop's first stage at head_dim 48, a grid
# smaller than one chunk, a grid that is neither square nor a multiple of 7 with two globals at head_dim 64, and a ragged narrow one
CASES = [((28, 28), 7, 1, 48), ((12, 12), 7, 1, 32), ((14, 14), 7, 2, 64), ((56, 56), 7, 1, 48),
         ((24, 24), 7, 1, 48), ((5, 5), 7, 1, 32), ((21, 35), 7, 2, 64), ((8, 15), 7, 1, 32)]


@pytest.mark.parametrize("grid,w,nglo,hd", CASES)
def test_fused_sliding_chunk_attention_matches_restatement(mods, grid, w, nglo, hd):
    """forward and backward of the fused kernels vs ops_ref.vit_attn_fwd / _bwd(chunk=...) at the bf16 tolerances of
    test_sliding_chunk_attention (out 2e-2, dqkv 3e-2 of the reference's largest magnitude); the error of BOTH routes against the fp32
    evaluation of the same bf16 inputs goes to profiles/chunk_attn_parity.jsonl"""
    ops, ref = mods
    dev = _dev()
    nx, ny = grid
    N, B, nH = nglo + nx * ny, 2, 2
    tab = _table(nglo, nx, ny, w, dev)
    lay = (tab, nglo, w * ny)
    assert ops.sliding_chunk_attn_supported(BF, hd, w, nglo)
    qkv = _rand((B * N, 3 * nH * hd), dev, 90)
    dout = _rand((B * N, nH * hd), dev, 91)
    scale = hd ** -0.5
    out, saved = ops.sliding_chunk_attn_fwd(qkv, B, N, nH, scale, lay)
    dq = ops.sliding_chunk_attn_bwd(dout, saved, B, N, nH, scale, lay)
    outr, savedr = ref.vit_attn_fwd(qkv, B, N, nH, scale, chunk=tab)
    dqr = ref.vit_attn_bwd(dout, savedr, B, N, nH, scale)
    # fp32 evaluation of the same bf16 inputs, and the dense route of the library
    out32, saved32 = ref.vit_attn_fwd(qkv.float(), B, N, nH, scale, chunk=tab)
    dq32 = ref.vit_attn_bwd(dout.float(), saved32, B, N, nH, scale)
    outd, savedd = ops.vit_attn_fwd(qkv, B, N, nH, scale, chunk=lay)
    dqd = ops.vit_attn_bwd(dout, savedd, B, N, nH, scale, chunk=lay)
    lse32 = torch.logsumexp((scale * (saved32[0][0] @ saved32[0][1].transpose(-2, -1))).masked_fill(~ref.chunk_mask(tab).to(dev), float("-inf")), -1)
    rec = dict(grid=list(grid), w=w, nglo=nglo, hd=hd, B=B, nH=nH,
               fused_out_vs_fp32=_rel(out, out32), dense_out_vs_fp32=_rel(outd, out32),
               fused_dqkv_vs_fp32=_rel(dq, dq32), dense_dqkv_vs_fp32=_rel(dqd, dq32),
               fused_out_vs_restatement=_rel(out, outr), fused_dqkv_vs_restatement=_rel(dq, dqr),
               fused_lse_abs_vs_fp32=(saved[2] - lse32).abs().max().item())
    print(json.dumps(rec))
    old = []
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            old = [json.loads(l) for l in f if l.strip()]
    old = [r for r in old if (r["grid"], r["nglo"], r["hd"]) != (rec["grid"], rec["nglo"], rec["hd"])]
    with open(PARITY, "w") as f:
        for r in old + [rec]:
            f.write(json.dumps(r) + "\n")
    assert rec["fused_out_vs_restatement"] <= 2e-2, rec
    assert rec["fused_dqkv_vs_restatement"] <= 3e-2, rec


def test_neighbourhood_is_exact(mods):
    """tolerance 0: what a local query cannot see does not reach it, what it can see does; every token reaches every global row;
    a key receives exactly nothing from queries that cannot see it; two launches give the same bits"""
    ops, ref = mods
    dev = _dev()
    nx = ny = 28
    nglo, w, hd, B, nH = 1, 7, 32, 1, 2
    N, C = nglo + nx * ny, nH * hd
    tab = _table(nglo, nx, ny, w, dev)
    lay = (tab, nglo, w * ny)
    mask = ref.chunk_mask(tab).to(dev)
    scale = hd ** -0.5
    qkv = _rand((B * N, 3 * C), dev, 5)
    out, saved = ops.sliding_chunk_attn_fwd(qkv, B, N, nH, scale, lay)
    tok = lambda x, y: nglo + x * ny + y  # noqa: E731
    qi = tok(10, 10)  # chunk (1, 1): sees x, y < 21
    unseen = ~mask[qi]
    assert unseen.sum().item() == nx * ny - 21 * 21 and not mask[qi, tok(25, 25)] and mask[qi, tok(20, 20)] and mask[qi, 0]
    q2 = qkv.clone()
    q2[unseen, C:] = _rand((int(unseen.sum().item()), 2 * C), dev, 6)  # k and v of everything the query cannot see
    out2, _ = ops.sliding_chunk_attn_fwd(q2, B, N, nH, scale, lay)
    assert torch.equal(out2[qi], out[qi])
    assert not torch.equal(out2[0], out[0])  # the global row sees them
    q3 = qkv.clone()
    q3[tok(20, 20), C:] += 1.0
    out3, _ = ops.sliding_chunk_attn_fwd(q3, B, N, nH, scale, lay)
    assert not torch.equal(out3[qi], out[qi])
    for t in (0, tok(0, 0), tok(13, 27), tok(27, 27)):  # any token moves every global row
        q4 = qkv.clone()
        q4[t, C:] += 1.0
        out4, _ = ops.sliding_chunk_attn_fwd(q4, B, N, nH, scale, lay)
        assert not torch.equal(out4[:nglo], out[:nglo]), t
    # backward: gradient only on queries that cannot see key j
    j = tok(25, 25)
    dout = _rand((B * N, C), dev, 7)
    dout[mask[:, j]] = 0
    assert (dout.abs().sum(1) > 0).sum().item() == N - int(mask[:, j].sum().item()) > 0
    dq = ops.sliding_chunk_attn_bwd(dout, saved, B, N, nH, scale, lay)
    assert (dq[j, C:] == 0).all()
    assert (dq[tok(0, 0), C:] != 0).any()
    # reproducible to the bit
    dfull = _rand((B * N, C), dev, 8)
    o_a, s_a = ops.sliding_chunk_attn_fwd(qkv, B, N, nH, scale, lay)
    o_b, s_b = ops.sliding_chunk_attn_fwd(qkv, B, N, nH, scale, lay)
    assert torch.equal(o_a, o_b) and torch.equal(s_a[2], s_b[2])
    assert torch.equal(ops.sliding_chunk_attn_bwd(dfull, s_a, B, N, nH, scale, lay), ops.sliding_chunk_attn_bwd(dfull, s_b, B, N, nH, scale, lay))


def test_memory_is_linear_in_tokens(mods):
    """vil_small's first stage at 448^2 (112 x 112 grid, head_dim 32, 3 heads, B = 2), forward + backward: the peak above the live
    inputs stays below 1/16 of ONE dense score tensor (B nH N^2 2 B / 16 = 118 MB; the dense route holds two of 1.9 GB), and the
    results agree with the dense route at the tolerances of the kernel test"""
    ops, ref = mods
    dev = _dev()
    nx = ny = 112
    nglo, w, hd, B, nH = 1, 7, 32, 2, 3
    N, C = nglo + nx * ny, nH * hd
    tab = _table(nglo, nx, ny, w, dev)
    lay = (tab, nglo, w * ny)
    scale = hd ** -0.5
    qkv = _rand((B * N, 3 * C), dev, 11)
    dout = _rand((B * N, C), dev, 12)
    ops.sliding_chunk_attn_fwd(qkv[:2 * (nglo + 49)], 2, nglo + 49, nH, scale, (_table(nglo, 7, 7, w, dev), nglo, w * 7))  # (the shared scratch exists before the measurement)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, saved = ops.sliding_chunk_attn_fwd(qkv, B, N, nH, scale, lay)
    dq = ops.sliding_chunk_attn_bwd(dout, saved, B, N, nH, scale, lay)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    dense_scores = B * nH * N * N * 2
    print(json.dumps(dict(test="memory", peak_above_inputs_MB=peak / 1e6, one_dense_score_tensor_MB=dense_scores / 1e6)))
    assert peak < dense_scores / 16, (peak, dense_scores / 16)
    outd, savedd = ops.vit_attn_fwd(qkv, B, N, nH, scale, chunk=lay)
    dqd = ops.vit_attn_bwd(dout, savedd, B, N, nH, scale, chunk=lay)
    assert _rel(out, outd) <= 2e-2 and _rel(dq, dqd) <= 3e-2, (_rel(out, outd), _rel(dq, dqd))


def _spy(monkeypatch, ops):
    calls = {"fwd": 0, "bwd": 0}
    f0, b0 = ops.sliding_chunk_attn_fwd, ops.sliding_chunk_attn_bwd
    monkeypatch.setattr(ops, "sliding_chunk_attn_fwd", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), f0(*a, **k))[1])
    monkeypatch.setattr(ops, "sliding_chunk_attn_bwd", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), b0(*a, **k))[1])
    return calls


@pytest.mark.parametrize("name", ["vil_tiny_k8192_b2", "vil_small_k8192_b2"])
def test_vil_full_width_fused_matches_reference_golden(name, lib_built, monkeypatch):
    """the Vision Longformer step with CHUNK_ATTENTION = "fused" against the reference's fixture, within the bounds the dense route has"""
    from esvit_amd import ops
    from esvit_amd.models import vision_longformer as vil
    from tests.test_step_gpu import FULL_VIL_BF16_BOUNDS, _setup, _teardown, check_full_vil_case
    dev = _setup("bf16")
    try:
        monkeypatch.setattr(vil, "CHUNK_ATTENTION", "fused")
        calls = _spy(monkeypatch, ops)
        check_full_vil_case(name, dev, False, FULL_VIL_BF16_BOUNDS[name], record="bf16-fused")
        assert calls["fwd"] > 0 and calls["bwd"] > 0, calls
    finally:
        _teardown()


def test_vil_routes_agree(lib_built, monkeypatch):
    """forward_return_n_last_blocks of the two routes agree, and three trainer steps of vil_tiny at B = 16 give finite losses whose
    first agrees with the dense route's within the loss bound of the fixture comparison"""
    import bench
    import esvit_amd
    from esvit_amd import ops
    from esvit_amd.engine import EsvitTrainer
    from esvit_amd.models import vision_longformer as vil
    from tests.test_step_gpu import FULL_VIL_BF16_BOUNDS, _setup, _teardown
    dev = _setup("bf16")
    calls = _spy(monkeypatch, ops)
    res, feats = {}, {}
    try:
        for route in ("dense", "fused"):
            monkeypatch.setattr(vil, "CHUNK_ATTENTION", route)
            torch.manual_seed(0)
            student, teacher, loss_fn = bench.build(dev, 0.0, "vil_tiny")
            student.eval()
            with torch.no_grad():
                crop = GU.make_crops(2, seed=3)[0][:2].to(dev)
                feats[route] = student.forward_return_n_last_blocks(crop, n=4, depth=[cf['n'] for cf in student.layer_cfgs]).float()
            student.train()
            trainer = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=1, teacher_stream=False)
            crops = [c.to(dev) for c in GU.make_crops(16, seed=1234)]
            res[route] = [trainer.step(crops, 5e-4 * 16 / 256.0, 0.04, 0.996, 1).item() for _ in range(3)]
            assert (calls["fwd"] > 0) == (route == "fused") and (calls["bwd"] > 0) == (route == "fused"), (route, calls)
            del student, teacher, loss_fn, trainer, crops
            torch.cuda.empty_cache()
    finally:
        _teardown()
    print(json.dumps(dict(test="routes", losses=res)))
    assert all(math.isfinite(x) for x in res["fused"]), res
    assert abs(res["fused"][0] - res["dense"][0]) < FULL_VIL_BF16_BOUNDS["vil_tiny_k8192_b2"][1], res
    d = (feats["fused"] - feats["dense"]).abs().max().item() / feats["dense"].abs().max().item()
    assert d < 3e-2, d  # (the bound forward_return_n_last_blocks has against the reference's fixture in bf16)
