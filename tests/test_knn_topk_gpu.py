"""Fused k-NN scoring on the MI355X (esvit_gemm_desc::topk -> ops.knn_topk -> eval.knn_classifier_multi): exact selection against
the kernel's own similarities, the similarities against fp64, order / determinism / streaming, the memory bound that is the point of
the kernel, and the end-to-end votes against the reference's golden numbers and the oracle."""
import json
import os

import pytest
import torch

from oracle import esvit_oracle as O
from tests import golden_utils as GU
from tests import knn_ref as KR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PARITY = os.path.join(ROOT, "profiles", "knn_topk_parity.jsonl")
KS = (10, 20, 100, 200)

# (Nt, Ntr, C, k): the issue's four, ragged sizes that are no multiple of any tile, Ntr just above k, one split / many splits
SHAPES = [(400, 1500, 48, 10), (400, 1500, 48, 200), (3000, 20000, 384, 256), (130, 257, 4, 1),
          (77, 1001, 20, 33), (129, 4099, 36, 256), (1, 300, 8, 7), (257, 201, 12, 200), (50, 257, 16, 256), (1031, 9001, 100, 64)]


def _unit(n, c, seed, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, c, generator=g), dim=1).to(dev)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selection_is_exact_and_similarities_are_right(shape, lib_built):
    from esvit_amd import ops
    Nt, Ntr, C, k = shape
    dev = _dev()
    te, tr = _unit(Nt, C, 1), _unit(Ntr, C, 2)
    vals, idx, sim = ops.knn_topk(te.to(dev), tr.to(dev), k, return_similarity=True)
    want_v, want_i = KR.topk_of(sim, k)
    assert torch.equal(vals, want_v), (vals - want_v).abs().max().item()
    assert torch.equal(idx, want_i)
    v2, i2 = ops.knn_topk(te.to(dev), tr.to(dev), k)  # no C: nothing of size Nt x Ntr is written
    assert torch.equal(v2, vals) and torch.equal(i2, idx)
    # the similarities against the fp64 product: the worst-case fp32 accumulation bound for unit rows
    sim64 = te.double() @ tr.double().t()
    bound = C * 2.0 ** -24
    err = (sim.cpu().double() - sim64).abs().max().item()
    line = dict(test="knn_topk_similarity", shape=list(shape), max_abs_err=err, bound=bound)
    GU.record_parity(**line)
    try:
        with open(PARITY, "a") as fh:
            fh.write(json.dumps(line) + "\n")
    except OSError:
        pass
    assert err <= bound, (err, bound)
    # neighbour sets against fp64, delta = twice that bound: nothing returned lies below the k-th fp64 value - delta, and
    # everything above the k-th fp64 value + delta is returned (every row, no cap on skipped cases)
    delta = 2 * bound
    kth = sim64.sort(dim=1, descending=True).values[:, k - 1:k]
    got64 = torch.gather(sim64, 1, idx.cpu().long())
    assert bool((got64 >= kth - delta).all())
    returned = torch.zeros(Nt, Ntr, dtype=torch.bool)
    returned.scatter_(1, idx.cpu().long(), True)
    assert bool(returned[sim64 > kth + delta].all())
    assert int(returned.sum()) == Nt * k  # k distinct rows each


def test_duplicated_rows_ascend_and_launches_repeat(lib_built):
    from esvit_amd import ops
    dev = _dev()
    te = _unit(300, 32, 3, dev)
    base = _unit(2000, 32, 4)
    tr = torch.cat([base, base[:700], base[100:400]]).to(dev)  # duplicates 128-column tiles and splits apart
    vals, idx = ops.knn_topk(te, tr, 120)
    same = vals[:, 1:] == vals[:, :-1]
    assert int(same.sum()) > 300
    assert bool((idx[:, 1:][same] > idx[:, :-1][same]).all())
    v2, i2 = ops.knn_topk(te, tr, 120)
    assert torch.equal(v2, vals) and torch.equal(i2, idx)


def test_ten_launches_at_full_occupancy_are_identical(lib_built):
    """1024 row tiles x 1 split = 1024 workgroups of the scan, four per CU (two resident at once): every launch gives the same bits"""
    from esvit_amd import ops
    dev = _dev()
    te, tr = _unit(128 * 1024, 32, 5, dev), _unit(4096, 32, 6, dev)
    tr[1000:1500] = tr[:500]  # ties, too
    first = ops.knn_topk(te, tr, 50)
    first = (first[0].clone(), first[1].clone())
    for _ in range(9):
        v, i = ops.knn_topk(te, tr, 50)
        assert torch.equal(v, first[0]) and torch.equal(i, first[1])
    te2, tr2 = _unit(128 * 40, 64, 7, dev), _unit(60000, 64, 8, dev)  # 40 row tiles x 12 splits
    first = tuple(t.clone() for t in ops.knn_topk(te2, tr2, 200))
    for _ in range(9):
        v, i = ops.knn_topk(te2, tr2, 200)
        assert torch.equal(v, first[0]) and torch.equal(i, first[1])


def test_streaming_equals_one_shot(lib_built):
    from esvit_amd import eval as E
    from esvit_amd import ops
    dev = _dev()
    te, tr = _unit(700, 64, 9, dev), _unit(30000, 64, 10, dev)
    tr[20000:20300] = tr[5:305]  # ties across pieces
    for k in (1, 200):
        want = ops.knn_topk(te, tr, k)
        out, base = None, 0
        for piece in (tr[:7001], tr[7001:7300], tr[7300:]):
            out = ops.knn_topk(te, piece.contiguous(), k, out=out, idx_base=base)
            base += piece.shape[0]
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
        trc = tr.cpu()
        got = E.knn_topk_streamed(te, [trc[:12345], trc[12345:12600], trc[12600:]], k)
        assert got[0].is_cuda and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a late piece shorter than k merges too
    want = ops.knn_topk(te, tr[:10050].contiguous(), 200)
    out = ops.knn_topk(te, tr[:10000].contiguous(), 200)
    out = ops.knn_topk(te, tr[10000:10050].contiguous(), 200, out=out, idx_base=10000)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    with pytest.raises(ValueError):
        ops.knn_topk(te, tr[:100].contiguous(), 200)


def test_memory_bound(lib_built):
    """nothing of size Nt x Ntr is allocated: the call grows the allocator's peak by its scratch (ESVIT_Q_TOPK_WS) and the two outputs"""
    from esvit_amd import ops
    dev = _dev()
    Nt, Ntr, C, k = 4096, 300000, 64, 200
    te, tr = _unit(Nt, C, 11, dev), _unit(Ntr, C, 12, dev)
    ops.knn_topk(te[:64], tr[:1000].contiguous(), 10)  # warm the cached ops.workspace() pool (and the kernels) with a small call
    ws = ops.query(ops.Q_TOPK_WS, Nt, Ntr, k)
    assert ws == ops.query(ops.Q_TOPK_WS, Nt, 1280000, k)  # rows, k and the split count; not the length of the scan
    dense = Nt * Ntr * 4
    assert 0 < ws < dense // 10
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    vals, idx = ops.knn_topk(te, tr, k)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    outputs = Nt * k * 8
    rounding = 3 * (2 << 20)  # three allocations, each rounded up by the caching allocator to at most 2 MiB
    GU.record_parity(test="knn_topk_memory", grown=grown, ws=ws, outputs=outputs, dense=dense)
    assert grown <= ws + outputs + rounding, (grown, ws, outputs)
    want_v, want_i = KR.topk_of(ops.linear_fwd(te[:256].contiguous(), tr), k)  # a corner against the dense route (same MFMA order)
    assert torch.equal(idx[:256], want_i) and torch.equal(vals[:256], want_v)


def test_end_to_end_votes(lib_built, monkeypatch):
    import esvit_amd
    from esvit_amd import eval as E
    from esvit_amd import ops
    dev = _dev()
    esvit_amd.set_precision("fp32")
    try:
        gold = torch.load(os.path.join(GOLD, "knn.pt"), weights_only=False)
        sets = [GU.make_knn_set(c["seed"], noise=c["noise"]) for c in GU.KNN_CASES]
        monkeypatch.setattr(E, "KNN_ROUTE", "fused")
        for c, want, (xtr, ytr, xte, yte) in zip(GU.KNN_CASES, gold["top"], sets):
            got = E.knn_classifier(xtr.to(dev), ytr.to(dev), xte.to(dev), yte.to(dev), c["k"], c["T"], num_classes=10)
            GU.record_parity(test="knn_fused_golden", case=c, got=got, want=want)
            assert got == pytest.approx(want, abs=0.26), (c, got, want)
        xtr, ytr, xte, yte = GU.make_knn_set(11, n_train=20000, n_test=3000, dim=384, classes=100, noise=6.0)
        got = E.knn_classifier_multi(xtr.to(dev), ytr.to(dev), xte.to(dev), yte.to(dev), KS, 0.07, num_classes=100)
        for k in KS:
            want = O.knn_classifier(xtr, ytr, xte, yte, k, 0.07, num_classes=100)
            GU.record_parity(test="knn_fused_oracle", k=k, got=got[k], want=want)
            assert got[k] == pytest.approx(want, abs=0.1), (k, got[k], want)
        # the default route is the old function: no top-k descriptor is issued
        monkeypatch.setattr(E, "KNN_ROUTE", "gemm")

        def boom(*a, **kw):
            raise AssertionError("the gemm route issued a top-k descriptor")
        monkeypatch.setattr(ops, "knn_topk", boom)
        c, (xtr, ytr, xte, yte) = GU.KNN_CASES[0], sets[0]
        got = E.knn_classifier(xtr.to(dev), ytr.to(dev), xte.to(dev), yte.to(dev), c["k"], c["T"], num_classes=10)
        assert got == pytest.approx(gold["top"][0], abs=0.26)
    finally:
        esvit_amd.set_precision("bf16")


def test_reference_written_checkpoint_through_the_fused_route(lib_built, monkeypatch):
    """load -> extract_features -> knn_classifier on the checkpoint the reference wrote, fp32 mode, with the fused route; fixture and
    tolerances of test_reference_written_checkpoint_through_the_knn_consumers_gpu"""
    import esvit_amd
    from esvit_amd import eval as E
    from esvit_amd import ops
    from tests.test_composition_cpu import check_ref_checkpoint
    dev = _dev()
    esvit_amd.set_precision("fp32")
    calls = []
    real = ops.knn_topk

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    try:
        monkeypatch.setattr(E, "KNN_ROUTE", "fused")
        monkeypatch.setattr(ops, "knn_topk", counted)
        check_ref_checkpoint(dev, tol=5e-6, top_tol=1.0)
        assert len(calls) == 2  # teacher and student, through the kernel
    finally:
        esvit_amd.set_precision("bf16")
