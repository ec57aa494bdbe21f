"""The fused update kernels on the MI355X (esvit_amd/csrc/update.hip: esvit_grad_sqnorm, esvit_fused_clip_update_ema) against the float64
statement of tests/update_ref.py, on hand-built tables: AdamW, SGD and LARS at every chunk edge, with and without gradient, teacher and
bf16 copies, at three levels so that a tight element check cannot hide a statistic error -- the atomic statistics against fp64, the
per-tensor factors c and q they give, and every element given the device's own statistics -- plus the properties that need no
tolerance, the bias correction at four step counts, the non-finite guard beyond one trip of its loop, and the hand-off of the bf16
copies between FusedClipAdamWEMA and esvit_amd.params.  Bounds and the count of roundings behind each K: tests/update_ref.py;
tests/test_update_cpu.py shows that plain fp32 arithmetic meets them on these very inputs.

Worst err / bound observed on the MI355X over all variants of a rule:
  adamw  statistics 0.034  c 0.029            m  0.401  v 0.482  p 0.549  ema 0.991
  sgd    statistics 0.034  c 0.029            mu 0.459           p 0.499  ema 0.987
  lars   statistics 0.051  c 0.029  q 0.035   mu 0.238           p 0.500  ema 0.998
(the EMA is two products and a sum against K = 2, and p' of the momentum rules one FMA against K = 2: those bounds are met nearly
with equality by construction; esvit_grad_sqnorm alone: 0.034 at stats = 1, 0.051 at stats = 3.)"""
import copy

import pytest
import torch

from tests import update_ref as UR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RULES = [UR.ADAMW, UR.SGD, UR.LARS]
RULE_ID = lambda r: UR.RULE_NAMES[r]  # noqa: E731


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert ops.update_chunk_elems() == UR.CHUNK
    assert (ops.RULE_ADAMW, ops.RULE_SGD, ops.RULE_LARS) == (UR.ADAMW, UR.SGD, UR.LARS)
    return ops


class Launch:
    """the arenas of a layout on the device, its tables, and a statistics buffer between two moats"""

    def __init__(self, L, rule, h, in32, in16):
        self.L, self.rule, self.h = L, rule, h
        self.d32, self.d16 = in32.to(DEV), in16.to(DEV)
        assert self.d32.data_ptr() % 16 == 0 and self.d16.data_ptr() % 16 == 0
        self.tab = torch.from_numpy(L.table(self.d32.data_ptr(), self.d16.data_ptr(), rule, h["bc"])).to(DEV)
        self.chunks = torch.from_numpy(L.chunks).to(DEV)

    def statistics(self, ops, stats):
        n = len(self.L) * stats
        buf = torch.full((2 * UR.MOAT + n,), 7.0, dtype=torch.float32, device=DEV)  # (whatever it held: the atomic form clears it itself)
        sq = buf[UR.MOAT:UR.MOAT + n]
        ops.grad_sqnorm(self.tab, len(self.L), self.chunks, self.L.nchunks, sq, stats=stats)
        torch.cuda.synchronize()
        assert bool((buf[:UR.MOAT] == 7.0).all()) and bool((buf[UR.MOAT + n:] == 7.0).all()), "esvit_grad_sqnorm wrote outside its statistics"
        return sq

    def update(self, ops, sq, skipped=None):
        h = self.h
        ops.fused_clip_update_ema(self.rule, self.tab, len(self.L), self.chunks, self.L.nchunks, sq, h["clip"], h["lr"], h["wd"], h["h1"], h["h2"],
                                  h["eps"], h["ema_m"], skipped=skipped)
        torch.cuda.synchronize()
        return self.d32.cpu(), self.d16.cpu()


@pytest.mark.parametrize("stats", [1, 3])
def test_atomic_statistics_against_fp64(ops, stats):
    """level 1: the default (atomicAdd) esvit_grad_sqnorm within (32 + chunks_t) 2^-24 sum|terms| of fp64; exactly 0 without the gradient bit"""
    L = UR.Layout(UR.SPECS)
    in32, in16 = UR.make_inputs(L, UR.LARS, special=True)
    run = Launch(L, UR.LARS, UR.hyper(UR.LARS), in32, in16)
    sq = run.statistics(ops, stats).cpu()
    worst, broken = UR.check_statistics(L, in32, sq, stats)
    print("UPDATE statistics stats=%d worst err / bound %.3f" % (stats, worst))
    assert not broken, broken
    assert float(sq.view(len(L), stats)[UR.ZERO_G, 0]) == 0.0  # g == 0 everywhere
    assert UR.unchanged(in32, in16, run.d32.cpu(), run.d16.cpu())  # the statistics pass writes no tensor


@pytest.mark.parametrize("rule", RULES, ids=RULE_ID)
def test_update_against_fp64(ops, rule):
    """levels 1 - 3 and the exact properties for every variant of the rule: the main launch, clip == 0, lr == 0, ema_m == 1 and 0, wd == 0
    (LARS: |c g + wd p| == 0 on the tensor without gradient values) and, for AdamW, the step counts 1 (zero moments), 2, 1000 and one at
    which 1 - b2^t is exactly 1.0f"""
    L = UR.Layout(UR.SPECS)
    S = 3 if rule == UR.LARS else 1
    worst_all, broken_all = {}, []
    for name, over in UR.variants(rule).items():
        over = dict(over)
        in32, in16 = UR.make_inputs(L, rule, zero_moments=over.pop("zero_moments", False), special=True)
        h = UR.hyper(rule, **over)
        run = Launch(L, rule, h, in32, in16)
        sq = run.statistics(ops, S)
        skipped = torch.zeros(1, dtype=torch.int32, device=DEV)
        out32, out16 = run.update(ops, sq, skipped)
        assert int(skipped.item()) == 0
        stats = sq.cpu()
        w1, b1 = UR.check_statistics(L, in32, stats, S)
        w2, b2 = UR.check_factors(L, rule, h, in32, stats)
        w3, b3 = UR.check_update(L, rule, h, in32, in16, out32, out16, stats)
        worst = {"statistics": w1, **w2, **w3}
        print("UPDATE", UR.RULE_NAMES[rule], name, " ".join("%s %.3f" % kv for kv in worst.items()))
        for k, v in worst.items():
            worst_all[k] = max(worst_all.get(k, 0.0), v)
        broken_all += ["%s: %s" % (name, b) for b in b1 + b2 + b3]
        if name == "main":  # both sides of the clip threshold in one launch, and the tensors the rule must move did move
            cs = [UR.factors(L, rule, h, in32, stats, i)[0] for i, s in enumerate(L.specs) if s.has_grad]
            assert any(c < 1.0 for c in cs) and any(c == 1.0 for c in cs)
            assert not torch.equal(L.get(out32, "p", UR.BIG), L.get(in32, "p", UR.BIG))
    print("UPDATE", UR.RULE_NAMES[rule], "worst err / bound over all variants:", " ".join("%s %.3f" % kv for kv in worst_all.items()))
    assert not broken_all, broken_all


@pytest.mark.parametrize("rule", RULES, ids=RULE_ID)
def test_guard_reads_every_statistic(ops, rule):
    """300 tensors: the non-finite statistic is the last tensor's (LARS: only its sum p^2, index 3 * 299 + 1), far behind the first trip of
    the guard's loop.  Nothing moves, the counter goes up by one (not one per workgroup), a NULL counter is accepted; with the value made
    finite the launch updates tensor 0."""
    L = UR.guard_layout()
    n, last = len(L), len(L) - 1
    S = 3 if rule == UR.LARS else 1
    h = UR.hyper(rule)
    assert L.nchunks >= 2 and n * S > 256

    def inputs(poison):
        in32, in16 = UR.make_inputs(L, rule, seed=9)
        if rule == UR.LARS:
            L.get(in32, "p", last)[0] = 2e19 if poison else 2e18  # 4e38 overflows fp32, 4e36 does not
        else:
            L.get(in32, "g", last)[0] = float("inf") if poison else 1.0
        return in32, in16

    in32, in16 = inputs(True)
    run = Launch(L, rule, h, in32, in16)
    sq = run.statistics(ops, S)
    bad = (~torch.isfinite(sq)).nonzero().view(-1).tolist()
    assert bad == [S * last + (1 if rule == UR.LARS else 0)], bad
    skipped = torch.zeros(1, dtype=torch.int32, device=DEV)
    out32, out16 = run.update(ops, sq, skipped)
    assert UR.unchanged(in32, in16, out32, out16), "a refused update wrote something"
    assert int(skipped.item()) == 1
    out32, out16 = run.update(ops, sq, None)
    assert UR.unchanged(in32, in16, out32, out16) and int(skipped.item()) == 1
    # the same launch, finite
    in32, in16 = inputs(False)
    run = Launch(L, rule, h, in32, in16)
    sq = run.statistics(ops, S)
    assert bool(torch.isfinite(sq).all())
    out32, out16 = run.update(ops, sq, skipped)
    assert int(skipped.item()) == 1
    assert not torch.equal(L.get(out32, "p", 0), L.get(in32, "p", 0)) and not torch.equal(L.get(out32, "p", last), L.get(in32, "p", last))
    if rule != UR.LARS:  # (K of the LARS buffer is counted for well-conditioned q; tensors of one element are not)
        worst, broken = UR.check_update(L, rule, h, in32, in16, out32, out16, sq.cpu())
        assert not broken, broken


# ---- FusedClipAdamWEMA and the copy cache of esvit_amd.params ---------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 6, 3)   # a 4-D weight, cast as a [6, 27] matrix
        self.lin = torch.nn.Linear(7, 5)       # 35 elements: not a multiple of 4
        self.norm = torch.nn.LayerNorm(5)


def _pair():
    torch.manual_seed(11)
    student = _Net().to(DEV)
    teacher = copy.deepcopy(student)
    for p in teacher.parameters():
        p.data.mul_(0.5)
        p.requires_grad_(False)
    return student, teacher


def _shape2d(name, p):
    return (p.shape[0], p[0].numel()) if name == "conv.weight" else None


def _bits_equal(copy_, p):
    return torch.equal(copy_.reshape(-1).view(torch.int16), p.detach().to(torch.bfloat16).reshape(-1).view(torch.int16))


@pytest.mark.parametrize("rule", ["adamw", "sgd", "lars"])
def test_wrapper_refreshes_cached_copies(ops, rule, monkeypatch):
    import esvit_amd
    import esvit_amd.params as P
    from esvit_amd.update import FusedClipAdamWEMA
    P.clear()
    esvit_amd.set_precision("bf16")
    try:
        student, teacher = _pair()
        upd = FusedClipAdamWEMA(student, teacher, rule=rule)
        UNCACHED = "norm.bias"
        named = [(m, n, p) for m, net in (("student", student), ("teacher", teacher)) for n, p in net.named_parameters()]
        held = {(m, n): P.cached_cast(p, _shape2d(n, p)) for m, n, p in named if n != UNCACHED}
        assert all(c.dtype == torch.bfloat16 for c in held.values()) and held[("student", "conv.weight")].shape == (6, 27)
        calls, seeds = [], []
        real = ops.cast_to_act
        monkeypatch.setattr(ops, "cast_to_act", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

        def step(poison=None):
            seeds.append(len(seeds) + 5)
            gen = torch.Generator().manual_seed(seeds[-1])
            before = [p.detach().clone() for _, _, p in named]
            for p in student.parameters():
                p.grad = torch.randn(p.shape, generator=gen).to(DEV)
            if poison is not None:
                student.lin.weight.grad.view(-1)[34] = poison
            upd.step(0.05, 0.04, 0.9, clip_grad=3.0)
            torch.cuda.synchronize()
            moved = [not torch.equal(b, p.detach()) for b, (_, _, p) in zip(before, named)]
            assert all(moved) if poison is None else not any(moved), moved
            for m, n, p in named:
                if n == UNCACHED:
                    continue
                assert P.cached_cast(p, _shape2d(n, p)) is held[(m, n)], (m, n)  # the same tensor object ...
                assert _bits_equal(held[(m, n)], p), (m, n)                     # ... holding bf16(the new fp32 value), written by the update kernel
            assert not calls, "a copy the update kernel had refreshed was cast again"

        step()
        step()
        for m, n, p in named:  # the parameter without a cached copy: cast on demand, from the new value
            if n == UNCACHED:
                c = P.cached_cast(p)
                assert _bits_equal(c, p) and c.data_ptr() != p.data_ptr()
                held[(m, n)] = c
        assert len(calls) == 2
        del calls[:]
        UNCACHED = None
        step(float("inf"))  # refused by the guard: nothing moved, the copies are those of the unchanged parameters
        assert upd.take_skipped() == 1
        step()
        # the device table carried the copies' addresses
        tab = upd._table_dev.cpu()
        for i, (p, tp) in enumerate(zip(upd.params, upd.teacher_params)):
            assert int(tab[i, 10]) == held[("student", upd.names[i])].data_ptr() and int(tab[i, 11]) == held[("teacher", upd.names[i])].data_ptr()
        # fp32 activations: there are no bf16 copies to hand over
        esvit_amd.set_precision("fp32")
        P.clear()
        for _, n, p in named:
            P.cached_cast(p, _shape2d(n, p))
        assert all(P.cast_buffer_ptr(p, []) == 0 for _, _, p in named)
        for p in student.parameters():
            p.grad = torch.randn_like(p)
        upd.step(0.05, 0.04, 0.9, clip_grad=3.0)
        torch.cuda.synchronize()
        assert not bool(upd._table_dev[:, 10:12].any())
        for _, n, p in named:
            assert torch.equal(P.cached_cast(p, _shape2d(n, p)).reshape(-1), p.detach().reshape(-1))
    finally:
        esvit_amd.set_precision("bf16")
        P.clear()
