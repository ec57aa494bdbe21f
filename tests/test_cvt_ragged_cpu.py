"""-m "not gpu": the ragged multi-crop route of CvT (models/cvt_v4_transformer.py: forward_feature_maps_multi; functional.CvtAttnMultiFn /
CvtFfnMultiFn / ConvEmbedMultiFn) on the torch restatement of every kernel (oracle/ops_ref.py has no grouped entries, so the spatial
kernels run group by group: the fallback of the route), and the argument checks of the grouped entries of the library."""
import ctypes as C
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import ops_ref
from tests import golden_utils as GU
from tests.test_composition_cpu import (build_cvt_variant, check_cvt_variant, check_nano_cvt, cpu_ops, nano_cvt_pair,  # noqa: F401  (cpu_ops: fixture)
                                        run_nano_cvt_step)
from tests.test_oracle_cpu import GOLD

NBLOCKS = sum(GU.NANO_CVT["depths"])


class CountingOps:
    """the ops module behind a proxy that counts the calls of every entry (and can record the arguments of some)"""

    def __init__(self, base, record=()):
        self._base, self.calls, self.seen, self._record = base, {}, {}, set(record)

    def __getattr__(self, name):
        attr = getattr(self._base, name)  # (AttributeError for an entry the base lacks: hasattr() stays truthful)
        if not callable(attr):
            return attr

        def call(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            if name in self._record:
                self.seen.setdefault(name, []).append((a, k))
            return attr(*a, **k)
        return call


def use_ops(monkeypatch, proxy):
    import esvit_amd.functional as Fn
    import esvit_amd.loss as L
    import esvit_amd.params as P
    for mod in (Fn, L, P):
        monkeypatch.setattr(mod, "ops", proxy)


def _step(ragged, loss_mod):
    student, teacher = nano_cvt_pair()
    student.ragged_multi_crop = ragged
    s_out, t_out, loss = run_nano_cvt_step(student, teacher, loss_mod)
    return student, s_out, t_out, loss


def test_ragged_equals_per_group(cpu_ops):  # noqa: F811
    """nano CvT, 2 global + 3 local crops: the three output tensors and the loss to 1e-5 of the per-group side's maximum, every parameter
    gradient to 20 times that -- the bounds of check_ragged_equals_reference_schedule, which the other ragged routes are held to (the
    gradients of the attention's pre-norm are sums that cancel to ~1e-7 behind the BatchNorm, which removes their scale: there the two
    summation orders differ by up to 1.3e-4 of the tensor's maximum, 1e-11 absolute) --, the BatchNorm running statistics to 1e-5,
    num_batches_tracked exactly"""
    import esvit_amd.loss as L
    tol = 1e-5
    (sa, oa, _, la), (sb, ob, _, lb) = _step(True, L), _step(False, L)
    assert list(oa[3]) == list(ob[3])
    for a, b in zip(oa[:3], ob[:3]):
        assert a.shape == b.shape and (a - b).abs().max().item() <= tol * (b.abs().max().item() + 1e-12)
    assert abs(la.item() - lb.item()) <= tol
    ga = {n: p.grad for n, p in sa.named_parameters() if p.grad is not None}
    gb = {n: p.grad for n, p in sb.named_parameters() if p.grad is not None}
    assert ga.keys() == gb.keys()
    for n in ga:
        err = (ga[n] - gb[n]).abs().max().item()
        print("grad %-50s %.2e of %.2e" % (n, err, gb[n].abs().max().item()))
        assert err <= 20 * tol * (gb[n].abs().max().item() + 1e-12), n
    ba, bb = sa.state_dict(), sb.state_dict()
    seen = 0
    for k in ba:
        if k.endswith("num_batches_tracked"):
            assert torch.equal(ba[k], bb[k]), k
            seen += 1
        elif "running_" in k:
            assert (ba[k] - bb[k]).abs().max().item() <= tol * (bb[k].abs().max().item() + 1e-12), k
    assert seen == NBLOCKS and all(int(ba[k]) == 2 for k in ba if k.endswith("num_batches_tracked"))  # one update per group and layer


def test_ragged_step_matches_reference_golden(cpu_ops):  # noqa: F811
    """the reference's own step (tests/golden/nano_cvt_step.pt) with the route on, under the bounds of
    test_cvt_composition_matches_reference_golden"""
    import esvit_amd.loss as L
    g = torch.load(os.path.join(GOLD, "nano_cvt_step.pt"), weights_only=False)
    student, s_out, t_out, loss = _step(True, L)
    check_nano_cvt(g, student, s_out, t_out, loss, rt=3e-4, loss_tol=2e-5, grad_tol=2e-3, buf_tol=1e-4)


def test_drop_path_rows_follow_their_samples(cpu_ops, monkeypatch):  # noqa: F811
    """stochastic depth with FIXED per-sample factors (the route draws once for the samples of all groups and expands to rows; its random
    stream is not the per-group schedule's, so the factors are pinned here): sample i of group g gets the same factor on both schedules ->
    same outputs and gradients to the bounds of test_ragged_equals_per_group"""
    from esvit_amd import models
    from esvit_amd.models import cvt_v4_transformer as M
    from oracle import ref_loader as RL
    nB = {0: 4, 1: 6}  # 2 global crops and 3 local crops of batch 2
    table = {}

    def fixed(self, n, device):
        depth = len(self.layers)
        F = table.setdefault(id(self), (torch.rand(depth, 2, 10, generator=torch.Generator().manual_seed(depth)) < 0.6).float() / 0.6)
        off = {nB[0]: 0, nB[1]: nB[0], 10: 0}[n]
        return F[:, :, off:off + n].contiguous()
    monkeypatch.setattr(M.Transformer, "drop_path_factors", fixed)
    crops = GU.make_crops(2, n_local=3, sizes=GU.NANO_CVT["sizes"])
    res = []
    for ragged in (True, False):
        cfg = RL.cvt_config(dims=GU.NANO_CVT["dims"], heads=GU.NANO_CVT["heads"], depths=GU.NANO_CVT["depths"])
        cfg.MODEL.SPEC["DROP_PATH_RATE"] = 0.4
        m = models.build_model(cfg, use_dense_prediction=True)
        m.head = m.head_dense = torch.nn.Identity()
        GU.fill_state_dict(m.state_dict(), 0)
        for k, v in m.state_dict().items():
            if k.endswith("running_var"):
                v.abs_().add_(0.5)
        m.ragged_multi_crop = ragged
        table.clear()
        cls, _, fea, _ = m(crops)
        (cls.square().sum() + fea.square().sum()).backward()
        res.append((cls, fea, {n: p.grad for n, p in m.named_parameters() if p.grad is not None}))
    (ca, fa, ga), (cb, fb, gb) = res
    assert (ca - cb).abs().max().item() <= 1e-5 * cb.abs().max().item() and (fa - fb).abs().max().item() <= 1e-5 * fb.abs().max().item()
    assert ga.keys() == gb.keys()
    for n in ga:
        assert (ga[n] - gb[n]).abs().max().item() <= 2e-4 * (gb[n].abs().max().item() + 1e-12), n


def _running_update(rm, rv, groups, order=None, pooled=False, momentum=0.1):
    """local restatement of the rule: one nn.BatchNorm2d momentum update per resolution group, in group order, each with the group's own
    batch statistics (unbiased variance).  groups: [(sums [2, C], n)].  Mutations: `order` (another sequence), `pooled` (one update with
    the statistics of all groups together)"""
    rm, rv = rm.clone(), rv.clone()
    if pooled:
        groups = [(sum(s for s, _ in groups), sum(n for _, n in groups))]
    for i in (order or range(len(groups))):
        s, n = groups[i]
        mean = s[0] / n
        var = (s[1] / n - mean * mean).clamp_min(0.0)
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * (n / (n - 1.0))
    return rm, rv


def test_the_fixture_pins_the_group_order_of_the_running_statistics(cpu_ops, monkeypatch):  # noqa: F811
    """the running statistics of the reference's step are those of two successive updates, 224-crop group first.  The statistics the route
    hands to its coefficient kernel for the first BatchNorm, put through a local restatement of the rule, reproduce the fixture's buffers to
    the bound of the golden test; the same restatement with the order swapped, or with the groups pooled into one update, misses it"""
    import esvit_amd.loss as L
    g = torch.load(os.path.join(GOLD, "nano_cvt_step.pt"), weights_only=False)
    key = "stage0.1.layers.0.0.fn.qkv.bn."
    proxy = CountingOps(ops_ref, record=("bn_fwd_coeffs",))
    use_ops(monkeypatch, proxy)
    student, teacher = nano_cvt_pair()
    rm0, rv0 = (student.state_dict()[key + n].clone() for n in ("running_mean", "running_var"))
    student.ragged_multi_crop = True
    proxy.seen.clear()
    crops = GU.make_crops(2, n_local=3, sizes=GU.NANO_CVT["sizes"])
    student(crops)
    first = proxy.seen["bn_fwd_coeffs"][:2]  # the first block's two groups (no call comes from the teacher here)
    groups = [(a[0].clone(), float(a[1])) for a, _ in first]
    assert groups[0][1] > groups[1][1]  # the 224-crop group (more positions) comes first, as the crops do
    want_m, want_v = g["bn_buffers"][key + "running_mean"].float(), g["bn_buffers"][key + "running_var"].float()

    def holds(rm, rv):
        return torch.allclose(rm, want_m, rtol=1e-4, atol=1e-4) and torch.allclose(rv, want_v, rtol=1e-4, atol=1e-4)
    assert holds(*_running_update(rm0, rv0, groups))
    assert not holds(*_running_update(rm0, rv0, groups, order=(1, 0)))
    assert not holds(*_running_update(rm0, rv0, groups, pooled=True))
    sd = student.state_dict()
    assert holds(sd[key + "running_mean"], sd[key + "running_var"]) and int(sd[key + "num_batches_tracked"]) == g["bn_buffers"][key + "num_batches_tracked"]


@pytest.mark.parametrize("name", sorted(GU.NANO_CVT_VARIANTS))
def test_variants_with_the_route_on_match_reference_golden(name, cpu_ops, monkeypatch):  # noqa: F811
    """REL_POS_EMBED / SHIFT / RES_STEM with the route on (the model reads ESVIT_CVT_RAGGED when it is built) at the bounds of
    test_cvt_variants_composition_matches_reference_golden; the student's blocks really ran through the multi functions"""
    import esvit_amd.functional as Fn
    import esvit_amd.loss as L
    monkeypatch.setenv("ESVIT_CVT_RAGGED", "1")
    multi, orig = [], Fn.cvt_block_multi
    monkeypatch.setattr(Fn, "cvt_block_multi", lambda *a, **k: (multi.append(len(a[1])), orig(*a, **k))[1])
    student = check_cvt_variant(name, L)
    assert student.ragged_multi_crop and len(multi) == sum(GU.NANO_CVT_VARIANTS[name]["cfg"]["depths"]) and set(multi) == {2}


def test_rpe_w14_with_the_route_on_matches_reference_golden(cpu_ops, monkeypatch):  # noqa: F811
    """tests/golden/nano_cvt_rpe_w14.pt (14x14 windows, head_dim 64, a table per attention, residual stem) with the route on, at the
    bounds of test_nano_rpe_w14_composition_matches_reference_golden"""
    import esvit_amd.loss as L
    from tests.test_rpe_hd64_cpu import load_fixture, nano_pair, run_step
    monkeypatch.setenv("ESVIT_CVT_RAGGED", "1")
    g = load_fixture()
    student, teacher = nano_pair(g["case"])
    assert student.ragged_multi_crop
    s_out, t_out, loss = run_step(g["case"], student, teacher, L)
    check_nano_cvt(g, student, s_out, t_out, loss, rt=3e-4, loss_tol=2e-5, grad_tol=2e-3, buf_tol=1e-4)
    got = dict(student.named_parameters())
    for n, ref in g["table_grads"].items():
        err = (got[n].grad - ref).abs().max().item()
        assert err <= 2e-3 * ref.abs().max().item(), (n, err, ref.abs().max().item())


def test_route_on_still_refuses_what_the_reference_cannot_run(cpu_ops, monkeypatch):  # noqa: F811
    """the refusals of test_cvt_variants_refuse_what_the_reference_cannot_run, raised per group with the route on: a second group whose map is
    narrower than the window, or (SHIFT) no multiple of it"""
    monkeypatch.setenv("ESVIT_CVT_RAGGED", "1")
    m = build_cvt_variant(GU.NANO_CVT_VARIANTS["rpe_shift"])
    assert m.ragged_multi_crop and m.training
    ok = GU.NANO_CVT_VARIANTS["rpe_shift"]["sizes"][0]
    with pytest.raises(RuntimeError, match="smaller than"):
        m([torch.randn(1, 3, ok, ok), torch.randn(1, 3, 24, 24)])
    with pytest.raises(RuntimeError, match="multiple"):
        m([torch.randn(1, 3, ok, ok), torch.randn(1, 3, 64, 64)])
    with pytest.raises(RuntimeError, match="smaller than"):  # (and the single-group path as before)
        m([torch.randn(1, 3, 24, 24)])


def test_routing_and_launch_counts(cpu_ops, monkeypatch):  # noqa: F811
    """a single group, eval mode and an unset ESVIT_CVT_RAGGED take the per-group functions (CvtAttnFn runs, the multi blocks do not); with
    the route on a block costs 2 LayerNorm and 4 GEMM launches per training pass whatever the number of groups"""
    import esvit_amd.functional as Fn
    from tests.test_composition_cpu import build_nano_cvt
    monkeypatch.delenv("ESVIT_CVT_RAGGED", raising=False)
    assert not build_nano_cvt().ragged_multi_crop
    monkeypatch.setenv("ESVIT_CVT_RAGGED", "1")
    assert build_nano_cvt().ragged_multi_crop
    monkeypatch.setenv("ESVIT_CVT_RAGGED", "0")
    assert not build_nano_cvt().ragged_multi_crop
    proxy = CountingOps(ops_ref)
    use_ops(monkeypatch, proxy)
    ran = {"per_group": 0, "multi": 0}
    f0, m0 = Fn.CvtAttnFn.forward, Fn.CvtAttnMultiFn.forward
    monkeypatch.setattr(Fn.CvtAttnFn, "forward", staticmethod(lambda *a, **k: (ran.__setitem__("per_group", ran["per_group"] + 1), f0(*a, **k))[1]))
    monkeypatch.setattr(Fn.CvtAttnMultiFn, "forward", staticmethod(lambda *a, **k: (ran.__setitem__("multi", ran["multi"] + 1), m0(*a, **k))[1]))
    S, Sl = GU.NANO_CVT["sizes"]
    crops2 = GU.make_crops(1, n_local=2, sizes=(S, Sl))            # two groups
    crops3 = crops2 + [torch.randn(1, 3, Sl - 8, Sl - 8)]         # three groups

    def run(model, crops):
        ran.update(per_group=0, multi=0)
        proxy.calls.clear()
        out = model(crops)
        return out, dict(ran), dict(proxy.calls)

    student, _ = nano_cvt_pair()
    _, r, _ = run(student, crops2)                                  # flag off (the default): today's path, once per group and block
    assert r == {"per_group": 2 * NBLOCKS, "multi": 0}
    student.ragged_multi_crop = True
    _, r, _ = run(student, crops2[:2])                              # one group of two crops
    assert r == {"per_group": NBLOCKS, "multi": 0}
    student.eval()
    with torch.no_grad():
        _, r, _ = run(student, crops2)                              # eval mode
    assert r == {"per_group": 2 * NBLOCKS, "multi": 0}
    student.train()
    stages = len(GU.NANO_CVT["dims"])                              # one ConvEmbed (GEMM + LayerNorm) per stage, one final norm
    for crops, G in ((crops2, 2), (crops3, 3)):
        _, r, _ = run(student, crops)
        assert r == {"per_group": 0, "multi": NBLOCKS}
        bounds = [(0, 2), (2, 4)] + ([(4, 5)] if G == 3 else [])
        proxy.calls.clear()
        student.forward_feature_maps_multi([crops[a:b] for a, b in bounds])   # (the backbone alone: the heads' GEMMs are not a block's)
        calls = dict(proxy.calls)
        assert calls["layernorm_fwd"] == 2 * NBLOCKS + stages + 1, (G, calls)
        assert calls["linear_fwd"] == 4 * NBLOCKS + stages, (G, calls)
        assert calls["window_attn_fwd"] == G * NBLOCKS and calls["bn_fwd_coeffs"] == G * NBLOCKS, (G, calls)


def test_every_student_gradient_is_one_contribution(cpu_ops, monkeypatch):  # noqa: F811
    """with a gradient sink armed (the data-parallel reducer's bucket slots) every backbone parameter's slot is handed out exactly once per
    backward with the route on, and the gradient autograd stores IS the slot: nothing was added to it.  The per-group schedule asks
    for every block parameter's slot once per group and gets it for the first contribution only"""
    import esvit_amd.loss as L
    import esvit_amd.params as P
    asked = {}
    g0 = P.grad_out

    def counting(p, shape2d=None):
        if p is not None:
            asked[id(p)] = asked.get(id(p), 0) + 1
        return g0(p, shape2d)
    monkeypatch.setattr(P, "grad_out", counting)
    for ragged in (True, False):
        student, teacher = nano_cvt_pair()
        student.ragged_multi_crop = ragged
        sinks = {id(p): torch.full_like(p, float("nan")) for p in student.parameters()}
        P.set_grad_sink(sinks)
        asked.clear()
        try:
            run_nano_cvt_step(student, teacher, L)
        finally:
            P.set_grad_sink(None)
        backbone = {n: p for n, p in student.named_parameters() if n.startswith("stage") or n.startswith("norm.")}
        assert len(backbone) > 16 * NBLOCKS
        if ragged:
            # (BatchNorm's and the depthwise filter's gradients are sums over the groups formed inside the node: one contribution, no slot)
            slotless = ("qkv.bn.", "qkv.dw.")
            for n, p in backbone.items():
                if any(s in n for s in slotless):
                    assert asked.get(id(p), 0) == 0 and p.grad is not None and not torch.isnan(p.grad).any(), n
                else:
                    assert asked.get(id(p), 0) == 1, (n, asked.get(id(p), 0))
                    assert p.grad.data_ptr() == sinks[id(p)].data_ptr(), n  # autograd adopted the slot: a single contribution
                    assert not torch.isnan(sinks[id(p)]).any(), n
        else:  # one pass per group: two contributions per parameter, summed by autograd into a tensor of its own
            summed = [n for n, p in backbone.items() if p.grad.data_ptr() != sinks[id(p)].data_ptr()]
            assert len(summed) >= 14 * NBLOCKS, len(summed)


def _world2_worker(rank, world, port, out):
    """two ranks, SyncBatchNorm over the default group: the reducer's averaged gradients and the BatchNorm buffers of the route equal the
    per-group schedule's on the same rank (rtol 2e-4 / atol 1e-5, what tests/test_dist_cpu.py holds the CvT block's gradients to); the
    route issues ONE statistics all-reduce per BatchNorm layer and pass"""
    from tests.test_dist_cpu import _init
    _init(rank, world, port)
    import esvit_amd.functional as Fn
    import esvit_amd.loss as L
    import esvit_amd.params as P
    from esvit_amd.engine import GradBucketReducer
    for mod in (Fn, L, P):
        mod.ops = ops_ref
    ops_ref.set_act_dtype(torch.float32)
    reduces, a0 = [], Fn._allreduce_stats
    Fn._allreduce_stats = lambda t, group: (reduces.append(tuple(t.shape)), a0(t, group))[1]

    def run(ragged):
        P.clear()
        student, teacher = nano_cvt_pair()
        student.ragged_multi_crop = ragged
        red = GradBucketReducer(student, bucket_mb=0.25)
        assert red.enabled
        crops = GU.make_crops(1, n_local=3, sizes=GU.NANO_CVT["sizes"], seed=500 + rank)
        loss_fn = L.DDINOLoss(GU.NANO_HEAD["out_dim"], 5, 0.04, 0.04, 0, 1)
        loss_fn._reduce_and_apply = lambda buf, apply: None
        with torch.no_grad():
            t_out = teacher(crops[:2])
        reduces.clear()
        s_out = student(crops)
        fwd = list(reduces)
        loss = loss_fn(s_out, t_out, 0, None)
        red.begin()
        reduces.clear()
        loss.backward()
        red.finish()
        bwd = list(reduces)
        grads = {n: p.grad.detach().clone() for n, p in student.named_parameters() if p.grad is not None}
        bufs = {k: v.clone() for k, v in student.state_dict().items() if "running_" in k or "num_batches" in k}
        red.close()
        return grads, bufs, fwd, bwd
    ga, ba, fa, wa = run(True)
    gb, bb, fb, wb = run(False)
    widths = lambda shapes: sorted(s[-1] for s in shapes)  # noqa: E731
    why = []
    if not (len(fa) == NBLOCKS and len(wa) == NBLOCKS and all(len(s) == 3 and s[0] == 2 for s in fa + wa)):  # stacked [G, 2, C], one per layer and pass
        why.append("route: all-reduces %r / %r" % (fa, wa))
    if not (len(fb) == 2 * NBLOCKS and len(wb) == 2 * NBLOCKS and widths(fb) == sorted(2 * widths(fa))):  # (twice as many: one per group)
        why.append("per group: all-reduces %r / %r" % (fb, wb))
    if set(ga) != set(gb):
        why.append("gradient names")
    why += ["grad " + n for n in ga if n in gb and not torch.allclose(ga[n], gb[n], rtol=2e-4, atol=1e-5)]
    why += ["buffer " + k for k in ba if not (torch.equal(ba[k], bb[k]) if "num_batches" in k else torch.allclose(ba[k], bb[k], rtol=2e-4, atol=1e-5))]
    out[rank] = "; ".join(why) or True
    dist.destroy_process_group()


def test_world2_gloo_route_equals_per_group(lib_built):
    out = mp.Manager().dict()
    mp.spawn(_world2_worker, args=(2, 29641, out), nprocs=2, join=True)
    assert dict(out) == {0: True, 1: True}, dict(out)


def test_grouped_entries_refuse_bad_records(lib_built):
    """one rejection per check of the grouped mode of each of the four entries: ESVIT_ERR_ARG before any launch, the cause in
    esvit_last_error().  The device pointers are fakes that nothing dereferences (the record array itself is host memory the entry
    reads); a well-formed grouped call gets past the checks and fails at the launch on this GPU-less host (ESVIT_ERR_HIP)"""
    from esvit_amd import _lib, ops
    lib = _lib.lib
    fake, odd = 0x1000, 0x1008
    BF, F32 = ops.BF16, ops.F32

    def recs(n=2, **over):
        arr = (_lib.GridGroup * max(n, 1))()
        for i, r in enumerate(arr):
            r.p0, r.p1, r.out, r.a1, r.a2, r.a3 = fake, fake, fake, fake, fake, fake
            r.nB, r.H, r.W, r.Hd, r.Wd, r.C, r.dtype = 2, 6, 6, 7, 7, 64, BF
            for k, v in over.items():
                if isinstance(v, tuple):
                    if v[0] == i:
                        setattr(r, k, v[1])
                else:
                    setattr(r, k, v)
        return arr

    def ptr(arr):
        return None if arr is None else C.c_void_p(C.addressof(arr))

    def pad(arr, n=-2, dtype=BF, Cc=64):
        return lib.esvit_pad_crop_tokens(dtype, ptr(arr), n, 0, 0, 0, 0, Cc, None, None), lib.esvit_last_error()

    def dw(arr, n=-2, dtype=BF, Cc=64, w=fake):
        return lib.esvit_dwconv3x3(dtype, ptr(arr), w, 0, n, 0, 0, Cc, None, None), lib.esvit_last_error()

    def sums(arr, n=-2, dtype=BF, Cc=64, out=fake, ws=fake):
        return lib.esvit_col_sums2(dtype, ptr(arr), None, n, Cc, out, ws, None), lib.esvit_last_error()

    def aff(arr, n=-2, dtype=BF, Cc=64, act=0):
        return lib.esvit_col_affine2(dtype, ptr(arr), None, n, Cc, None, None, None, act, None, None), lib.esvit_last_error()

    cases = []
    for fn in (pad, dw, sums, aff):  # the checks all four share
        cases += [(fn(recs(), n=-5), b"1..4 groups"), (fn(None), b"without a record array"), (fn(recs(C=(1, 128))), b"group 1 has C=128"),
                  (fn(recs(dtype=(1, F32))), b"group 1 has dtype"), (fn(recs(), dtype=7), b"bad dtype"), (fn(recs(nB=(1, 0))), b"group 1: bad grid"),
                  (fn(recs(H=(0, -3))), b"group 0: bad grid")]
    cases += [(pad(recs(p0=(1, None))), b"group 1: bad args"), (pad(recs(Hd=(1, 0))), b"group 1: bad args"), (pad(recs(out=(0, odd))), b"group 0: src, dst"),
              (pad(recs(C=60), Cc=60), b"C=60"),
              (dw(recs(out=(1, None))), b"group 1: null x / y"), (dw(recs(), w=None), b"bad args"), (dw(recs(C=62), Cc=62), b"bad args (C=62)"),
              (dw(recs(p0=(1, odd))), b"1 of 2 groups are 16-byte aligned"), (dw(recs(C=2048, dtype=F32), Cc=2048, dtype=F32), b"too wide"),
              (dw(recs(dtype=F32, p0=(1, odd)), dtype=F32), b"group 1: x, y must be aligned"),
              (sums(recs(p1=(1, None))), b"group 1: null a / b"), (sums(recs(), out=None), b"bad args"), (sums(recs(C=2048), Cc=2048), b"C <= 1024"),
              (sums(recs(), ws=odd), b"ws must be aligned"), (sums(recs(p0=(0, 0x1004))), b"group 0: a, b must be aligned"),
              (aff(recs(a3=(1, None))), b"group 1: null x1"), (aff(recs(), act=5), b"bad args"), (aff(recs(a2=(1, None))), b"group 1: x2 / a2 do not fit act=0"),
              (aff(recs(), act=3), b"do not fit act=3"), (aff(recs(p1=(0, None)), act=4), b"group 0: x2 / a2 do not fit act=4")]
    for got, cause in cases:
        assert got[0] == -1 and cause in got[1], (got, cause)
    # well-formed: past every check, refused by the runtime only (no device here)
    for got in (pad(recs()), dw(recs()), sums(recs()), aff(recs()), aff(recs(p1=None, a2=None)), pad(recs(1), n=-1), sums(recs(4), n=-4)):
        assert got[0] not in (0, -1), got
    # the plain calls are untouched by the mode: a zero count is still "bad args"
    assert lib.esvit_pad_crop_tokens(BF, fake, 0, 6, 6, 7, 7, 64, fake, None) == -1 and b"bad args" in lib.esvit_last_error()
    assert lib.esvit_col_sums2(BF, fake, fake, 0, 64, fake, fake, None) == -1 and b"bad args" in lib.esvit_last_error()
