"""The deterministic mode on the MI355X (esvit_amd.set_deterministic): the ordered table gradient (esvit_relpos_bias_bwd |
ESVIT_RELPOS_ORDERED) and the ordered norm statistics (esvit_grad_sqnorm | ESVIT_SQNORM_ORDERED) against fp64 under the sequential
fp32 summation bound, bit-equal from launch to launch; and the whole training step -- student and teacher forward, loss, backward,
clip + optimizer + EMA -- bit-equal between two builds from one seed, in one process and between processes."""
import hashlib
import os
import subprocess
import sys
from functools import partial

import pytest
import torch

from tests import golden_utils as GU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24  # unit roundoff of fp32
SENTINEL = -12345.5
MOAT = 512


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def ops(lib_built):
    from esvit_amd import ops as o
    return o


# ---- ordered table gradient -----------------------------------------------------------------------------------------------------------
def _frag_offsets(N, nt):
    """element of (q, key) inside one head's frag-layout slab (include/esvit_hip.h)"""
    q, k = torch.arange(N)[:, None], torch.arange(N)[None, :]
    return ((((k >> 4) * nt + (q >> 4)) * 64 + ((k & 15) >> 2) * 16 + (q & 15)) * 4 + (k & 3)).reshape(-1)


def _slabs(parts, nH, fe, seed):
    """randn * 10**U(-3, 3): magnitudes over six decades, so that the order of the additions shows in the last bits"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(parts, nH, fe, generator=g) * 10.0 ** (6.0 * torch.rand(parts, nH, fe, generator=g) - 3.0)


def _table_ref(ws, index, N, nt, trows):
    """fp64 gather of the same slabs -> (table [trows, nH], the same reduction of |slab|, pairs per row [trows, 1])"""
    off = _frag_offsets(N, nt)
    idx = index.reshape(-1)
    ok = (idx >= 0) & (idx < trows)
    out = []
    for w in (ws.double(), ws.double().abs()):
        dense = w.sum(0)[:, off].t()  # [N * N, nH]
        out.append(torch.zeros(trows, ws.shape[1], dtype=torch.float64).index_add_(0, idx[ok], dense[ok]))
    pairs = torch.bincount(idx[ok], minlength=trows).double()[:, None]
    return out[0], out[1], pairs


def _moated(trows, nH, dev, fill=None):
    buf = torch.full((2 * MOAT + trows * nH,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[MOAT:MOAT + trows * nH].view(trows, nH)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _moat_intact(buf):
    return bool((buf[:MOAT] == SENTINEL).all()) and bool((buf[-MOAT:] == SENTINEL).all())


def _swin_index(ops, w):
    return torch.from_numpy(ops.relative_position_index(w)), (2 * w - 1) ** 2


TABLE_CASES = [("n49_p1", 49, 3, 1, "swin7"), ("n49_p2", 49, 3, 2, "swin7"), ("n49_p9", 49, 3, 9, "swin7"), ("n49_p341", 49, 3, 341, "swin7"),
               ("n196_p1", 196, 3, 1, "swin14"), ("n196_p5", 196, 3, 5, "swin14"), ("n36_6x6", 36, 1, 3, "swin6"),
               ("n37_block", 37, 3, 2, "block37"), ("n37_full", 37, 3, 2, "full37"), ("n196_any_content", 196, 3, 1, "any")]


def _table_case(ops, N, kind):
    """-> (index as handed to the wrapper, the [N, N] block the kernel reads, table rows)"""
    if kind == "any":  # a few rows own thousands of pairs each (more than one LDS list), some entries point outside the table
        g = torch.Generator().manual_seed(5)
        idx = torch.randint(-1, 6, (N, N), generator=g, dtype=torch.int64)
        return idx, idx, 5
    w = {"swin7": 7, "swin14": 14, "swin6": 6, "block37": 7, "full37": 7}[kind]
    full, trows = _swin_index(ops, w)
    block = full[:N, :N].contiguous()
    return (full if kind == "full37" else block), block, trows


@pytest.mark.parametrize("name,N,nH,parts,kind", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_ordered_table_gradient(ops, name, N, nH, parts, kind):
    """bound per element: (parts + P_t) 2^-24 M, the sequential fp32 summation bound of the documented order (M: the same reduction of
    |slab| in fp64, P_t: the pairs of the row); the accumulate form adds the prefilled value ONCE: one more rounding, of a sum whose
    terms now include |base|"""
    dev = _dev()
    fe = ops.attn_frag_elems(N)
    nt = 4 if N <= 64 else 14
    assert fe == nt * nt * 256
    given, block, trows = _table_case(ops, N, kind)
    ws = _slabs(parts, nH, fe, seed=parts + N)
    want, mag, pairs = _table_ref(ws, block, N, nt, trows)
    bound = (parts + pairs) * U * mag
    base = torch.randn(trows, nH, generator=torch.Generator().manual_seed(3)) * 100.0
    ws_dev, idx_dev = ws.to(dev), given.to(dev)
    # overwrite
    work = ws_dev.clone()
    buf, out = _moated(trows, nH, dev)
    assert ops.relpos_bias_bwd(work, idx_dev, N, trows, out=out, accumulate=False, ordered=True).data_ptr() == out.data_ptr()
    got = out.cpu().double()
    err = (got - want).abs()
    print(name, "overwrite: worst err / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    assert _moat_intact(buf)
    if parts > 1:
        assert torch.equal(work[1:], ws_dev[1:])  # slabs 1.. untouched; slab 0 holds the sum
    # a fresh output tensor (out=None) is the same table
    assert torch.equal(ops.relpos_bias_bwd(ws_dev.clone(), idx_dev, N, trows, ordered=True), out)
    # accumulate into a prefilled table
    buf2, acc = _moated(trows, nH, dev, fill=base.to(dev))
    ops.relpos_bias_bwd(ws_dev.clone(), idx_dev, N, trows, out=acc, accumulate=True, ordered=True)
    err2 = (acc.cpu().double() - (base.double() + want)).abs()
    bound2 = (parts + pairs + 1) * U * (mag + base.double().abs())
    print(name, "accumulate: worst err / bound", float((err2 / bound2.clamp_min(1e-300)).max()))
    assert bool((err2 <= bound2).all())
    assert _moat_intact(buf2)
    # accumulate = overwrite + one addition, bit for bit
    assert torch.equal(acc, base.to(dev) + out)
    if kind != "any":  # (the scatter of the default form would follow the stray entries out of the table)
        default = ops.relpos_bias_bwd(ws_dev.clone(), idx_dev, N, trows).cpu().double()
        assert bool(((got - default).abs() <= 2 * bound).all())


def test_ordered_table_gradient_is_bit_identical_across_launches(ops):
    dev = _dev()
    N, nH, parts = 49, 3, 341
    index, trows = _swin_index(ops, 7)
    ws, idx = _slabs(parts, nH, ops.attn_frag_elems(N), seed=11).to(dev), index.to(dev)
    first = ops.relpos_bias_bwd(ws.clone(), idx, N, trows, ordered=True)
    for _ in range(9):
        assert torch.equal(ops.relpos_bias_bwd(ws.clone(), idx, N, trows, ordered=True), first)


# ---- ordered norm statistics ------------------------------------------------------------------------------------------------------------
NUMELS = (1, 5, 4095, 4096, 4097, 3 * 4096 + 7, 1200000)
NO_GRAD = 4  # the tensor without the has-gradient bit


def _stat_tables(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ps = [(torch.randn(n, generator=g) * 10.0 ** (4.0 * torch.rand(n, generator=g) - 2.0)).to(dev) for n in NUMELS]
    gs = [(torch.randn(n, generator=g) * 10.0 ** (4.0 * torch.rand(n, generator=g) - 2.0)).to(dev) for n in NUMELS]
    mus = [torch.zeros_like(p) for p in ps]
    tab = torch.zeros(len(NUMELS), 12, dtype=torch.int64)
    chunks = []
    for i, n in enumerate(NUMELS):
        tab[i, 0], tab[i, 1], tab[i, 2], tab[i, 5], tab[i, 6], tab[i, 7] = ps[i].data_ptr(), gs[i].data_ptr(), mus[i].data_ptr(), n, i % 2, int(i != NO_GRAD)
        chunks += [(i, c) for c in range(-(-n // 4096))]
    return ps, gs, mus, tab.to(dev), torch.tensor(chunks, dtype=torch.int32).to(dev), len(chunks)


@pytest.mark.parametrize("stats", [1, 3])
def test_ordered_norm_statistics(ops, stats):
    """head vs fp64 within (32 + chunks_t) 2^-24 of the sum of the absolute terms (for sum g^2 and sum p^2 that is the statistic itself):
    one rounding per product, at most 16 + 10 additions in the chunk, at most chunks_t - 1 in the fold (include/esvit_hip.h)"""
    dev = _dev()
    assert ops.update_chunk_elems() == 4096
    ps, gs, mus, tab, chunks, nchunks = _stat_tables(dev, 21)
    nt = len(NUMELS)
    buf = torch.full((2 * MOAT + (nt + nchunks) * stats,), SENTINEL, dtype=torch.float32, device=dev)
    sq = buf[MOAT:MOAT + (nt + nchunks) * stats]
    ops.grad_sqnorm(tab, nt, chunks, nchunks, sq, stats=stats, ordered=True)
    head = sq[:nt * stats].clone()
    assert bool((buf[:MOAT] == SENTINEL).all()) and bool((buf[-MOAT:] == SENTINEL).all())
    got = head.cpu().double().view(nt, stats)
    for i, n in enumerate(NUMELS):
        g, p = gs[i].cpu().double(), ps[i].cpu().double()
        terms = [g * g, p * p, g * p][:stats]
        for k, t in enumerate(terms):
            if i == NO_GRAD:
                assert got[i, k] == 0.0
                continue
            lim = (32 + -(-n // 4096)) * U * float(t.abs().sum())
            err = abs(float(got[i, k]) - float(t.sum()))
            print("stats", stats, "numel", n, "k", k, "err / bound", err / lim)
            assert err <= lim, (n, k, err, lim)
    for _ in range(9):
        sq.fill_(7.0)  # (whatever the buffer held: no memset is needed)
        ops.grad_sqnorm(tab, nt, chunks, nchunks, sq, stats=stats, ordered=True)
        assert torch.equal(sq[:nt * stats], head)
    # the default form agrees to its own (atomic) order
    plain = torch.zeros(nt * stats, dtype=torch.float32, device=dev)
    ops.grad_sqnorm(tab, nt, chunks, nchunks, plain, stats=stats)
    assert torch.allclose(plain, head, rtol=1e-5, atol=0.0)
    # esvit_fused_clip_update_ema reads the head whether or not the partials follow it
    rule, h1, h2 = (ops.RULE_SGD, 0.9, 0.0) if stats == 1 else (ops.RULE_LARS, 0.9, 0.001)
    res = []
    for stat_buf in (sq, head.clone()):
        ps2, gs2, mus2, tab2, _, _ = _stat_tables(dev, 21)
        ops.fused_clip_update_ema(rule, tab2, nt, chunks, nchunks, stat_buf, 3.0, 0.1, 0.05, h1, h2, 1e-8, 0.99)
        res.append((ps2, mus2))
        torch.cuda.synchronize()
    for a, b, p0 in zip(res[0][0] + res[0][1], res[1][0] + res[1][1], ps + mus):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][0][-1], ps[-1]) and torch.equal(res[0][0][NO_GRAD], ps[NO_GRAD])


# ---- the whole step ---------------------------------------------------------------------------------------------------------------------
VIL_ARCH = 'l1,h1,d32,n1,s1,g1,p4,f7_l2,h2,d64,n1,s1,g1,p2,f7_l3,h2,d64,n2,s0,g1,p2,f7_l4,h2,d64,n1,s0,g0,p2,f7'  # (tests/test_composition_cpu.py)
SWIN96 = dict(embed_dim=96, depths=(2, 2), heads=(3, 6), window=7)
STEP_CASES = ["swin_w7", "swin_w14", "swin96", "swin96_bwd_fused", "cvt_rpe", "cvt_rpe_ragged", "vit", "vil", "swin_w7_lars"]


def _heads(m, fea):
    from esvit_amd import models
    hk = dict(hidden_dim=GU.NANO_HEAD["hidden_dim"], bottleneck_dim=GU.NANO_HEAD["bottleneck_dim"])
    m.head = models.DINOHead(fea, GU.NANO_HEAD["out_dim"], norm_last_layer=True, **hk)
    m.head_dense = models.DINOHead(fea, GU.NANO_HEAD["out_dim"], norm_last_layer=False, **hk)
    return m


def _build_net(case, teacher):
    import esvit_amd
    from esvit_amd import config as CFG
    from esvit_amd import models
    from oracle import ref_loader as RL
    if case.startswith("swin"):
        spec = SWIN96 if case.startswith("swin96") else dict(GU.NANO, window=14 if case == "swin_w14" else 7)
        cfg = RL.swin_config(embed_dim=spec["embed_dim"], depths=spec["depths"], heads=spec["heads"], window=spec["window"], drop_path=0.1)
        m = models.build_model(cfg, is_teacher=teacher, use_dense_prediction=True)
        return _heads(m, m.num_features)
    if case.startswith("cvt"):
        c = GU.NANO_CVT_VARIANTS["rpe"]
        m = models.build_model(RL.cvt_config(drop_path=0.1, **c["cfg"]), is_teacher=teacher, use_dense_prediction=True)
        return _heads(m, m.num_features)
    if case == "vit":
        from esvit_amd.models import vision_transformer as V
        v = GU.NANO_VIT
        m = V.VisionTransformer(img_size=[v["sizes"][0]], patch_size=v["patch"], embed_dim=v["embed_dim"], depth=v["depth"], num_heads=v["heads"],
                                mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), drop_path_rate=0.0 if teacher else 0.1,
                                use_dense_prediction=True)
        return _heads(m, v["embed_dim"])
    assert case == "vil"
    m = esvit_amd.build_model(CFG.vil_config("vil_tiny", arch=VIL_ARCH, DROP_PATH=0.1), is_teacher=teacher, use_dense_prediction=True)
    return _heads(m, m.num_features)


def _crop_sizes(case):
    if case.startswith("cvt"):
        return GU.NANO_CVT_VARIANTS["rpe"]["sizes"], 2
    if case == "vit":
        return GU.NANO_VIT["sizes"], 3
    if case == "vil":
        return (112, 48), 3
    return (224, 96), 3


def run_steps(case, dev):
    """one build from torch.manual_seed(0) and three EsvitTrainer.step's on fixed crops at B = 2 -> {name: tensor}"""
    import esvit_amd.functional as Fn
    import esvit_amd.loss as L
    from esvit_amd import params as P
    from esvit_amd.engine import EsvitTrainer
    from esvit_amd.update import FusedClipAdamWEMA
    P.clear()
    was = Fn.ATTN_BWD_FUSED
    Fn.ATTN_BWD_FUSED = case == "swin96_bwd_fused"
    try:
        torch.manual_seed(0)
        student, teacher = _build_net(case, False), _build_net(case, True)
        GU.fill_state_dict(student.state_dict(), 0)
        GU.fill_state_dict(teacher.state_dict(), 7)
        for m in (student, teacher):
            for k, v in m.state_dict().items():
                if k.endswith("running_var"):
                    v.abs_().add_(0.5)
        student.head.last_layer.weight_g.data.fill_(1)
        for p in teacher.parameters():
            p.requires_grad = False
        student, teacher = student.to(dev), teacher.to(dev)
        if case == "cvt_rpe_ragged":
            student.ragged_multi_crop = True
        sizes, n_local = _crop_sizes(case)
        crops = [c.to(dev) for c in GU.make_crops(2, n_local=n_local, seed=99, sizes=sizes)]
        loss_fn = L.DDINOLoss(GU.NANO_HEAD["out_dim"], 2 + n_local, 0.04, 0.07, 5, 10).to(dev)
        upd = FusedClipAdamWEMA(student, teacher, rule="lars") if case.endswith("lars") else None
        tr = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=1, updater=upd)
        lr = 0.05 if upd is not None else 5e-4
        losses = [tr.step(crops, lr, 0.04, 0.99, epoch=i) for i in range(3)]
        torch.cuda.synchronize()
        assert tr.updater.take_skipped() == 0
        tr.reducer.close()
        out = {"loss%d" % i: l.detach().float().clone() for i, l in enumerate(losses)}
        for tag, net in (("student", student), ("teacher", teacher)):
            for n, p in net.named_parameters():
                out["%s.%s" % (tag, n)] = p.detach().clone()
        for tag, moments in (("exp_avg", tr.updater.exp_avg), ("exp_avg_sq", tr.updater.exp_avg_sq)):
            for i, t in enumerate(moments):
                if t is not None:
                    out["%s.%d" % (tag, i)] = t.detach().clone()
        for k, v in loss_fn.state_dict().items():
            out["loss_fn." + k] = v.detach().clone()
        assert all(bool(torch.isfinite(l)) for l in losses)
        return out
    finally:
        Fn.ATTN_BWD_FUSED = was
        P.clear()


def digest(out):
    h = hashlib.sha256()
    for k in sorted(out):
        h.update(k.encode())
        h.update(out[k].detach().float().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.fixture()
def deterministic_mode(lib_built):
    import esvit_amd
    was = esvit_amd.is_deterministic()
    esvit_amd.set_precision("bf16")
    esvit_amd.set_deterministic(True)
    yield esvit_amd
    esvit_amd.set_deterministic(was)
    esvit_amd.set_precision("bf16")


def _same(a, b):
    assert a.keys() == b.keys() and len(a) > 20
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (len(bad), len(a), bad[:8])


@pytest.mark.parametrize("case", STEP_CASES)
def test_whole_step_is_bit_identical_between_two_builds(deterministic_mode, case):
    dev = _dev()
    flag = torch.are_deterministic_algorithms_enabled()
    _same(run_steps(case, dev), run_steps(case, dev))
    assert torch.are_deterministic_algorithms_enabled() == flag  # the mode never sets torch's global flag itself


@pytest.mark.parametrize("case", STEP_CASES)
def test_whole_step_under_torch_deterministic_algorithms(deterministic_mode, case):
    """torch raises on every op of its own without a deterministic form: nothing may, and the setting is put back"""
    dev = _dev()
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a = run_steps(case, dev)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert torch.are_deterministic_algorithms_enabled() == was
    assert all(bool(torch.isfinite(v.float()).all()) for v in a.values())


def test_whole_step_digest_is_the_same_in_fresh_processes(deterministic_mode):
    """two child interpreters, one after the other, each under its own time limit, print the SHA-256 of the step's tensors"""
    want = digest(run_steps("swin_w7", _dev()))
    env = dict(os.environ, ESVIT_DETERMINISTIC="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = ("import torch, esvit_amd\n"
            "from tests.test_deterministic_gpu import digest, run_steps\n"
            "assert esvit_amd.is_deterministic()\n"
            "esvit_amd.set_precision('bf16')\n"
            "print('DIGEST', digest(run_steps('swin_w7', torch.device('cuda:0'))))\n")
    got = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        got.append([l.split()[1] for l in r.stdout.splitlines() if l.startswith("DIGEST")][0])
    assert got[0] == got[1] == want, (got, want)


def test_mode_on_computes_the_same_step_as_mode_off(deterministic_mode):
    """a sanity check, not a precision claim: same seed, the three losses agree to 1e-5 relative"""
    dev = _dev()
    on = run_steps("swin_w7", dev)
    deterministic_mode.set_deterministic(False)
    off = run_steps("swin_w7", dev)
    for i in range(3):
        a, b = on["loss%d" % i].item(), off["loss%d" % i].item()
        assert abs(a - b) <= 1e-5 * abs(b), (i, a, b)
