"""-m gpu: the relative-position-bias gradient of the 224-slot window kernels at head_dim 64 (attn_big_bwd_dbias_kernel,
csrc/window_attn_big.hip), from the kernel up to the CvT / Swin models that need it (res_stem/s1_rpe_w14.yaml).

Kernel level: the reference is the fp64 autograd statement `attention64` below, evaluated on the same bf16-rounded inputs.  Per table
entry e = |dt - dt64| / sum |dS64 contributions to that entry|.  The yardstick is the EXISTING head_dim-32 path (dq4) on the twin
problem -- the same tensors read as 2 nH heads of 32 channels, a table of 2 nH columns -- and the requirement is
max e (head_dim 64) <= 3 x max e (head_dim 32) of the same case: 3 is the project's convention for bf16 bounds and also covers the
twice-longer dot products, whose fp32-accumulated error grows at most linearly.  Every run writes the figures to
profiles/rpe_hd64_parity_observed.jsonl (and beside golden_utils.record_parity's file when its directory exists)."""
import json
import os

import pytest
import torch

from oracle import esvit_oracle as O
from oracle import ref_loader as RL
from tests import golden_utils as GU
from tests.test_composition_cpu import check_cvt_variant, check_nano_cvt
from tests.test_oracle_cpu import GOLD
from tests.test_rpe_hd64_cpu import load_fixture, nano_pair, run_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = [os.path.join(ROOT, "profiles", "rpe_hd64_parity_observed.jsonl"), os.path.join(os.path.dirname(GU.PARITY_OBSERVED), "rpe_hd64_parity_observed.jsonl")]
WS, N, NT = 14, 196, 14


@pytest.fixture(scope="module", autouse=True)
def _session(lib_built):
    import esvit_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    esvit_amd.set_precision("bf16")
    for path in OBSERVED:  # one file per run
        try:
            if os.path.isdir(os.path.dirname(path)):
                open(path, "w").close()
        except OSError:
            pass
    yield
    esvit_amd.set_precision("bf16")
    _REF.clear()
    _CASES.clear()


def record(**kw):
    line = json.dumps(kw)
    print("RPE_HD64", line)
    for path in OBSERVED:
        try:
            if os.path.isdir(os.path.dirname(path)):
                with open(path, "a") as fh:
                    fh.write(line + "\n")
        except OSError:
            pass


def dev():
    return torch.device("cuda:0")


# ---- cases (all ws = 14, N = 196); nH counts head_dim-64 heads, the twin reads the same columns as 2 nH heads of 32 -------------------
# name: (map side, shift, images, heads, zero every other dout row)
CASES = {
    "a_one_window_Bw_lt_parts": (14, 0, 3, 1, False),       # Bw = 3 < parts
    "b_130_windows_8_heads": (14, 0, 130, 8, False),        # parts = 64: three iterations, the last with two live parts
    "c_shifted_28": (28, 7, 2, 2, False),                   # four windows per image, the shifted-window region ids
    "d_map24_padded_to_28": (24, 7, 2, 2, False),           # -1 slots: whole query tiles without a live slot, pad keys
    "d_map6_in_one_window": (6, 0, 3, 2, False),            # 36 live slots of 196
    "e_zero_dout_rows": (14, 0, 4, 2, True),
}
_CASES, _REF = {}, {}


def make_case(name):
    if name in _CASES:
        return _CASES[name]
    from esvit_amd import ops
    H, shift, nB, nH, zero_rows = CASES[name]
    C, L = 64 * nH, H * H
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    bf = lambda t: t.to(torch.bfloat16)  # noqa: E731
    c = dict(name=name, H=H, L=L, nB=nB, C=C, nH64=nH,
             w2t=torch.from_numpy(ops.window_maps(H, H, WS, shift)[0]).to(dev()),
             regions=torch.from_numpy(ops.shift_region_ids(H, H, WS, shift)).to(dev()) if shift else None,
             qkv=bf(torch.randn(nB * L, 3 * C, generator=g)).to(dev()),
             qb=bf(0.5 * torch.randn(3 * C, generator=g)).float().to(dev()),  # (bf16-representable: a pad slot holds it as bf16)
             dout=bf(torch.randn(nB * L, C, generator=g)).to(dev()),
             table2=(0.2 * torch.randn((2 * WS - 1) ** 2, 2 * nH, generator=g)).to(dev()),
             index=torch.from_numpy(ops.relative_position_index(WS)).to(dev()))
    if zero_rows:
        c["dout"][::2] = 0
    c["nW"] = c["w2t"].numel() // N
    _CASES[name] = c
    return c


def table_of(c, hd):
    return c["table2"] if hd == 32 else c["table2"][:, :c["nH64"]].contiguous()


def attention64(c, hd):
    """the fp64 statement: windows gathered by win2tok (a -1 slot holds the qkv bias of its head), bias = table[index], -100 where the
    region ids differ, softmax, P V; the table gradient by autograd.  -> out [nB*L, C], d table [rows, nH], sum |dS| per table entry
    [rows, nH], |dS| [Bw, nH, N, N] (float32)"""
    key = (c["name"], hd)
    if key in _REF:
        return _REF[key]
    nB, L, C, nW = c["nB"], c["L"], c["C"], c["nW"]
    nH = C // hd
    w = c["w2t"].long()
    live = (w >= 0)

    def windows(x, fill):  # token rows [nB*L, ch] -> [nB, nW*N, ch]
        xw = x.double().view(nB, L, -1)[:, w.clamp(min=0)]
        return torch.where(live[None, :, None], xw, fill.double()[None, None, :].expand_as(xw))

    q, k, v = windows(c["qkv"], c["qb"]).view(nB * nW, N, 3, nH, hd).permute(2, 0, 3, 1, 4)
    do = windows(c["dout"], torch.zeros(C, device=dev())).view(nB * nW, N, nH, hd).permute(0, 2, 1, 3)
    tab = table_of(c, hd).double().requires_grad_(True)
    idx = c["index"].view(-1)
    s = (q * hd ** -0.5) @ k.transpose(-1, -2) + tab[idx].view(N, N, nH).permute(2, 0, 1)[None]
    if c["regions"] is not None:
        r = c["regions"].view(nW, N)
        mask = (r[:, :, None] != r[:, None, :]).double() * -100.0
        s = (s.view(nB, nW, nH, N, N) + mask[None, :, None]).view(nB * nW, nH, N, N)
    p = torch.softmax(s, -1)
    o = p @ v
    (dt,) = torch.autograd.grad((o * do).sum(), tab)
    with torch.no_grad():
        p = p.detach()
        dp = do @ v.transpose(-1, -2)
        ds = (p * (dp - (p * dp).sum(-1, keepdim=True))).abs()  # (zero rows where dout is zero: pad-slot and zeroed queries)
        den = torch.zeros_like(dt).index_add_(0, idx, ds.sum(0).permute(1, 2, 0).reshape(N * N, nH))
        out = torch.zeros(nB, L, C, dtype=torch.float64, device=dev())
        ow = o.detach().permute(0, 2, 1, 3).reshape(nB, nW * N, C)
        out[:, w[live]] = ow[:, live]
    res = dict(out=out.view(nB * L, C), dt=dt.detach(), den=den, ds_abs=ds.float())
    _REF[key] = res
    return res


def run_kernels(c, hd, want_dbias=True, ws_flags=0, dbias_out=None):
    from esvit_amd import ops
    nH = c["C"] // hd
    table = table_of(c, hd)
    o, lse = ops.window_attn_fwd(c["qkv"], c["qb"], c["w2t"], c["L"], table, WS, c["regions"], c["nW"], N, nH, hd ** -0.5)
    dqkv, slabs, pad = ops.window_attn_bwd(c["qkv"], c["qb"], c["w2t"], c["L"], c["dout"], o, lse, table, WS | ws_flags, c["regions"], c["nW"], N, nH,
                                           hd ** -0.5, want_dbias=want_dbias, dbias_out=dbias_out)
    return o, dqkv, slabs, pad


def table_error(c, hd, slabs):
    """max over the table entries of |dt - dt64| / sum |dS64|; an entry no (live query, key) pair maps to must come out as exactly 0"""
    from esvit_amd import ops
    ref = attention64(c, hd)
    dt = ops.relpos_bias_bwd(slabs, c["index"], N, ref["dt"].shape[0]).double()
    assert bool(torch.isfinite(dt).all())
    used = ref["den"] > 0
    assert bool((dt[~used] == 0).all()), "a table entry without contributions received a gradient"
    return ((dt - ref["dt"]).abs()[used] / ref["den"][used]).max().item()


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_gradient_at_head_dim_64_within_3x_of_the_head_dim_32_kernel(name):
    c = make_case(name)
    _, _, slabs64, _ = run_kernels(c, 64)
    _, _, slabs32, _ = run_kernels(c, 32)
    e64, e32 = table_error(c, 64, slabs64), table_error(c, 32, slabs32)
    record(test="table_gradient", case=name, e_hd64=e64, e_hd32=e32, ratio=e64 / e32)
    assert e64 <= 3 * e32, (name, e64, e32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_with_a_table_at_head_dim_64_within_3x_of_head_dim_32(name):
    """the head_dim-64 forward of the 224-slot kernels with a NON-zero table (the ViTs, its only users so far, pass zeros):
    max |out - out64| / max |out64| against the twin's"""
    c = make_case(name)
    err = {}
    for hd in (64, 32):
        ref = attention64(c, hd)["out"]
        o = run_kernels(c, hd)[0].double()
        assert bool(torch.isfinite(o).all())
        err[hd] = ((o - ref).abs().max() / ref.abs().max()).item()
    record(test="forward", case=name, e_hd64=err[64], e_hd32=err[32], ratio=err[64] / err[32])
    assert err[64] <= 3 * err[32], (name, err)


def _dense_index():
    """[N, N] positions of (query, key) in the fragment-order slab: ((ki * NT + qj) * 64 + lane) * 4 + r, lane = 16 g + c"""
    t = torch.arange(N, device=dev())
    q, k = t[:, None], t[None, :]
    return ((k // 16 * NT + q // 16) * 64 + (k % 16) // 4 * 16 + q % 16) * 4 + k % 4


@pytest.mark.parametrize("name", ["b_130_windows_8_heads", "c_shifted_28", "d_map24_padded_to_28", "d_map6_in_one_window"])
def test_head_dim_32_instance_of_the_new_kernel_matches_dq4(name):
    """ws | ATTN_SPLIT_DBIAS at head_dim 32: dq4 runs, then the new kernel writes the slabs.  Same window order per wave and the same
    arithmetic, so a slab element may differ from dq4's by at most one extra rounding per term (a differently fused multiply-add):
    4 * 2^-24 * sum |dS| over the windows of its part"""
    from esvit_amd import ops
    c = make_case(name)
    _, dq_a, a, pad_a = run_kernels(c, 32)
    _, dq_b, b, pad_b = run_kernels(c, 32, ws_flags=ops.ATTN_SPLIT_DBIAS)
    assert torch.equal(dq_a, dq_b) and torch.equal(pad_a, pad_b)
    assert bool(torch.isfinite(b).all())
    parts, nH = a.shape[0], a.shape[1]
    ds = attention64(c, 32)["ds_abs"]  # [Bw, nH, N, N]
    Bw = ds.shape[0]
    iters = -(-Bw // parts)
    ds = torch.cat([ds, ds.new_zeros((iters * parts - Bw,) + ds.shape[1:])]).view(iters, parts, nH, N, N).sum(0)
    idx = _dense_index().view(-1)
    diff = (a[:, :, idx] - b[:, :, idx]).abs().view(parts, nH, N, N)
    bound = 4 * 2.0 ** -24 * ds
    worst = (diff / bound.clamp(min=1e-30)).max().item()
    record(test="split_vs_dq4", case=name, worst_over_bound=worst, identical=bool(torch.equal(a, b)))
    assert bool((diff <= bound).all()), (name, worst)
    rest = torch.ones(a.shape[2], dtype=torch.bool, device=dev())
    rest[idx] = False
    assert bool((b[:, :, rest] == 0).all())  # slots beyond N carry no gradient


def test_dqkv_and_pad_slab_do_not_depend_on_want_dbias():
    for name in ("b_130_windows_8_heads", "d_map24_padded_to_28"):
        c = make_case(name)
        _, dq_a, slabs, pad_a = run_kernels(c, 64)
        _, dq_b, none, pad_b = run_kernels(c, 64, want_dbias=False)
        assert none is None and slabs is not None
        assert torch.equal(dq_a, dq_b) and torch.equal(pad_a, pad_b)


def test_slabs_are_bit_reproducible_and_fully_written():
    from esvit_amd import ops
    c = make_case("b_130_windows_8_heads")
    _, _, first, _ = run_kernels(c, 64)
    _, _, second, _ = run_kernels(c, 64)
    assert torch.equal(first, second)
    for name in ("b_130_windows_8_heads", "d_map6_in_one_window"):  # (d: tiles that never meet a live query write their zeros)
        c = make_case(name)
        parts = ops.query(ops.Q_ATTN_BWD_PARTS, N, c["nB"] * c["nW"], c["nH64"])
        buf = torch.full((parts, c["nH64"], ops.attn_frag_elems(N)), float("nan"), device=dev())
        _, _, slabs, _ = run_kernels(c, 64, dbias_out=buf)
        assert slabs.data_ptr() == buf.data_ptr() and not bool(torch.isnan(buf).any())
        assert torch.equal(buf, run_kernels(c, 64)[2])


def test_null_slabs_are_refused_where_a_kernel_would_write_them():
    from esvit_amd import ops
    c = make_case("a_one_window_Bw_lt_parts")
    o, lse = ops.window_attn_fwd(c["qkv"], c["qb"], c["w2t"], c["L"], table_of(c, 32), WS, None, 1, N, 2, 32 ** -0.5)
    sentinel = torch.full_like(c["qkv"], 7.0)
    with pytest.raises(RuntimeError, match="dbias_ws may be NULL only"):
        ops.window_attn_bwd(c["qkv"], c["qb"], c["w2t"], c["L"], c["dout"], o, lse, table_of(c, 32), WS, None, 1, N, 2, 32 ** -0.5, dqkv_out=sentinel,
                            want_dbias=False)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())  # refused before any launch
    # 7x7 windows at head_dim 64: the <= 64-token kernel writes its slabs unconditionally
    w2t = torch.from_numpy(ops.window_maps(7, 7, 7, 0)[0]).to(dev())
    qkv, dout = c["qkv"][:49 * 2, :192].contiguous(), c["dout"][:49 * 2, :64].contiguous()
    with pytest.raises(RuntimeError, match="dbias_ws may be NULL only"):
        ops.window_attn_bwd(qkv, c["qb"][:192].contiguous(), w2t, 49, dout, None, None, torch.zeros(169, 1, device=dev()), 7, None, 1, 49, 1, 0.125, want_dbias=False)
    with pytest.raises(RuntimeError, match="ATTN_SPLIT_DBIAS"):
        ops.window_attn_bwd(qkv, c["qb"][:192].contiguous(), w2t, 49, dout, None, None, torch.zeros(169, 1, device=dev()), 7 | ops.ATTN_SPLIT_DBIAS, None, 1, 49, 1,
                            0.125)
    hdr = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "#define ESVIT_ATTN_SPLIT_DBIAS 0x%x" % ops.ATTN_SPLIT_DBIAS in hdr
    assert ops.ATTN_SPLIT_DBIAS & (ops.ATTN_GLOBAL | ops.ATTN_SLIDING_CHUNK) == 0 and ops.ATTN_SPLIT_DBIAS > 0xffff


def test_vit_backward_at_197_tokens_asks_for_no_bias_gradient(monkeypatch):
    import esvit_amd.functional as Fn
    from esvit_amd import ops
    seen = []
    orig = ops.window_attn_bwd
    monkeypatch.setattr(ops, "window_attn_bwd", lambda *a, **k: (seen.append(k.get("want_dbias", True)), orig(*a, **k))[1])
    nB, T, nH, C = 3, 197, 2, 128
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(nB * T, 3 * C, generator=g).to(torch.bfloat16).to(dev())
    bqkv = (0.1 * torch.randn(3 * C, generator=g)).to(dev())
    dao = torch.randn(nB * T, C, generator=g).to(torch.bfloat16).to(dev())
    ao, att = Fn.vit_attention(Fn.ops_module(), qkv, bqkv, nB, T, nH, 0.125, True)
    dqkv = Fn.vit_attention_bwd(Fn.ops_module(), dao, att, bqkv, nB, T, nH, 0.125)
    assert seen == [False] and bool(torch.isfinite(dqkv.float()).all())
    # 37 tokens run in the <= 64-token kernel, which always writes its slabs
    seen.clear()
    qkv, dao = qkv[:nB * 37].contiguous(), dao[:nB * 37].contiguous()
    ao, att = Fn.vit_attention(Fn.ops_module(), qkv, bqkv, nB, 37, nH, 0.125, True)
    Fn.vit_attention_bwd(Fn.ops_module(), dao, att, bqkv, nB, 37, nH, 0.125)
    assert seen == [True]


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def _probe_rel_l2(t, p):
    """relative L2 error over the entries a golden_utils.probe keeps of a tensor"""
    q = GU.probe(t)
    got, ref = torch.cat([q["head"], q["strided"]]), torch.cat([p["head"], p["strided"]])
    return _rel_l2(got, ref)


def test_nano_cvt_rpe_w14_step_matches_reference_golden():
    """one step of the nano case through the HIP path in bf16 against the reference's fixture: loss, outputs, gradient norms and
    BatchNorm buffers under the bf16 bounds tests/test_step_gpu.py gives the CvT variants; the three table gradients element-wise, as
    relative L2 error, within 3 x the larger error the `rpe` (7x7, head_dim 64) and `res_stem` (14x14, head_dim 32) variants show in
    this session -- for their tables, for `res_stem` (no table) its qkv weights -- over the entries their fixtures keep"""
    import esvit_amd.loss as L
    g = load_fixture()
    yard = {}
    variants = torch.load(os.path.join(GOLD, "nano_cvt_variants.pt"), weights_only=False)
    for name, pick in (("rpe", "rel_pos_bias_table"), ("res_stem", "qkv.pw.weight")):
        student = check_cvt_variant(name, L, dev=dev(), rt=6e-2, loss_tol=3e-3, grad_tol=0.08, buf_tol=2e-2, probes=False)
        errs = {n: _probe_rel_l2(p.grad.float().cpu(), variants[name]["grads"][n]) for n, p in student.named_parameters() if pick in n}
        assert errs
        yard[name] = max(errs.values())
    student, teacher = nano_pair(g["case"], dev())
    s_out, t_out, loss = run_step(g["case"], student, teacher, L, dev())
    got = dict(student.named_parameters())
    errs = {n: _rel_l2(got[n].grad.float().cpu(), ref) for n, ref in g["table_grads"].items()}
    record(test="nano_cvt_rpe_w14", loss_err=abs(loss.item() - g["ddino_loss"]), table_rel_l2=errs, yardstick_rpe=yard["rpe"], yardstick_res_stem=yard["res_stem"])
    check_nano_cvt(g, student, s_out, t_out, loss, rt=6e-2, loss_tol=3e-3, grad_tol=0.08, buf_tol=2e-2)
    bound = 3 * max(yard.values())
    for n, e in errs.items():
        assert e <= bound, (n, e, yard)


SWIN64 = dict(embed_dim=64, depths=(2, 2, 2, 2), heads=(1, 2, 4, 8), window=14, img=224)


def _swin_table_deltas(cfg, ragged):
    """relative L2 error of every relative-position-table gradient of a nano Swin (crops 224 / 96, B = 1, two local crops) against
    oracle.esvit_oracle.swin_multicrop on the same weights"""
    import esvit_amd.loss as L
    from esvit_amd import models
    K = GU.NANO_HEAD["out_dim"]
    hk = dict(hidden_dim=GU.NANO_HEAD["hidden_dim"], bottleneck_dim=GU.NANO_HEAD["bottleneck_dim"])

    def make(teacher):
        m = models.build_model(RL.swin_config(embed_dim=cfg["embed_dim"], depths=cfg["depths"], heads=cfg["heads"], window=cfg["window"]),
                               is_teacher=teacher, use_dense_prediction=True)
        m.head = models.DINOHead(m.num_features, K, norm_last_layer=True, **hk)
        m.head_dense = models.DINOHead(m.num_features, K, norm_last_layer=False, **hk)
        GU.fill_state_dict(m.state_dict(), 7 if teacher else 0)
        return m

    student, teacher = make(False), make(True)
    student.head.last_layer.weight_g.data.fill_(1)
    for p in teacher.parameters():
        p.requires_grad = False
    key = (cfg["embed_dim"],)
    if key not in _REF:  # the oracle's gradients: once per model, shared by the two routes
        sd = {k: v.clone() for k, v in student.state_dict().items()}
        tsd = {k: v.clone() for k, v in teacher.state_dict().items()}
        crops = GU.make_crops(1, n_local=2)
        leaf = {n: sd[n].clone().requires_grad_(True) for n, p in student.named_parameters() if "relative_position_bias_table" in n}
        full = dict(sd)
        full.update(leaf)
        s_ref = O.swin_multicrop(full, crops, cfg)
        with torch.no_grad():
            t_ref = O.swin_multicrop(tsd, crops[:2], cfg)
        c0 = torch.zeros(1, K)
        l_ref, _, _ = O.ddino_loss(s_ref, t_ref, c0, c0, O.teacher_temp(0, 0.04, 0.04, 0, 1), 4)
        l_ref.backward()
        _REF[key] = (l_ref.item(), {n: t.grad.clone() for n, t in leaf.items()})
    l_ref, g_ref = _REF[key]
    student, teacher = student.to(dev()), teacher.to(dev())
    student.ragged_multi_crop = ragged
    crops = [c.to(dev()) for c in GU.make_crops(1, n_local=2)]
    loss_fn = L.DDINOLoss(K, 4, 0.04, 0.04, 0, 1).to(dev())
    with torch.no_grad():
        t_out = teacher(crops[:2])
    s_out = student(crops)
    loss = loss_fn(s_out, t_out, 0, None)
    loss.backward()
    got = dict(student.named_parameters())
    assert all(bool(torch.isfinite(p.grad).all()) for p in got.values() if p.grad is not None)
    return abs(loss.item() - l_ref), {n: _rel_l2(got[n].grad.float().cpu(), r) for n, r in g_ref.items()}


@pytest.mark.parametrize("ragged", [False, True], ids=["per_group", "ragged"])
def test_swin_w14_head_dim_64_table_gradients_within_3x_of_head_dim_32(ragged):
    """the nano W = 14 Swin at embed_dim 64 (head_dim 64: shift masks, and pad slots in the 96^2 groups) against the oracle; its table
    gradients within 3 x the deltas of the existing NANO14 model (head_dim 32) against the same oracle, measured here"""
    loss32, d32 = _swin_table_deltas(dict(GU.NANO14), ragged)
    loss64, d64 = _swin_table_deltas(SWIN64, ragged)
    record(test="swin_w14", route="ragged" if ragged else "per_group", loss_err_hd64=loss64, loss_err_hd32=loss32, table_rel_l2_hd64=d64, table_rel_l2_hd32=d32)
    assert loss64 < 3e-3, loss64  # (the bf16 loss bound of the nano steps)
    bound = 3 * max(d32.values())
    for n, e in d64.items():
        assert e <= bound, (n, e, bound)


def test_full_s1_rpe_w14_trains_one_step():
    """res_stem/s1_rpe_w14.yaml at full width, B = 2, the two 224^2 crops (a 96^2 crop's first map is 12x12, smaller than the window:
    the reference fails on its bias shape and so do we): one trainer step -- finite loss, a finite gradient for every parameter, no
    table gradient all zero"""
    import esvit_amd
    from esvit_amd import config as CFG
    from esvit_amd.engine import EsvitTrainer
    K = GU.NANO_HEAD["out_dim"]
    hk = dict(hidden_dim=GU.NANO_HEAD["hidden_dim"], bottleneck_dim=GU.NANO_HEAD["bottleneck_dim"])
    cfg = CFG.cvt_config("cvt_s1", REL_POS_EMBED=True, RES_STEM=True, WINDOW_SIZE=[14, 14, 14, 7], DROP_PATH_RATE=0.0)

    def make(teacher):
        m = esvit_amd.build_model(cfg, is_teacher=teacher, use_dense_prediction=False)
        m.head = esvit_amd.DINOHead(m.num_features, K, **hk)
        return m

    student, teacher = make(False), make(True)
    GU.fill_state_dict(student.state_dict(), 0)
    for k, v in student.state_dict().items():
        if k.endswith("running_var"):
            v.abs_().add_(0.5)
    teacher.load_state_dict(student.state_dict())
    student, teacher = student.to(dev()), teacher.to(dev())
    for p in teacher.parameters():
        p.requires_grad = False
    with pytest.raises(RuntimeError, match="smaller than"):
        with torch.no_grad():
            student([torch.randn(1, 3, 96, 96, device=dev())])
    # (the view-level loss: the region-level one indexes the patch count of a second resolution, as main_esvit.py:710 does)
    loss_fn = esvit_amd.DINOLoss(K, 2, 0.04, 0.04, 0, 10).to(dev())
    trainer = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=0)
    grads = {}
    step0 = trainer.updater.step

    def snapshot(*a, **k):  # the gradients as the update sees them (the trainer clears them afterwards)
        for n, p in student.named_parameters():
            grads[n] = None if p.grad is None else (bool(torch.isfinite(p.grad).all()), p.grad.abs().max().item())
        return step0(*a, **k)

    trainer.updater.step = snapshot
    crops = [c.to(dev()) for c in GU.make_crops(2, n_local=0)]
    loss = trainer.step(crops, 5e-4, 0.04, 0.996, epoch=1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)), loss
    missing = [n for n, p in student.named_parameters() if p.requires_grad and grads.get(n) is None]
    assert not missing, missing
    grads = {n: v for n, v in grads.items() if v is not None}  # (parameters outside the graph keep none, trainable ones were checked above)
    assert all(fin for fin, _ in grads.values()), [n for n, (fin, _) in grads.items() if not fin]
    tables = {n: mx for n, (_, mx) in grads.items() if "rel_pos_bias_table" in n}
    assert len(tables) == 12 and all(mx > 0 for mx in tables.values()), tables
    record(test="full_s1_rpe_w14", loss=loss.item(), table_grad_absmax_min=min(tables.values()), table_grad_absmax_max=max(tables.values()))
