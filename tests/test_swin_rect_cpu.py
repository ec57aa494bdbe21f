"""Swin backbones on H x W images, without a GPU: the fp64 statement tests/swin_rect_ref.py against the oracle and the reference's
fixture on square inputs, then the model -- host logic of esvit_amd.models.swin_transformer / functional over the CPU restatement of
the kernels (oracle/ops_ref.py, which has no pad mode: the copy route) -- against the statement on rectangles; crop grouping; the
helpers feature_grid / swin_window_to_grid; the refusals of ESVIT_MERGE_PAD; and the statement's mutants."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import esvit_oracle as O
from oracle import ops_ref
from oracle import ref_loader as RL
from tests import golden_utils as GU
from tests import swin_rect_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECT = [(112, 80), (60, 100), (100, 60), (4, 36)]  # image (H, W); the last: a 1 x 9 grid, one token row, odd at every merge
TOL = 2e-5       # tests/test_variants.py:test_odd_patch_merging_host_logic_cpu: outputs; five times that for gradients
SEED = 23


@pytest.fixture()
def cpu_ops(monkeypatch, lib_built):
    import esvit_amd
    import esvit_amd.functional as Fn
    import esvit_amd.params as P
    esvit_amd.set_precision("fp32")
    for mod in (Fn, P):
        monkeypatch.setattr(mod, "ops", ops_ref)
    ops_ref.set_act_dtype(torch.float32)
    P.clear()
    Fn._GEOM.clear()
    yield ops_ref
    ops_ref.set_act_dtype(torch.float32)
    P.clear()
    Fn._GEOM.clear()
    esvit_amd.set_precision("bf16")


def build(cfg, seed=SEED, **kw):
    from esvit_amd import models
    c = RL.swin_config(embed_dim=cfg["embed_dim"], depths=cfg["depths"], heads=cfg["heads"], window=cfg["window"], img=cfg.get("img", 224))
    for k, v in kw.items():
        c.MODEL["SPEC"][k] = v
    m = models.build_model(c, is_teacher=False, use_dense_prediction=True)
    GU.fill_state_dict(m.state_dict(), seed)
    return m


def inputs(H, W, nf, B=2):
    g = torch.Generator().manual_seed(1000 * H + W)
    return torch.randn(B, 3, H, W, generator=g), torch.randn(B, nf, generator=g)


def statement(cfg, H, W, m, mut=None, name="nano"):
    x, pr = inputs(H, W, m.num_features)
    return SR.run((name, H, W, mut), m.state_dict(), x, cfg, pr, mut)


def model_run(m, x, pr):
    m.zero_grad()
    cls, region = m.forward_features(x)
    SR.loss_of(cls, region, pr).backward()
    return cls.detach(), region.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


# ---- the statement on square inputs --------------------------------------------------------------------------------------------------
def test_statement_equals_oracle_on_square_inputs():
    """forward and backward of the statement against oracle/esvit_oracle.py, both in fp64: a 64^2 image under a model built for 64^2
    (grids 16, 8, 4, 2; windows 7 shifted, 7 shifted, 4, 2) and a 224^2-built model on 56^2 (14 -> 7: padded windows, even merges)"""
    for cfg, S in ((dict(GU.NANO, img=64), 64), (dict(GU.NANO, depths=(2, 2), heads=(1, 2), img=224), 56)):
        m = build(cfg)
        x, pr = inputs(S, S, m.num_features)
        want = SR.run(("anchor", S, len(cfg["depths"])), m.state_dict(), x, cfg, pr)
        p = SR.to64(m.state_dict(), grad=True)
        cls, region = O.swin_features(p, x.double(), cfg)
        SR.loss_of(cls, region, pr).backward()
        assert SR.rel(cls, want["cls"]) < 1e-12 and SR.rel(region, want["region"]) < 1e-12
        for n, g in want["grads"].items():
            assert SR.rel(p[n].grad, g) < 1e-12, n


def test_statement_equals_the_reference_fixture_on_an_odd_square_map():
    """tests/golden/variants.pt["oddmerge"]: the reference's own modules at 112^2 (28 -> 14 -> 7 -> 4).  The fixture was recorded in
    fp32, so the fp64 statement can meet it only to fp32 rounding: the 2e-5 / 1e-4 the model is held to against the same fixture"""
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "variants.pt"), map_location="cpu", weights_only=False)["oddmerge"]
    cfg = dict(GU.NANO, img=112)
    m = build(cfg)
    x, pr = GU.ape_inputs(m.num_features)
    got = SR.run(("oddmerge",), m.state_dict(), x, cfg, pr)
    assert got["region"].shape == gold["region"].shape and got["grids"] == [(28, 28), (14, 14), (7, 7), (4, 4)]
    assert SR.rel(gold["cls"], got["cls"]) < TOL and SR.rel(gold["region"], got["region"]) < TOL
    for n, g in gold["grads"].items():
        assert SR.rel(g, got["grads"][n]) < 5 * TOL, n


# ---- the model against the statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", RECT)
def test_model_matches_statement_fp32(cpu_ops, hw):
    H, W = hw
    m = build(GU.NANO)
    x, pr = inputs(H, W, m.num_features)
    want = statement(GU.NANO, H, W, m)
    cls, region, grads = model_run(m, x, pr)
    assert m.feature_grid(H, W) == want["grids"]
    assert region.shape == want["region"].shape
    errs = dict(cls=SR.rel(cls, want["cls"]), region=SR.rel(region, want["region"]))
    assert max(errs.values()) < TOL, errs
    assert set(grads) == set(want["grads"])
    gerr = {n: SR.rel(g, want["grads"][n]) for n, g in grads.items()}
    worst = max(gerr, key=gerr.get)
    assert gerr[worst] < 5 * TOL, (worst, gerr[worst])


def test_remainder_rows_and_columns_are_lost(cpu_ops):
    m = build(GU.NANO)
    x, _ = inputs(113, 83, m.num_features)
    with torch.no_grad():
        a = m.forward_features(x)
        b = m.forward_features(x[..., :112, :80].contiguous())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_explicit_square_grid_is_the_default(cpu_ops):
    m = build(GU.NANO)
    x = torch.randn(2, 14 * 14, 32, generator=torch.Generator().manual_seed(3))
    layer = m.layers[0]
    with torch.no_grad():
        assert torch.equal(layer.blocks[1](x, hw=(14, 14))[0], layer.blocks[1](x)[0])
        assert torch.equal(layer.downsample(x, hw=(14, 14)), layer.downsample(x))
        assert layer.downsample.out_hw == (7, 7)
        for fn in (layer.forward, lambda t, hw=None: layer.forward_with_features(t, hw=hw)[0], lambda t, hw=None: layer.forward_with_attention(t, hw=hw)[0]):
            assert torch.equal(fn(x, hw=(14, 14)), fn(x))
        with pytest.raises(ValueError, match="does not hold"):
            layer.blocks[0](x, hw=(14, 13))


def test_crops_are_grouped_by_height_and_width(cpu_ops):
    """[2 x (64, 96), 3 x (32, 96)]: the crops share their width; two groups, each equal to a call of its own"""
    g = torch.Generator().manual_seed(11)
    crops = [torch.randn(2, 3, 64, 96, generator=g) for _ in range(2)] + [torch.randn(2, 3, 32, 96, generator=g) for _ in range(3)]
    m = build(GU.NANO)
    m.head = m.head_dense = torch.nn.Identity()
    with torch.no_grad():
        want = [m.forward_feature_maps(torch.cat(crops[:2])), m.forward_feature_maps(torch.cat(crops[2:]))]
        want_cls = torch.cat([w[0] for w in want])
        want_fea = torch.cat([w[1].reshape(-1, w[1].shape[-1]) for w in want])
        for ragged in (False, True):
            m.ragged_multi_crop = ragged
            seen = []
            orig = m.forward_feature_maps_multi
            m.forward_feature_maps_multi = lambda groups, _o=orig: (seen.append([len(x) for x in groups]), _o(groups))[1]
            cls, fea, fea2, npatch = m(crops)
            m.forward_feature_maps_multi = orig
            assert npatch == [2 * 3, 1 * 3] and cls.shape == want_cls.shape and fea.shape == want_fea.shape
            if ragged:
                assert seen == [[2, 3]]
                for a, b in ((cls, want_cls), (fea, want_fea)):
                    assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()  # (tests/test_composition_cpu.py: the ragged route's figure)
            else:
                assert seen == [] and torch.equal(cls, want_cls) and torch.equal(fea, want_fea)
    assert m._even_maps([224, 96]) and not m._even_maps([224, 112])
    assert m._even_maps([(64, 96), (32, 96)]) and not m._even_maps([(64, 96), (32, 80)]) and not m._even_maps([(60, 96)])


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------
def test_feature_grid():
    m = build(GU.NANO)
    assert m.feature_grid(224, 224) == [(56, 56), (28, 28), (14, 14), (7, 7)]
    assert m.feature_grid(112, 80) == [(28, 20), (14, 10), (7, 5), (4, 3)]
    assert m.feature_grid(113, 83) == m.feature_grid(112, 80)
    assert m.feature_grid(4, 36) == [(1, 9), (1, 5), (1, 3), (1, 2)]


@pytest.mark.parametrize("geo", [(28, 20, 7, 0), (28, 20, 7, 3), (15, 25, 7, 3), (1, 9, 7, 3), (14, 14, 7, 3), (4, 3, 4, 0)])
def test_swin_window_to_grid_inverts_the_statements_partition(lib_built, geo):
    """a window-ordered tensor made by the statement's own pad / roll / partition of a labelled grid comes back as the grid, pad slots
    dropped -- through the map the kernels walk (the library's esvit_window_maps)"""
    from esvit_amd import analysis as A
    import torch.nn.functional as F
    H, W, ws, shift = geo
    B, nH = 2, 3
    lab = torch.arange(B * nH * H * W, dtype=torch.float32).view(B, nH, H, W)
    g = F.pad(lab.permute(0, 2, 3, 1), (0, 0, 0, (ws - W % ws) % ws, 0, (ws - H % ws) % ws), value=-1.0)
    if shift:
        g = torch.roll(g, shifts=(-shift, -shift), dims=(1, 2))
    vals = SR.windows_of(g, ws).permute(0, 2, 1).contiguous()  # [B * nW, nH, N]
    assert torch.equal(A.swin_window_to_grid(vals, H, W, ws, shift), lab)
    with pytest.raises(ValueError, match="swin_window_to_grid"):
        A.swin_window_to_grid(vals[:, :, :-1], H, W, ws, shift)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_pad_mode_refusals_before_any_device_call(lib_built):
    from esvit_amd import _lib, ops
    lib = _lib.lib
    fake = 0x1000
    PAD = ops.MERGE_PAD_FLAG
    assert ops.MERGE_LN_PAD is True and not getattr(ops_ref, "MERGE_LN_PAD", False)

    def fwd(H, W, x=fake, y=fake, Cc=32, nB=1, dt=None):
        return lib.esvit_merge_ln_fwd(ops.F32 if dt is None else dt, x, fake, fake, 1e-6, nB, H, W, Cc, y, fake, fake, None), lib.esvit_last_error()

    def bwd(H, W, dy=fake, dx=fake, Cc=32, nB=1, dt=None, act=None, rs=None):
        return lib.esvit_merge_ln_bwd(ops.F32 if dt is None else dt, dy, fake, fake, fake, fake, nB, H, W, Cc, dx, fake, fake, fake, act, rs, 1, 0,
                                      None), lib.esvit_last_error()

    for fn in (fwd, bwd):
        for (H, W) in ((32768, 8), (7, 32768), (40000, 3), (0, 5), (5, 0), (7, -1)):
            rc, msg = fn(PAD | H, W)
            assert rc == -1 and b"ESVIT_MERGE_PAD takes 1 <= H, W < 32768" in msg, (H, W, rc, msg)
        rc, msg = fn(PAD | 0x10000 | 7, 5)  # a stray bit beside the flag
        assert rc == -1 and b"ESVIT_MERGE_PAD" in msg
        for kw in (dict(Cc=30), dict(nB=0)):
            rc, msg = fn(PAD | 7, 5, **kw)
            assert rc == -1 and b"bad geometry" in msg
        rc, msg = fn(PAD | 7, 5, dt=7)
        assert rc == -1 and b"bad dtype" in msg
        # well-formed: past every check, refused by the runtime only (no device here) -- or launched where there is one
        assert fn(PAD | 32767, 32767)[0] != -1 or torch.cuda.is_available()
    for got in (fwd(PAD | 7, 5, x=None), fwd(PAD | 7, 5, y=None), bwd(PAD | 7, 5, dy=None), bwd(PAD | 7, 5, dx=None)):
        assert got[0] == -1 and b"null pointer" in got[1], got
    rc, msg = bwd(PAD | 7, 5, rs=fake)
    assert rc == -1 and b"rowscale scales dx_act" in msg
    # without the flag nothing changed: odd sides are still refused
    assert fwd(7, 6)[0] == -1 and b"must be even" in fwd(7, 6)[1]
    assert bwd(6, 7)[0] == -1 and b"bad geometry" in bwd(6, 7)[1]


def test_merge_pad_switch(cpu_ops, monkeypatch):
    import esvit_amd.functional as Fn
    from esvit_amd import ops
    assert Fn.MERGE_PAD == os.environ.get("ESVIT_MERGE_PAD", "copy")
    monkeypatch.setattr(Fn, "MERGE_PAD", "kernel")
    assert not Fn.merge_pad_in_kernel()  # the CPU restatement does not offer the mode: the copy route
    monkeypatch.setattr(Fn, "ops", ops)
    assert Fn.merge_pad_in_kernel()
    monkeypatch.setattr(Fn, "MERGE_PAD", "copy")
    assert not Fn.merge_pad_in_kernel()
    monkeypatch.setattr(Fn, "MERGE_PAD", "both")
    with pytest.raises(ValueError, match="copy or kernel"):
        Fn.merge_pad_in_kernel()


def test_merge_pad_environment_switch(lib_built):
    """the package reads ESVIT_MERGE_PAD at import: a fresh interpreter per value"""
    def run(val):
        env = dict(os.environ, ESVIT_MERGE_PAD=val)
        return subprocess.run([sys.executable, "-c", "import esvit_amd.functional as Fn; print(Fn.MERGE_PAD)"], cwd=ROOT, env=env,
                              capture_output=True, text=True)
    ok = run("kernel")
    assert ok.returncode == 0 and ok.stdout.strip() == "kernel", ok.stderr
    bad = run("Kernel")
    assert bad.returncode != 0 and "ESVIT_MERGE_PAD: copy or kernel, not 'Kernel'" in bad.stderr


def test_ape_refuses_another_grid(cpu_ops):
    m = build(dict(GU.NANO, depths=(2, 2, 2), heads=(1, 2, 4), img=112), USE_APE=True)
    x, _ = inputs(112, 80, m.num_features)
    with pytest.raises(ValueError, match=r"built for a 28 x 28 token grid, the image gives 28 x 20"):
        m.forward_features(x)
    with pytest.raises(ValueError, match=r"28 x 28 token grid, the image gives 16 x 16"):
        m.forward_selfattention(torch.zeros(1, 3, 64, 64))
    with torch.no_grad():
        m.forward_features(torch.zeros(1, 3, 112, 112))


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------
def test_every_mutant_is_caught_where_it_must_be():
    """a case catches a mutant when the mutant's outputs leave the statement's by more than the bound the model is held to (or have
    another shape).  Every mutant is caught by each case named for it, is NOT seen by a case that is not (there it is the statement),
    and every rectangular case catches at least one"""
    m = build(GU.NANO)
    cases = RECT + [(64, 64)]
    caught = {hw: set() for hw in cases}
    for mut in SR.MUTANTS:
        named = [hw for hw in cases if SR.catches(mut, hw[0] // SR.PATCH, hw[1] // SR.PATCH, GU.NANO)]
        assert named, mut
        for (H, W) in cases:
            want = statement(GU.NANO, H, W, m)
            x, pr = inputs(H, W, m.num_features)
            with torch.no_grad():
                cls, region, _, _ = SR.features(SR.to64(m.state_dict()), x.double(), GU.NANO, mut)
            differs = region.shape != want["region"].shape or max(SR.rel(cls, want["cls"]), SR.rel(region, want["region"])) > TOL
            assert differs == ((H, W) in named), (mut, H, W)
            if differs:
                caught[(H, W)].add(mut)
    for hw in RECT:
        assert caught[hw], hw
