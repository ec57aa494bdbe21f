"""The deterministic mode, host side (no GPU): the two flags of the header and their refusals, the switch and its environment variable,
the routing of functional / update with a recording ops module (mode off: the calls of today, mode on: `ordered=True` everywhere), the
CPU restatement untouched by the mode, and the matrix route of the square ViT crops against torch's own interpolation."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import ops_ref
from tests import golden_utils as GU
from tests.test_composition_cpu import GOLD, build_cvt_variant, cpu_ops, nano_pair, run_nano14_step, run_nano_step  # noqa: F401  (fixture)
from tests.test_vit_cpu import build_nano_vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def mode():
    """-> set_deterministic; whatever the test leaves is put back"""
    import esvit_amd
    was = esvit_amd.is_deterministic()
    yield esvit_amd.set_deterministic
    esvit_amd.set_deterministic(was)


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------
def test_header_constants_match_ops_and_collide_with_nothing(lib_built):
    from esvit_amd import ops
    raw = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    flags = {n: int(v, 16) for n, v in re.findall(r"#define (ESVIT_RELPOS_ORDERED|ESVIT_SQNORM_ORDERED) (0x[0-9a-fA-F]+)", raw)}
    assert flags == {"ESVIT_RELPOS_ORDERED": ops.RELPOS_ORDERED, "ESVIT_SQNORM_ORDERED": ops.SQNORM_ORDERED}
    # accumulate is 0 / 1 today, stats 1 / 3: the flags sit above the byte that holds them
    assert ops.RELPOS_ORDERED & 0xff == 0 and ops.RELPOS_ORDERED not in (0, 1)
    assert ops.SQNORM_ORDERED & 0xff == 0 and ops.SQNORM_ORDERED not in (1, 3) and (ops.SQNORM_ORDERED | 1) != 3
    # slab 0 is written in the ordered form: the header's prototype says so
    assert re.search(r"int esvit_relpos_bias_bwd\(float\* dbias_ws,", raw)


def test_grad_sqnorm_refuses_bad_stats_before_any_launch(lib_built):
    from esvit_amd import ops
    from esvit_amd._lib import lib
    fake = C.c_void_p(0x1000)  # never dereferenced: the argument checks come first
    for stats in (0x100, 0x102, 0x104, 0, 2, 4):
        assert lib.esvit_grad_sqnorm(fake, 1, fake, 1, stats, fake, None) == -1, hex(stats)  # ESVIT_ERR_ARG
        assert lib.esvit_last_error()
    assert ops.SQNORM_ORDERED == 0x100


def test_switch_is_parsed_from_the_environment():
    code = "import esvit_amd; print('MODE', esvit_amd.is_deterministic())"
    env = {k: v for k, v in os.environ.items() if k != "ESVIT_DETERMINISTIC"}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    procs = [(val, subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, env=dict(env, **({} if val is None else {"ESVIT_DETERMINISTIC": val})),
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for val in (None, "0", "1", "yes")]
    for val, p in procs:
        out, err = p.communicate(timeout=120)
        if val == "yes":
            assert p.returncode != 0 and "ValueError" in err and "ESVIT_DETERMINISTIC" in err, err[-500:]
        else:
            assert p.returncode == 0 and "MODE %s" % (val == "1") in out, (val, out, err[-500:])


def test_switch_function(mode):
    import esvit_amd
    mode(True)
    assert esvit_amd.is_deterministic() is True
    mode(False)
    assert esvit_amd.is_deterministic() is False
    for bad in ("1", None, 2):
        with pytest.raises(ValueError):
            mode(bad)
    assert esvit_amd.is_deterministic() is False


# ---- routing, with a recording stand-in for the ops module ------------------------------------------------------------------------------
class _Rec:
    """oracle.ops_ref plus a relpos_bias_bwd that knows `ordered` (and says so), every call of it recorded"""
    RELPOS_BWD_ORDERED = True

    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        return getattr(ops_ref, name)

    def relpos_bias_bwd(self, *a, **k):
        self._calls.append((a, dict(k)))
        k.pop("ordered", None)
        return ops_ref.relpos_bias_bwd(*a, **k)


@pytest.fixture()
def rec_ops(monkeypatch, lib_built):
    import esvit_amd.functional as Fn
    import esvit_amd.loss as L
    import esvit_amd.params as P
    calls = []
    stub = _Rec(calls)
    for mod in (Fn, L, P):
        monkeypatch.setattr(mod, "ops", stub)
    ops_ref.set_act_dtype(torch.float32)
    P.clear()
    Fn._GEOM.clear()
    yield calls
    ops_ref.set_act_dtype(torch.float32)
    P.clear()
    Fn._GEOM.clear()


def _nano_backward():
    import esvit_amd.loss as L
    nano = torch.load(os.path.join(GOLD, "nano_step.pt"), weights_only=False)
    student, teacher = nano_pair()
    run_nano_step(nano, student, teacher, L, GU.make_crops(2))
    return student


def _cvt_rpe_backward(ragged):
    import esvit_amd.loss as L
    case = GU.NANO_CVT_VARIANTS["rpe"]
    student, teacher = build_cvt_variant(case), build_cvt_variant(case, teacher=True)
    GU.fill_state_dict(student.state_dict(), 0)
    GU.fill_state_dict(teacher.state_dict(), 7)
    for m in (student, teacher):
        for k, v in m.state_dict().items():
            if k.endswith("running_var"):
                v.abs_().add_(0.5)
    student.ragged_multi_crop = ragged
    crops = GU.make_crops(2, n_local=case["n_local"], sizes=case["sizes"])
    loss_fn = L.DDINOLoss(GU.NANO_HEAD["out_dim"], 2 + case["n_local"], 0.04, 0.07, 5, 10)
    with torch.no_grad():
        t_out = teacher(crops[:2])
    loss_fn(student(crops), t_out, 2, None).backward()


def test_mode_off_makes_the_calls_of_today(rec_ops, mode):
    """one Swin nano backward: positional (slabs, index, N, table rows) and at most the out / accumulate keywords, no `ordered`"""
    mode(False)
    _nano_backward()
    assert len(rec_ops) == sum(GU.NANO["depths"])  # one table gradient per block
    for a, k in rec_ops:
        assert len(a) == 4 and set(k) <= {"out", "accumulate"}, k
        assert k.get("out") is None and k.get("accumulate") is None


def test_mode_on_orders_every_table_gradient(rec_ops, mode):
    """the ragged Swin block (one call over both groups' slabs), W = 14, CvT with REL_POS_EMBED per group and on its ragged route (first
    group overwrites, second accumulates), and a call whose `out` is a reducer slot"""
    import esvit_amd.loss as L
    import esvit_amd.params as P
    mode(True)
    _nano_backward()
    assert len(rec_ops) == sum(GU.NANO["depths"])
    n0 = len(rec_ops)
    student, teacher = nano_pair(window=14)
    run_nano14_step(student, teacher, L)
    assert len(rec_ops) > n0 and any(a[2] == 196 for a, _ in rec_ops[n0:])
    n1 = len(rec_ops)
    _cvt_rpe_backward(ragged=False)
    n2 = len(rec_ops)
    _cvt_rpe_backward(ragged=True)
    assert n2 > n1 and len(rec_ops) > n2
    assert any(k.get("accumulate") is True and k.get("out") is not None for _, k in rec_ops[n2:])  # the second group of a ragged block
    assert any(not k.get("accumulate") for _, k in rec_ops[n2:])
    # a reducer slot as `out`
    n3 = len(rec_ops)
    student = nano_pair()[0]
    sinks = {id(p): torch.zeros_like(p) for p in student.parameters()}
    tables = [sinks[id(p)] for n, p in student.named_parameters() if "relative_position_bias_table" in n]
    P.set_grad_sink(sinks)
    try:
        out = student(GU.make_crops(2, n_local=2))
        (out[0].square().sum() + out[1].square().sum()).backward()
    finally:
        P.set_grad_sink(None)
    slot_calls = [k for _, k in rec_ops[n3:] if any(k.get("out") is t for t in tables)]
    assert len(slot_calls) == len(tables) and all(k["accumulate"] is False for k in slot_calls)
    for a, k in rec_ops:
        assert k.get("ordered") is True and len(a) == 4, k


def test_cpu_restatement_is_called_without_the_keyword_and_gives_the_same_bits(cpu_ops, mode):  # noqa: F811
    """oracle/ops_ref.relpos_bias_bwd has no `ordered`: the mode must not pass it, and the composition equals mode off exactly"""
    import inspect
    assert "ordered" not in inspect.signature(ops_ref.relpos_bias_bwd).parameters and not hasattr(ops_ref, "RELPOS_BWD_ORDERED")
    grads = []
    for on in (False, True):
        mode(on)
        student = _nano_backward()
        grads.append({n: p.grad.clone() for n, p in student.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 50
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n


class _UpdOps:
    RULE_ADAMW, RULE_SGD, RULE_LARS = 0, 1, 2

    def __init__(self):
        self.calls = []

    def update_chunk_elems(self):
        return 4096

    def grad_sqnorm(self, *a, **k):
        self.calls.append(("grad_sqnorm", a, k))

    def fused_clip_update_ema(self, *a, **k):
        self.calls.append(("fused_clip_update_ema", a, k))


class _NoEvent:
    def record(self):
        pass

    def synchronize(self):
        pass


@pytest.mark.parametrize("rule", ["adamw", "lars"])
def test_updater_sizes_its_buffer_and_passes_the_flag(monkeypatch, mode, rule):
    """mode off: grad_sqnorm(table, n, chunks, nchunks, sqnorms, stats=...) as today, sqnorms [n * stats]; mode on: ordered=True and
    sqnorms [(n + nchunks) * stats] (include/esvit_hip.h), also for an updater built before the mode was switched on"""
    import esvit_amd.update as U
    stub = _UpdOps()
    monkeypatch.setattr(U, "ops", stub)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda t: t)  # (no GPU here: the staging tables stay pageable)
    monkeypatch.setattr(torch.cuda, "Event", _NoEvent)
    stats = 3 if rule == "lars" else 1

    def build():
        torch.manual_seed(0)
        net = torch.nn.Sequential(torch.nn.Linear(70, 130), torch.nn.LayerNorm(130), torch.nn.Linear(130, 5))
        upd = U.FusedClipAdamWEMA(net, None, **({} if rule == "adamw" else {"rule": rule}))
        for p in net.parameters():
            p.grad = torch.ones_like(p)
        return net, upd
    mode(False)
    net, early = build()
    n, nchunks = len(list(net.parameters())), 3 + 1 + 1 + 1 + 1 + 1  # 9100 = 3 chunks, the rest one each
    assert early.nchunks == nchunks and early.sqnorms.numel() == n * stats
    early.step(1e-3, 0.04, 0.99)
    name, a, k = stub.calls[0]
    assert name == "grad_sqnorm" and len(a) == 5 and a[1] == n and a[3] == nchunks and a[4] is early.sqnorms and k == {"stats": stats}
    assert a[4].numel() == n * stats
    assert stub.calls[1][0] == "fused_clip_update_ema" and stub.calls[1][1][5] is early.sqnorms
    mode(True)
    _, late = build()
    assert late.sqnorms.numel() == (n + nchunks) * stats
    for upd in (late, early):
        del stub.calls[:]
        upd.step(1e-3, 0.04, 0.99)
        name, a, k = stub.calls[0]
        assert name == "grad_sqnorm" and len(a) == 5 and k == {"stats": stats, "ordered": True}
        assert a[4] is upd.sqnorms and a[4].numel() == (n + nchunks) * stats and a[4].dtype == torch.float32
        assert stub.calls[1][0] == "fused_clip_update_ema" and stub.calls[1][1][5] is upd.sqnorms  # the head has the layout the update reads


# ---- ViT: the matrix route of square crops ------------------------------------------------------------------------------------------------
def test_vit_square_crops_take_the_matrix_route(cpu_ops, mode):  # noqa: F811
    """NANO_VIT on the CPU in fp32, 64^2 (the construction grid) and 32^2 (resampled) crops: tokens of the two modes agree to 1e-6
    absolute; mode off calls F.interpolate exactly as before, mode on never does"""
    m = build_nano_vit()
    GU.fill_state_dict(m.state_dict(), 0)
    calls = []
    real = torch.nn.functional.interpolate

    def spy(*a, **k):
        calls.append(k.get("mode"))
        return real(*a, **k)
    g = torch.Generator().manual_seed(4)
    for side, resampled in ((64, False), (32, True)):
        x = torch.randn(2, 3, side, side, generator=g)
        toks = []
        for on in (False, True):
            mode(on)
            del calls[:]
            torch.nn.functional.interpolate = spy
            try:
                with torch.no_grad():
                    toks.append(m._tokens(x))
            finally:
                torch.nn.functional.interpolate = real
            assert calls == (["bicubic"] if resampled and not on else []), (side, on, calls)
        assert toks[0].shape == toks[1].shape == (2, 1 + (side // 16) ** 2, 64)
        assert (toks[0] - toks[1]).abs().max().item() <= 1e-6, side
        if not resampled:
            assert torch.equal(toks[0], toks[1])


def test_vit_pos_embed_gradient_matches_fp64_autograd_of_the_reference_formulation(cpu_ops, mode):  # noqa: F811
    mode(True)
    m = build_nano_vit()
    GU.fill_state_dict(m.state_dict(), 0)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 3, 32, 32, generator=g)
    w = torch.randn(3, 5, 64, generator=g)
    (m._tokens(x) * w).sum().backward()
    got = m.pos_embed.grad.double()
    # vision_transformer.py:263-277 in fp64
    pos = m.pos_embed.detach().double().requires_grad_(True)
    n_new, n_old = 4, pos.shape[1] - 1
    side = int(math.sqrt(n_old))
    grid = pos[:, 1:].reshape(1, side, side, 64).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, scale_factor=math.sqrt(n_new / n_old), mode="bicubic")
    ref = torch.cat((pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, -1, 64)), dim=1)
    assert ref.shape[1] == 5
    (ref * w.double().sum(0, keepdim=True)).sum().backward()
    want = pos.grad
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()
