"""-m gpu: esvit_mlp_fused_bwd with the weight gradients accumulated on the chip (bf16, C = 96) against the torch restatement of the
data-gradient path, fp64 autograd of the unfused branch, and the present route (NULL trailing arguments + two GEMMs) as the yardstick
of the summation-order error.  Row counts: below one tile, ragged tiles, fewer tiles than workgroups, and two tiles per workgroup plus
a ragged tail (the grid is asked of the library)."""
import ctypes
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 96
DT = torch.bfloat16
NAMES = ("dgamma", "dbeta", "dW1", "db1", "dW2", "db2", "dx")
_OBSERVED = []


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _rand(shape, dev, seed, dt=torch.float32, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dt)


def _close(name, got, ref, tol):
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    assert math.isfinite(err), "%s: non-finite output" % name
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e (rel %.3e > tol %.1e)" % (name, err, scale, err / scale, tol)


@pytest.fixture(scope="module")
def mods(lib_built):
    from esvit_amd import ops
    from oracle import ops_ref
    return ops, ops_ref


@pytest.fixture(scope="module", autouse=True)
def _write_observed():
    yield
    if _OBSERVED:
        try:
            with open(os.path.join(ROOT, "profiles", "mlp_dw_parity_observed.jsonl"), "w") as f:
                for rec in _OBSERVED:
                    f.write(json.dumps(rec) + "\n")
        except OSError:
            pass  # (a read-only checkout: the figures are in the assertion messages)


def _row_counts(ops):
    G = ops.mlp_fused_dw_grid(DT, C, 1 << 40)  # the grid of a launch with more tiles than workgroups
    assert G > 0
    return [1, 49, 127, 128, 129, 128 * 3 + 37, 128 * (2 * G) + 77], G


CASES = [(i, dp) for i in range(7) for dp in (False, True)]
_CACHE = {}


def _case(mods, i, dp):
    """inputs, the new route (three launches), the present route and the fp64 reference of one (M, DropPath) case, computed once"""
    key = (i, dp)
    if key in _CACHE:
        return _CACHE[key]
    ops, ref = mods
    dev = _dev()
    Ms, G = _row_counts(ops)
    M = Ms[i]
    x = _rand((M, C), dev, 70) * 1.5 + 0.3
    gy = _rand((M, C), dev, 71) * 0.5
    g, b = 1.0 + 0.2 * _rand((C,), dev, 72), 0.1 * _rand((C,), dev, 73)
    W1f, b1 = _rand((4 * C, C), dev, 74, torch.float32, 0.08), 0.1 * _rand((4 * C,), dev, 75)
    W2f = _rand((C, 4 * C), dev, 76, torch.float32, 0.05)
    W1, W2 = W1f.to(DT), W2f.to(DT)
    W1T, W2T = W1.t().contiguous(), W2.t().contiguous()
    K1, K2T, K1T = (ops.mlp_fused_weight(k, w) for k, w in ((ops.MLP_W1_BWD, W1f), (ops.MLP_W2T_BWD, W2f), (ops.MLP_W1T_BWD, W1f)))
    rs_mlp = rs_out = None
    if dp:  # DropPath row factors, rows with factor 0 among them
        gen = torch.Generator().manual_seed(77)
        rs_mlp = (torch.rand(M, generator=gen) > 0.3).float().div(0.7).to(dev)
        rs_out = (torch.rand(M, generator=gen) > 0.2).float().div(0.8).to(dev)
        if M > 1:
            assert bool((rs_mlp == 0).any()) or M < 8
    kw = dict(rowscale_mlp=rs_mlp, rowscale_out=rs_out)

    def finish(gx, G_, db1, dW2, db2):
        dW1, dg, dbeta = ops.ln_fold_finish(G_.clone(), db1, W1.float(), g, b)
        return dict(dgamma=dg, dbeta=dbeta, dW1=dW1, db1=db1, dW2=dW2, db2=db2, dx=gx)

    runs = []
    for _ in range(3):
        gx, gxa, dW2, db2, G_, db1 = ops.mlp_fused_bwd_dw(x, gy, g, b, 1e-6, K1, K2T, K1T, b1, **kw)
        runs.append(tuple(t.clone() for t in (gx, gxa, dW2, db2, G_, db1)))
    gx, gxa, dW2, db2, G_, db1 = runs[0]
    new = finish(gx, G_, db1, dW2, db2)
    # the present route of the same build
    ogx, ogxa, xhat, a1g, da1 = ops.mlp_fused_bwd(x, gy, g, b, 1e-6, K1, K2T, K1T, b1, **kw)
    dyb = (gy if rs_mlp is None else gy * rs_mlp[:, None]).to(DT)
    odW2, odb2 = ops.linear_wgrad(dyb, a1g, want_bias=True)
    oG, odb1 = ops.linear_wgrad(da1, xhat, want_bias=True)
    old = finish(ogx, oG, odb1, odW2, odb2)
    want = ref.mlp_fused_bwd(x, gy, g, b, 1e-6, W1, W2T, W1T, b1, **kw)
    # fp64 autograd of the unfused formula on the same bf16-rounded weights
    xa = x.double().requires_grad_(True)
    prm = [t.double().clone().requires_grad_(True) for t in (g, b, W1, b1, W2)]
    h = torch.nn.functional.layer_norm(xa, (C,), prm[0], prm[1], 1e-6)
    br = torch.nn.functional.gelu(h @ prm[2].t() + prm[3]) @ prm[4].t()
    y = xa + (br if rs_mlp is None else br * rs_mlp.double()[:, None])
    y.backward(gy.double())
    db2_ref = (gy.double() if rs_mlp is None else gy.double() * rs_mlp.double()[:, None]).sum(0)
    exact = dict(dgamma=prm[0].grad, dbeta=prm[1].grad, dW1=prm[2].grad, db1=prm[3].grad, dW2=prm[4].grad, db2=db2_ref, dx=xa.grad)
    out = dict(M=M, G=G, runs=runs, new=new, old=old, want=want, exact=exact, gx=gx, gxa=gxa, rs_out=rs_out)
    _CACHE[key] = out
    return out


@pytest.mark.parametrize("i,dp", CASES)
def test_data_gradients_match_the_restatement(mods, i, dp):
    c = _case(mods, i, dp)
    _close("gx", c["gx"], c["want"][0], 6e-3)
    _close("gx_act", c["gxa"], c["want"][1], 1e-2)


@pytest.mark.parametrize("i,dp", CASES)
def test_branch_gradients_against_fp64_and_the_present_route(mods, i, dp):
    c = _case(mods, i, dp)
    pairs = {}
    for name in NAMES:
        ex = c["exact"][name]
        scale = ex.abs().max().item() + 1e-12
        e_new = (c["new"][name].double() - ex).abs().max().item() / scale
        e_old = (c["old"][name].double() - ex).abs().max().item() / scale
        pairs[name] = (e_new, e_old)
    _OBSERVED.append(dict(M=c["M"], grid=c["G"], droppath=dp, rel_err_new_vs_present={k: [float("%.4e" % a), float("%.4e" % b)] for k, (a, b) in pairs.items()}))
    print("M=%d dp=%s" % (c["M"], dp), {k: "%.3e / %.3e" % v for k, v in pairs.items()})
    for name, (e_new, e_old) in pairs.items():
        tol = 1.5e-2 if name == "dx" else 2e-2
        assert math.isfinite(e_new) and e_new <= tol, "%s: rel err %.3e > %.1e vs fp64" % (name, e_new, tol)
    for name, (e_new, e_old) in pairs.items():
        # both routes sum the same bf16-rounded products in fp32 and differ in order only
        assert e_new <= 1.5 * e_old, "%s: rel err %.3e on chip vs %.3e on the present route (M=%d)" % (name, e_new, e_old, c["M"])


@pytest.mark.parametrize("i,dp", CASES)
def test_three_launches_are_identical(mods, i, dp):
    c = _case(mods, i, dp)
    for k in (1, 2):
        for j, (a, r) in enumerate(zip(c["runs"][k], c["runs"][0])):
            assert torch.equal(a, r), "output %d differs between launch 0 and launch %d" % (j, k)


def _raw_bwd(ops, x, gy, g, b, K1, K2T, K1T, b1, outs, trailing):
    from esvit_amd._lib import lib
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    M, Cc = x.shape
    return lib.esvit_mlp_fused_bwd(1, p(x), p(gy), None, None, p(g), p(b), 1e-6, p(K1), p(K2T), p(K1T), p(b1), M, Cc, *[p(t) for t in outs],
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), *[p(t) for t in trailing])


def _legacy_inputs(ops, Cc, M):
    dev = _dev()
    x, gy = _rand((M, Cc), dev, 70) * 1.5 + 0.3, _rand((M, Cc), dev, 71) * 0.5
    g, b = 1.0 + 0.2 * _rand((Cc,), dev, 72), 0.1 * _rand((Cc,), dev, 73)
    W1f, b1, W2f = _rand((4 * Cc, Cc), dev, 74, torch.float32, 0.08), 0.1 * _rand((4 * Cc,), dev, 75), _rand((Cc, 4 * Cc), dev, 76, torch.float32, 0.05)
    K1, K2T, K1T = (ops.mlp_fused_weight(k, w) for k, w in ((ops.MLP_W1_BWD, W1f), (ops.MLP_W2T_BWD, W2f), (ops.MLP_W1T_BWD, W1f)))
    outs = [torch.zeros((M, Cc), device=dev), torch.zeros((M, Cc), device=dev, dtype=DT), torch.zeros((M, Cc), device=dev, dtype=DT),
            torch.zeros((M, 4 * Cc), device=dev, dtype=DT), torch.zeros((M, 4 * Cc), device=dev, dtype=DT)]
    return x, gy, g, b, K1, K2T, K1T, b1, outs


@pytest.mark.parametrize("Cc,M", [(96, 128 * 3 + 37), (192, 77)])
def test_null_trailing_arguments_are_the_present_mode(mods, Cc, M):
    ops, _ = mods
    x, gy, g, b, K1, K2T, K1T, b1, outs = _legacy_inputs(ops, Cc, M)
    assert _raw_bwd(ops, x, gy, g, b, K1, K2T, K1T, b1, outs, [None] * 5) == 0
    for a, r in zip(outs, ops.mlp_fused_bwd(x, gy, g, b, 1e-6, K1, K2T, K1T, b1)):
        assert torch.equal(a, r)


def test_argument_checks_launch_nothing(mods):
    ops, _ = mods
    dev = _dev()
    for Cc in (96, 192):
        M = 77
        x, gy, g, b, K1, K2T, K1T, b1, outs = _legacy_inputs(ops, Cc, M)
        dW2, G_ = torch.full((Cc, 4 * Cc), 7.0, device=dev), torch.full((4 * Cc, Cc), 7.0, device=dev)
        db1, db2 = torch.full((4 * Cc,), 7.0, device=dev), torch.full((Cc,), 7.0, device=dev)
        ws = torch.full((max(ops.query(ops.Q_MLP_DW_WS, 1, 96, M) // 4, 1),), 7.0, device=dev)
        full = [dW2, G_, db1, db2, ws]
        tries = [full] if Cc == 192 else [full[:k] + [None] + full[k + 1:] for k in range(5)] + [[dW2] + [None] * 4]
        for trailing in tries:
            assert _raw_bwd(ops, x, gy, g, b, K1, K2T, K1T, b1, outs, trailing) == -1  # ESVIT_ERR_ARG
        torch.cuda.synchronize()
        for t in outs:
            assert not bool(t.float().abs().sum())  # nothing ran
        for t in full:
            assert bool((t == 7.0).all())
    assert ops.query(ops.Q_MLP_DW_WS, 1, 192, 77) == 0 and ops.query(ops.Q_MLP_DW_WS, 0, 96, 77) == 0
