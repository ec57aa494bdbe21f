"""The normalisation kernels on the MI355X (esvit_amd/csrc/norm.hip behind ops.layernorm_fwd / layernorm_bwd / layernorm_bwd_cast /
layernorm_bwd_to_act / merge_ln_fwd / merge_ln_bwd / l2norm_fwd / l2norm_bwd / weightnorm_fwd / weightnorm_bwd) against the fp64
statement of tests/norm_ref.py: all twelve LayerNorm instantiations and all four row-iteration counts in both dtypes, partly filled lane
groups, one row and a ragged last block, the grid-stride loop of the backward taken twice by some lane groups and once by others, the
dgamma / dbeta folds above 48 KiB of LDS, row maps with pads, g_in / dx_act / rowscale / gb_out variants, rows with a mean far from 0,
constant rows, mixed scales, both eps, the merge gather on rectangular grids with act_out and accumulate, zero and tiny rows of the L2
normalise -- every element of every output under its bound (the module docstring of tests/norm_ref.py derives them and lists the case ->
instantiation table), every launch twice with the same bits.  tests/test_norm_cpu.py proves the statement, the bounds and the mutants
the cases catch without a GPU.  Every err / bound ratio goes to golden_utils.record_parity; the device run is committed as
profiles/norm_parity_observed.jsonl, a record only."""
import pytest
import torch

from tests import golden_utils as GU
from tests import norm_ref as NR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


def _params(kinds, prefix=""):
    ps = [p for p in NR.params(kinds) if p[0]["name"].startswith(prefix)]
    return [pytest.param(c, dt, id="%s-%s" % (c["name"], NR.dt_name(dt))) for c, dt in ps]


def _run_case(ops, case, dt):
    if case["kind"] in ("ln", "merge"):
        assert ops.query(ops.Q_LN_BWD_BLOCKS, case["rows"], case["C"]) == NR.ln_bwd_blocks(case["rows"], case["C"])
    got = NR.run(ops, DEV, case, dt, repeat=True)
    NR.check("device", case, dt, NR.metrics(case, dt, got), record=GU.record_parity, where="mi355x")


@pytest.mark.parametrize("case,dt", _params(("ln",), "ln_w"))
def test_layernorm_widths(ops, case, dt):
    """every width of the table with one row and with 2 RPB + 1 rows: forward and backward"""
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params(("ln",), "ln_pass"))
def test_layernorm_backward_walks_the_grid_twice(ops, case, dt):
    """1024 blocks for more than 1024 RPB rows: some lane groups take two trips through the loop, the others one; dgamma / dbeta over
    all of the rows"""
    assert ops.query(ops.Q_LN_BWD_BLOCKS, case["rows"], case["C"]) == 1024
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params(("ln",), "ln_var"))
def test_layernorm_variants(ops, case, dt):
    """want_f32, g_in, the dx_act copy with and without rowscale (samples of one and of several rows, a factor 0), the fp32 -> activation
    backward without dx, gb_out adjacent (one fold) and separate (two folds)"""
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params(("ln",), "ln_map"))
def test_layernorm_row_maps(ops, case, dt):
    """token -> window slot maps on the store of the forward and the load of the backward; pad rows exactly 0"""
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params(("ln",), "ln_num"))
def test_layernorm_numerics(ops, case, dt):
    """|mean| >> std, constant rows, rows of scale 1e-4 and 1e4, eps 1e-6 and 1e-5"""
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params(("merge",)))
def test_merge_layernorm(ops, case, dt):
    """the 2 x 2 gather on square and rectangular grids up to 4 C = 2048: forward (also into row slices), backward, act_out with and
    without per-token rowscale, accumulate=True onto a first call's result"""
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params(("l2",)))
def test_l2_normalise(ops, case, dt):
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params(("wn",)))
def test_weight_norm(ops, case, dt):
    _run_case(ops, case, dt)


# ---- refusals: argument checks on the host, nothing is launched and nothing is written ----------------------------------------------------
class _Poison:
    """every tensor the wrapper allocates during the call is filled with the sentinel and kept"""

    def __init__(self, monkeypatch):
        self.made = []
        empty, empty_like, zeros = torch.empty, torch.empty_like, torch.zeros

        def fill(t):
            if t.is_floating_point():
                t.fill_(NR.SENTINEL)
                self.made.append(t)
            return t
        monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(empty(*a, **k)))
        monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(empty_like(*a, **k)))
        monkeypatch.setattr(torch, "zeros", lambda *a, **k: fill(zeros(*a, **k)))

    def intact(self):
        torch.cuda.synchronize()
        return all(bool((t == NR.SENTINEL).all()) for t in self.made)


def _refused(fn, *tensors):
    with pytest.raises(RuntimeError, match="failed"):
        fn()
    torch.cuda.synchronize()
    for t in tensors:
        assert bool((t == NR.SENTINEL).all())


def _sent(*shape, dt=torch.float32):
    return torch.full(shape, NR.SENTINEL, dtype=dt, device=DEV)


@pytest.mark.parametrize("dt", NR.DTYPES, ids=NR.dt_name)
@pytest.mark.parametrize("C", NR.REFUSED_LN)
def test_layernorm_refuses_widths_without_an_instantiation(ops, monkeypatch, C, dt):
    rows = 5
    x, gamma, beta = (NR.data(("ref", C, k), s).to(DEV) for k, s in (("x", (rows, C)), ("g", (C,)), ("b", (C,))))
    dy, st = NR.data(("ref", C, "dy"), (rows, C), dt).to(DEV), NR.data(("ref", C, "st"), (rows,)).to(DEV)
    gb = _sent(2, C)
    assert ops.query(ops.Q_LN_BWD_BLOCKS, rows, C) == 0
    ops.workspace(1, DEV, slot=1)  # (the shared scratch exists before the allocations are watched)
    made = _Poison(monkeypatch)
    _refused(lambda: ops.layernorm_fwd(x, gamma, beta, 1e-6, dtype=dt, want_f32=True))
    _refused(lambda: ops.layernorm_bwd(dy, x, st, st, gamma, gb_out=(gb[0], gb[1])), gb)
    _refused(lambda: ops.layernorm_bwd_cast(dy, x, st, st, gamma, gb_out=(gb[0], gb[1])), gb)
    assert made.made and made.intact()


@pytest.mark.parametrize("dt", NR.DTYPES, ids=NR.dt_name)
def test_merge_layernorm_refuses_an_odd_height(ops, monkeypatch, dt):
    nB, H, W, Cin = 1, 3, 4, 96
    rows = nB * (H // 2) * (W // 2)
    x = NR.data(("ref", "mx"), (nB, H * W, Cin)).to(DEV)
    gamma, beta = NR.data(("ref", "mg"), (4 * Cin,)).to(DEV), NR.data(("ref", "mb"), (4 * Cin,)).to(DEV)
    y, mean, rstd = _sent(rows, 4 * Cin, dt=dt), _sent(rows), _sent(rows)
    _refused(lambda: ops.merge_ln_fwd(x, gamma, beta, 1e-6, H, W, dtype=dt, out=(y, mean, rstd)), y, mean, rstd)
    dy, st = NR.data(("ref", "mdy"), (rows, 4 * Cin), dt).to(DEV), NR.data(("ref", "mst"), (rows,)).to(DEV)
    dx, gb, act = _sent(nB * H * W, Cin), _sent(2, 4 * Cin), _sent(nB * H * W, Cin, dt=dt)
    ops.workspace(1, DEV, slot=1)
    made = _Poison(monkeypatch)
    _refused(lambda: ops.merge_ln_bwd(dy, x, st, st, gamma, H, W, dx_out=dx, gb_out=gb, act_out=act), dx, gb, act)
    assert made.intact()


@pytest.mark.parametrize("dt", NR.DTYPES, ids=NR.dt_name)
@pytest.mark.parametrize("D", NR.REFUSED_ROW)
def test_l2_and_weight_norm_refuse_unsupported_widths(ops, monkeypatch, D, dt):
    R = 5
    x, dz = NR.data(("ref", D, "x"), (R, D), dt).to(DEV), NR.data(("ref", D, "dz"), (R, D), dt).to(DEV)
    v, gw, inv = NR.data(("ref", D, "v"), (R, D)).to(DEV), NR.data(("ref", D, "g"), (R, 1)).to(DEV), NR.data(("ref", D, "i"), (R,)).to(DEV)
    dv = _sent(R, D)
    made = _Poison(monkeypatch)
    _refused(lambda: ops.l2norm_fwd(x))
    _refused(lambda: ops.l2norm_bwd(dz, x, inv))
    _refused(lambda: ops.weightnorm_fwd(v, gw, dtype=dt))
    _refused(lambda: ops.weightnorm_bwd(v, v, gw, inv, True, dv_out=dv), dv)
    assert made.made and made.intact()
