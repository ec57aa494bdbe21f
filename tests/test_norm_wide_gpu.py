"""The wide LayerNorm rows on the MI355X (ln_wide_fwd_kernel / ln_wide_bwd_kernel of esvit_amd/csrc/norm.hip: 2048 < C <= 8192,
C % 1024 == 0) through the C ABI -- esvit_layernorm_fwd / esvit_layernorm_bwd / esvit_merge_ln_fwd / esvit_merge_ln_bwd -- against the
fp64 statement of tests/norm_wide_ref.py, per element, fp32 and bf16: C = 3072, 5120 and 8192 with 1, 5 and 1024 + 5 rows (the backward
loop taken twice by five workgroups, once by the others); at 3072 a row map with pad slots, want_f32, g_in, the dx_act copy with and
without rowscale (a factor 0 among them), the fp32 -> activation backward without dx, separate dgamma / dbeta destinations, rows with
|mean| = 100 std, constant rows, both eps; the merge gather on 2 x 2, on 4 x 6 with two samples and in pad mode on 3 x 5, into row slices,
with act_out, per-token rowscale and accumulate.  Every output sits in a moat of sentinels (the workspace too, sized by
ESVIT_Q_LN_BWD_BLOCKS), every input between NaN rows, every launch is made twice with equal bits, and the widths the library refuses
write nothing.  The bounds are the derived ones (module docstring of tests/norm_wide_ref.py); tests/test_swin_large_cpu.py proves the
statement and the mutants the cases catch without a GPU.  Every err / bound ratio goes to golden_utils.record_parity; the device run is
committed as profiles/norm_wide_parity_observed.jsonl, a record only."""
import pytest
import torch

from tests import golden_utils as GU
from tests import norm_ref as NR
from tests import norm_wide_ref as NW

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def device(lib_built):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return NW.Device()


def _params(prefix):
    return [pytest.param(c, dt, id="%s-%s" % (c["name"], NR.dt_name(dt))) for c, dt in NW.params(prefix)]


def _run_case(device, case, dt):
    assert device.o.query(device.o.Q_LN_BWD_BLOCKS, case["rows"], case["C"]) == NW.blocks(case["rows"], case["C"]) > 0
    got = NW.run(device, DEV, case, dt, repeat=True)
    NR.check("device_wide", case, dt, NW.metrics(case, dt, got), record=GU.record_parity, where="mi355x")


@pytest.mark.parametrize("case,dt", _params("wln_w"))
def test_wide_layernorm_widths_and_rows(device, case, dt):
    """3, 5 and 8 vectors per lane; one row, five, and 1024 + 5: forward and backward"""
    _run_case(device, case, dt)


@pytest.mark.parametrize("case,dt", _params("wln_var"))
def test_wide_layernorm_options(device, case, dt):
    _run_case(device, case, dt)


@pytest.mark.parametrize("case,dt", _params("wln_map"))
def test_wide_layernorm_row_map(device, case, dt):
    """token -> window slot on the store of the forward and the load of the backward; pad slots exactly 0"""
    _run_case(device, case, dt)


@pytest.mark.parametrize("case,dt", _params("wln_num"))
def test_wide_layernorm_numerics(device, case, dt):
    """|mean| = 100 std, constant rows, eps 1e-6 and 1e-5"""
    _run_case(device, case, dt)


@pytest.mark.parametrize("case,dt", _params("wmerge"))
def test_wide_merge_layernorm(device, case, dt):
    """4 x 768 = 3072: the PatchMerging norm in front of Swin-L's last stage"""
    _run_case(device, case, dt)


@pytest.mark.parametrize("dt", NW.DTYPES, ids=NR.dt_name)
@pytest.mark.parametrize("C", NW.REFUSED)
def test_refused_widths_write_nothing(device, C, dt):
    """98, 2052, 2560, 9216: the block-count answer is 0, every entry returns an error and no output, statistic or workspace element
    changes"""
    o, rows = device.o, 5
    assert o.query(o.Q_LN_BWD_BLOCKS, rows, C) == 0
    x, gamma, beta = (NR.data(("wref", C, k), s).to(DEV) for k, s in (("x", (rows, C)), ("g", (C,)), ("b", (C,))))
    dy, st = NR.data(("wref", C, "dy"), (rows, C), dt).to(DEV), NR.data(("wref", C, "st"), (rows,)).abs().to(DEV)
    y, yf, mean, rstd = NW.Out((rows, C), dt, DEV), NW.Out((rows, C), torch.float32, DEV), NW.Out((rows,), torch.float32, DEV), NW.Out((rows,), torch.float32, DEV)
    dx, dxa, gb = NW.Out((rows, C), torch.float32, DEV), NW.Out((rows, C), dt, DEV), NW.Out((2, C), torch.float32, DEV)
    assert device.fwd(dt, x, gamma, beta, 1e-6, rows, C, y.t, yf.t, mean.t, rstd.t, None, 0, 0) != 0
    assert device.bwd(dt, dy, x, st, st, gamma, None, rows, C, dx.t, gb.t[0], gb.t[1], None, 0, 0, dxa.t, dt, None, 0) != 0
    outs = [y, yf, mean, rstd, dx, dxa, gb]
    if C % 16 == 0:  # a merge of four C / 4-channel tokens
        nB, H, W, Cin = 1, 2, 2, C // 4
        xm = NR.data(("wref", C, "xm"), (nB * H * W, Cin)).to(DEV)
        ym, dxm = NW.Out((1, C), dt, DEV), NW.Out((nB * H * W, Cin), torch.float32, DEV)
        assert device.merge_fwd(dt, xm, gamma, beta, 1e-6, nB, H, W, Cin, False, ym.t, mean.t[:1], rstd.t[:1]) != 0
        assert device.merge_bwd(dt, dy[:1], xm, st[:1], st[:1], gamma, nB, H, W, Cin, False, dxm.t, gb.t[0], gb.t[1], None, None, 1, 0) != 0
        outs += [ym, dxm]
    torch.cuda.synchronize()
    ws, device.ws = device.ws, []
    assert all(bool((w.buf == NW.SENTINEL).all()) for w in outs + ws)
