"""The convolution and BatchNorm kernels on the MI355X (esvit_amd/csrc/conv.hip behind esvit_amd.ops) against the fp64 statement of
tests/conv_ref.py: one test per entry point over the case table -- every kernel instantiation, every grid-stride loop taken twice,
non-square grids, W from 1 to 8, channel-lane counts that do not divide 256 -- and both dtypes, under bounds derived from the number
formats (the module docstring of tests/conv_ref.py lists them and the case -> kernel table).  tests/test_conv_cpu.py proves the cases,
the bounds and the mutants they catch without a GPU.  Every err / bound ratio goes to golden_utils.record_parity; the device run is
committed as profiles/conv_parity_observed.jsonl, a record only."""
import pytest
import torch

from tests import conv_ref as CR
from tests import golden_utils as GU

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


def _params(table):
    return [pytest.param(c, dt, id="%s-%s" % (c["name"], CR.dt_name(dt))) for c in table for dt in CR.DTYPES if dt in c["dts"]]


def _check(entry, case, dt, metrics):
    CR.check(entry, case["name"] if isinstance(case, dict) else case, dt, metrics, record=GU.record_parity, where="mi355x")


def test_the_offset_views_defeat_every_16_byte_test(ops):
    t = CR.place(torch.zeros(6, 8, dtype=torch.bfloat16), DEV, CR.OFF)
    assert t.is_contiguous() and t.data_ptr() % 16 == 8
    assert CR.place(torch.zeros(6, 8), DEV, CR.OFF).data_ptr() % 16 == 0


@pytest.mark.parametrize("case,dt", _params(CR.IM2COL))
def test_conv_im2col(ops, case, dt):
    """bit-equal to the gather, zero tail included; fp32 NCHW -> bf16 columns: torch's round-to-nearest-even"""
    _check("conv_im2col", case, dt, CR.run_im2col(ops, DEV, case, dt))


@pytest.mark.parametrize("case,dt", _params(CR.COL2IM))
def test_conv_col2im(ops, case, dt):
    _check("conv_col2im", case, dt, CR.run_col2im(ops, DEV, case, dt))


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("case,dt", _params(CR.DWCONV))
def test_dwconv3x3(ops, case, dt, flip):
    _check("dwconv3x3" + ("_flip" if flip else ""), case, dt, CR.run_dwconv(ops, DEV, case, dt, flip))


@pytest.mark.parametrize("case,dt", _params(CR.WGRAD))
def test_dwconv3x3_wgrad(ops, case, dt):
    """(L + 1) u abs_sum per tap and channel, and the same bits on a second run"""
    _check("dwconv3x3_wgrad", case, dt, CR.run_wgrad(ops, DEV, case, dt))


@pytest.mark.parametrize("case,dt", _params(CR.COL_SUMS))
def test_col_sums2(ops, case, dt):
    """C from 4 to 4096 (above 1024: the channel-tiled kernel), (L + 1) u abs_sum per channel, the same bits on a second run"""
    _check("col_sums2", case, dt, CR.run_col_sums(ops, DEV, case, dt))


@pytest.mark.parametrize("act", CR.AFFINE_ACTS)
@pytest.mark.parametrize("case,dt", _params(CR.AFFINE_SHAPES))
def test_col_affine2(ops, case, dt, act):
    _check("col_affine2_act" + act, case, dt, CR.run_affine(ops, DEV, case, dt, act))


@pytest.mark.parametrize("case,dt", _params(CR.PAD_CROP))
def test_pad_crop_tokens(ops, case, dt):
    _check("pad_crop_tokens", case, dt, CR.run_pad_crop(ops, DEV, case, dt))


@pytest.mark.parametrize("case", CR.BN_COEF, ids=CR.ids(CR.BN_COEF))
def test_bn_coefficient_kernels(ops, case):
    """fed fp32 sums, against fp64 from the same sums: n = 2, a constant channel (var = 0, rstd = eps^-1/2), a channel whose variance
    clamps, the running statistics with n / (n - 1), eval coefficients, the backward pair with red and with red = None"""
    _check("bn_coeffs", case, None, CR.run_bn_coef(ops, DEV, case))


def test_bn_coefficients_at_mean_over_std_up_to_16(ops):
    _check("bn_coeffs", "offset", None, CR.run_bn_offset(ops, DEV))


@pytest.mark.parametrize("dt", CR.DTYPES, ids=CR.dt_name)
@pytest.mark.parametrize("r,rows", CR.BN_CHAIN)
def test_bn_end_to_end_conditioning(ops, r, rows, dt):
    """col_sums2 -> bn_fwd_coeffs -> col_affine2 against the fp64 batch norm of the input: the contract of the E[x^2] - mean^2 form is
    a relative rstd error of at most 8 (1 + r^2) u at mean / std = r; torch's own fp32 batch_norm is recorded next to it"""
    _check("bn_chain", "r%d_rows%d" % (r, rows), dt, CR.run_bn_chain(ops, DEV, r, rows, dt))


# ---- DINOHead(use_bn=True) at the reference's default hidden width ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_bn_head_at_hidden_2048(ops, prec):
    """forward and backward of DINOHead(48, 96, use_bn=True, bottleneck_dim=32) at hidden_dim = 2048 (its BatchNorm statistics are
    col_sums2 at C = 2048) against the fp64 autograd of the torch modules it is made of.  Bounds, relative in the 2-norm: the ones
    tests/test_variants.py holds the same module to at hidden 64 -- 2e-5 in fp32, 2e-2 in bf16, four times that for the gradients;
    a dot product 32 times as long averages its roundings, it does not add them up.  Before col_sums2 took C > 1024 this failed with
    "esvit_col_sums2: bad C=2048"."""
    import esvit_amd
    sd, x, probe = CR.head_case()
    ref = CR.head_ref(sd, x, probe)
    tol = 2e-5 if prec == "fp32" else 2e-2
    esvit_amd.set_precision(prec)
    try:
        head = esvit_amd.DINOHead(CR.HEAD["in_dim"], CR.HEAD["out_dim"], use_bn=True, hidden_dim=CR.HEAD["hidden_dim"], bottleneck_dim=CR.HEAD["bottleneck_dim"])
        head.load_state_dict(sd)
        head.sync_bn_group = False
        head = head.to(DEV).train()
        xg = x.to(DEV).requires_grad_(True)
        out = head(xg)
        (out * probe.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        esvit_amd.set_precision("bf16")
    rel = lambda a, b: ((a.detach().double().cpu() - b).norm() / b.norm()).item()  # noqa: E731
    m = dict(ratio_logits=rel(out, ref["logits"]) / tol, ratio_dx=rel(xg.grad, ref["dx"]) / (4 * tol))
    params = dict(head.named_parameters())
    for n, p in params.items():
        if n in ("mlp.0.bias", "mlp.3.bias"):
            # a bias in front of a BatchNorm has an exactly-zero gradient; what arrives is the rounding of a column sum of the weight's terms
            m["ratio_" + n] = p.grad.norm().item() / (20 * tol * params[n.replace("bias", "weight")].grad.norm().item())
        elif n in ref["grads"]:
            m["ratio_" + n] = rel(p.grad, ref["grads"][n]) / (4 * tol)
        else:
            assert p.grad is None, n
    for n, b in head.named_buffers():
        if b.is_floating_point():
            m["ratio_" + n] = rel(b, ref["buffers"][n]) / tol
        else:
            m["equal_" + n] = float(int(b) == int(ref["buffers"][n]))
    _check("bn_head_2048", prec, None, m)


# ---- contracts that are refused, not assumed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,off_bytes", [(torch.bfloat16, 4), (torch.float32, 4), (torch.float32, 8)], ids=["bf16-4", "fp32-4", "fp32-8"])
def test_pointers_below_the_four_channel_alignment_are_refused(ops, dt, off_bytes):
    """the per-channel kernels and col_sums2 move four channels per load: 8 bytes of bf16, 16 of fp32.  C = 12 keeps bf16 out of the
    strip kernel, so the alignment in question is the fallback's own"""
    off = off_bytes // (2 if dt == torch.bfloat16 else 4)
    nB, H, W, C = 2, 3, 5, 12
    good = CR.data(("refuse",), (nB * H * W, C), dt).to(DEV)
    bad = CR.place(good.cpu(), DEV, off)
    assert bad.data_ptr() % 16 == off_bytes
    w = torch.ones(C, 9, device=DEV)
    launched = []
    with pytest.raises(RuntimeError, match="aligned to four channels"):
        launched.append(ops.dwconv3x3(bad, w, nB, H, W))
    with pytest.raises(RuntimeError, match="aligned to four channels"):
        launched.append(ops.dwconv3x3_wgrad(bad, good, nB, H, W))
    with pytest.raises(RuntimeError, match="aligned to four channels"):
        launched.append(ops.dwconv3x3_wgrad(good, bad, nB, H, W))
    with pytest.raises(RuntimeError, match="aligned to four channels"):
        launched.append(ops.col_sums2(bad, good))
    with pytest.raises(RuntimeError, match="aligned to four channels"):
        launched.append(ops.col_sums2(good, bad))
    assert not launched
    torch.cuda.synchronize()  # nothing was launched: the stream is clean


@pytest.mark.parametrize("dt", CR.DTYPES, ids=CR.dt_name)
def test_pad_crop_refuses_a_source_off_its_16_bytes(ops, dt):
    C = 8
    src = CR.place(CR.data(("refuse_pc",), (2 * 3 * 4, C), dt), DEV, 8 // (2 if dt == torch.bfloat16 else 4))
    assert src.data_ptr() % 16 == 8
    launched = []
    with pytest.raises(RuntimeError, match="aligned to 16 bytes"):
        launched.append(ops.pad_crop_tokens(src, 2, 3, 4, 4, 5))
    assert not launched
    torch.cuda.synchronize()


def test_widths_only_the_strip_kernels_reach_are_refused_elsewhere(ops):
    """C = 2048 is C / 8 = 256 strip lanes in bf16; the per-channel kernels stop at C / 4 = 256"""
    x = torch.zeros(2 * 3, 2048, device=DEV)
    launched = []
    with pytest.raises(RuntimeError, match="too wide"):
        launched.append(ops.dwconv3x3(x, torch.ones(2048, 9, device=DEV), 1, 2, 3))
    with pytest.raises(RuntimeError, match="bad C=2048"):
        launched.append(ops.dwconv3x3_wgrad(x, x, 1, 2, 3))
    with pytest.raises(RuntimeError, match="bad C=6"):
        launched.append(ops.col_sums2(torch.zeros(4, 6, device=DEV), torch.zeros(4, 6, device=DEV)))
    assert not launched
    torch.cuda.synchronize()


def test_col_affine2_asserts_on_its_second_operand(ops):
    x1 = torch.zeros(6, 8, dtype=torch.bfloat16, device=DEV)
    a = torch.ones(8, device=DEV)
    for x2 in (torch.zeros(6, 8, device=DEV), torch.zeros(5, 8, dtype=torch.bfloat16, device=DEV), torch.zeros(6, 16, dtype=torch.bfloat16, device=DEV)[:, ::2]):
        with pytest.raises(AssertionError):
            ops.col_affine2(x1, a, a, x2, a)
    x2 = torch.zeros_like(x1)
    for a2 in (torch.ones(8, dtype=torch.float64, device=DEV), torch.ones(4, device=DEV), torch.ones(16, device=DEV)[::2]):
        with pytest.raises(AssertionError):
            ops.col_affine2(x1, a, a, x2, a2)
    assert bool((ops.col_affine2(x1, a, a, x2, a) == 1).all())
