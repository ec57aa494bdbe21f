"""esvit_gemm on the MI355X (esvit_amd/csrc/gemm.hip, gemm_kernels.h, gemm_p8.hip behind esvit_amd.ops._gemm) against the fp64 statement
of tests/gemm_ref.py on inputs for which the GEMM is exact: every main loop and tile, the three operand layouts, every epilogue option on
both its straight-line and its general path (aligned-dense and alignment-defeated placement), split-K with empty slices, batching, and
the eight-phase loop walking more than one item per workgroup.  Each case is a tiny launch with an explicit descriptor and an explicit
kernel=; it is followed by the exact comparison (bit for bit in fp32, torch's round-to-nearest-even in bf16 -- no tolerance before the
activation function), the moat check (NaN pads around every input, a sentinel bit pattern around and between everything written) and a
second launch whose bits must equal the first.  Only the four activation epilogues have a bound (module docstring of tests/gemm_ref.py);
their err / bound ratios go to golden_utils.record_parity, and the device run is committed as profiles/gemm_parity_observed.jsonl, a
record only.  tests/test_gemm_cpu.py proves the cases, the coverage claims and the mutants this comparison catches without a GPU."""
import pytest
import torch

from tests import gemm_ref as GR
from tests import golden_utils as GU

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


def _run(ops, cases):
    assert cases
    bad = []
    for case, dt in cases:
        bad += GR.run_and_verify(ops, DEV, case, dt, record=GU.record_parity)
    assert not bad, "%d failures, first: %s" % (len(bad), bad[:8])


def _groups(family):
    """one test per (loop, layout) the table has cases of"""
    keys = sorted({(c["kern"], c["lay"]) for c in GR.table() if c["family"] == family})
    return [pytest.param(k, lay, id="%s-%s" % (GR.KNAME[k], lay)) for k, lay in keys]


def test_the_views_defeat_the_alignment_checks(ops):
    """the device addresses really are what tests/test_gemm_cpu.py assumed when it evaluated the fast-path predicates"""
    case = next(c for c, dt in GR.select("epi", GR.DMA4, "nt") if c["name"].startswith("epi-res-rs-f32-off"))
    for dense in (False, True):
        prob = GR.build(dict(case, defeat=()) if dense else case, GR.BF16)
        d = {n: b.to(DEV) for n, b in prob["bufs"].items()}
        for n in d:
            assert d[n].data_ptr() % 16 == 0
        ptr = lambda f: d[prob["desc"][f][0]][prob["desc"][f][1]:].data_ptr()
        assert ptr("A") % 16 == 0 and ptr("B") % 16 == 0
        assert ptr("C") % 16 == (0 if dense else 8) and ptr("residual") % 16 == (0 if dense else 8) and ptr("bias") % 16 == (0 if dense else 4)
        assert prob["desc"]["ldc"] % 8 == (0 if dense else 4) and prob["desc"]["ldr"] % 4 == (0 if dense else 2)
    prob = GR.build(next(c for c, dt in GR.select("epi", GR.DMA4, "nt") if c["name"].startswith("epi-gelu-aux-off")), GR.BF16)
    d = prob["bufs"]["aux"].to(DEV)
    assert d[prob["desc"]["aux"][1]:].data_ptr() % 16 == 8 and prob["desc"]["ldaux"] % 8 == 4
    prob = GR.build(next(c for c, dt in GR.select("batch", GR.DMA4, "nt") if "stridec" in c["name"]), GR.BF16)
    assert prob["desc"]["strideC"] % 8 == 4 and prob["desc"]["ldc"] % 8 == 0


@pytest.mark.parametrize("kern,lay", _groups("shape"))
def test_gemm_shapes(ops, kern, lay):
    """sub-tile, interior + ragged, odd N, every tile width, one to seven k-tiles and a partial one (fp32 mode beside the default loop)"""
    _run(ops, GR.select("shape", kern, lay))


@pytest.mark.parametrize("kern,lay", _groups("wgrad"))
def test_gemm_wgrad(ops, kern, lay):
    """both operands k-strided: plain, with the fused bias gradient, and accumulating through residual = C"""
    _run(ops, GR.select("wgrad", kern, lay))


@pytest.mark.parametrize("kern,lay", _groups("epi"))
def test_gemm_epilogues(ops, kern, lay):
    """every epilogue option on the interior-plus-ragged shape of every tile, aligned-dense and alignment-defeated"""
    _run(ops, GR.select("epi", kern, lay))


@pytest.mark.parametrize("kern,lay", _groups("rowmap"))
def test_gemm_rowmap(ops, kern, lay):
    """window -> token scatter with dropped rows and untargeted token rows, with residual, rowscale and out_rows"""
    _run(ops, GR.select("rowmap", kern, lay))


@pytest.mark.parametrize("kern,lay", _groups("single"))
def test_gemm_one_fast_path_condition_at_a_time(ops, kern, lay):
    _run(ops, GR.select("single", kern, lay))


@pytest.mark.parametrize("kern,lay", _groups("splitk"))
def test_gemm_splitk(ops, kern, lay):
    """explicit splitk 2, 3, 7 and 4 (empty slices), fp32 and bf16 output, accumulate, colsum_partial, alpha, an unaligned workspace"""
    _run(ops, GR.select("splitk", kern, lay))


@pytest.mark.parametrize("lay", ("nt", "dg", "wg"))
def test_gemm_batch(ops, lay):
    """batch = 3 at the ViT attention shapes on AUTO and on every forced loop, dense and with item 1 of C off the 16-byte grid"""
    _run(ops, GR.select("batch", lay=lay))


@pytest.mark.parametrize("case", [pytest.param(c, id=c["name"]) for c, _ in GR.select("multi")])
def test_gemm_p8_multi_item_walk(ops, case):
    """more than 256 work items: every workgroup streams its DMA requests across an item boundary; 31 of 66 split-K slices are empty"""
    assert GR.p8_items(case) > 256
    _run(ops, [(case, GR.BF16)])


# ---- the Python wrappers on exact inputs: their own split-K choices and the sizing of `partial` -------------------------------------------
def _exact(key, shape, lim, probs, scale, dt):
    return (GR.ints((key,), shape, lim, probs) * scale).to(dt)


@pytest.mark.parametrize("dt", GR.DTYPES, ids=GR.dt_name)
def test_wrapper_linear_fwd(ops, dt):
    x, w = _exact("wf-x", (168, 72), 3, GR.A_SKEW, 0.25, dt), _exact("wf-w", (152, 72), 2, GR.B_SKEW, 0.5, dt)
    bias, res = _exact("wf-b", (152,), 40, None, 0.125, GR.F32), _exact("wf-r", (168, 152), 60, None, 0.125, GR.F32)
    want = (x.double() @ w.double().t() + bias.double()) + res.double()
    got = ops.linear_fwd(x.to(DEV), w.to(DEV), bias.to(DEV), residual=res.to(DEV), out_f32=True).cpu()
    assert torch.equal(got, want.float())
    got = ops.linear_fwd(x.to(DEV), w.to(DEV), bias.to(DEV)).cpu()
    assert torch.equal(got, (x.double() @ w.double().t() + bias.double()).float().to(dt))


@pytest.mark.parametrize("dt", GR.DTYPES, ids=GR.dt_name)
def test_wrapper_linear_dgrad_splits_a_4096_long_reduction(ops, dt):
    dy, w = _exact("wd-dy", (264, 4096), 3, GR.A_SKEW, 0.25, dt), _exact("wd-w", (4096, 256), 2, GR.B_SKEW, 0.5, dt)
    want = dy.double() @ w.double()
    assert float((dy.double().abs() @ w.double().abs()).max()) * 8 < 2 ** 24   # units of 2^-3: exact in fp32
    for of32 in (True, False):
        got = ops.linear_dgrad(dy.to(DEV), w.to(DEV), out_f32=of32).cpu()
        assert torch.equal(got, want.float() if of32 else want.float().to(dt))


@pytest.mark.parametrize("dt", GR.DTYPES, ids=GR.dt_name)
def test_wrapper_linear_wgrad_with_the_empty_slice_of_pick_splitk(ops, dt):
    """8256 rows x 96 x 96: _pick_splitk gives 16 slices of 9 k-tiles over 129 -- slice 15 is empty"""
    rows = 8256
    dy, x = _exact("ww-dy", (rows, 96), 3, GR.A_SKEW, 0.25, dt), _exact("ww-x", (rows, 96), 2, GR.B_SKEW, 0.5, dt)
    if dt == GR.BF16:
        _, tm, tn, slots = ops.gemm_select(dt, M=96, N=96, K=rows, lda=96, ldb=96, ldc=96, a_kstrided=1, b_kstrided=1)
        sk = ops._pick_splitk(rows, 96, 96, (-(-96 // tm)) * (-(-96 // tn)), slots)
        assert sk == 16 and GR.empty_slices(rows, sk, 64)
    want, wdb = dy.double().t() @ x.double(), dy.double().sum(0)
    out = _exact("ww-out", (96, 96), 50, None, 0.125, GR.F32)
    got, db = ops.linear_wgrad(dy.to(DEV), x.to(DEV), want_bias=True)
    assert torch.equal(got.cpu(), want.float()) and torch.equal(db.cpu(), wdb.float())
    acc = out.to(DEV)
    ops.linear_wgrad(dy.to(DEV), x.to(DEV), out=acc, accumulate=True)
    assert torch.equal(acc.cpu(), (want + out.double()).float())
    # few rows: no split, the accumulate route through residual = C
    acc = out.to(DEV)
    ops.linear_wgrad(dy[:200].to(DEV), x[:200].to(DEV), out=acc, accumulate=True)
    assert torch.equal(acc.cpu(), (dy[:200].double().t() @ x[:200].double() + out.double()).float())


def test_wrapper_batched_nt(ops):
    a, b = _exact("wb-a", (3, 49, 32), 3, GR.A_SKEW, 0.25, GR.F32), _exact("wb-b", (3, 49, 32), 2, GR.B_SKEW, 0.5, GR.F32)
    got = ops.batched_nt(a.to(DEV), b.to(DEV), 52).cpu()
    assert torch.equal(got[:, :, :49], torch.bmm(a.double(), b.double().transpose(1, 2)).float())
