"""Sliding-chunk attention on the MI355X against the fp64 statement of tests/chunk_attn_ref.py, both routes: the fused kernels of
esvit_amd/csrc/chunk_attn.hip (ops.sliding_chunk_attn_fwd / _bwd, bf16) and the dense route ops.vit_attn_fwd / _bwd(chunk=...) (batched
GEMMs + the row softmax of esvit_amd/csrc/vit_attn.hip, fp32 and bf16, plain table and span form), over the case table -- nglo 0 and 7,
L = 512 k and 512 k + 1, one-row and one-column grids, head_dim 48 on ragged grids, B != nH, planted scores of 300 -- every element of
every output under bounds derived from the number formats (the module docstring of tests/chunk_attn_ref.py lists them and the case ->
kernel table); and the row-softmax kernels alone on a prepared S with NaN in every pad.  tests/test_chunk_attn_exact_cpu.py proves the
cases, the bounds and the mutants they catch without a GPU.  Every err / bound ratio goes to golden_utils.record_parity; the device run
is committed as profiles/chunk_attn_exact_observed.jsonl, a record only."""
import pytest
import torch

from tests import chunk_attn_ref as R
from tests import golden_utils as GU

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64  # rows behind the B L the kernels write
CASE_IDS = [c["name"] for c in R.CASES]


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


def _nan_rows(rows, cols, dt):
    return torch.full((rows + GUARD, cols), float("nan"), dtype=dt, device=DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


# ---- the fused route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_fused_route_under_the_bounds(ops, case):
    """out, lse (directly) and dqkv per element; NaN-filled destinations with 64 guard rows: every live row finite and within bound (a
    row a kernel skips keeps its NaN), the guard rows untouched; two launches, equal bits"""
    x = R.inputs(case, BF16)
    B, nH, hd, L, nglo = case["B"], case["nH"], case["hd"], case["L"], case["nglo"]
    C = nH * hd
    assert ops.sliding_chunk_attn_supported(BF16, hd, R.W, nglo)
    qkv, dout = x["qkv"].to(DEV), x["dout"].to(DEV)
    lay = R.layout(case, DEV)

    def once():
        obuf, gbuf = _nan_rows(B * L, C, BF16), _nan_rows(B * L, 3 * C, BF16)
        out, saved = ops.sliding_chunk_attn_fwd(qkv, B, L, nH, x["scale"], lay, out=obuf)
        assert out.data_ptr() == obuf.data_ptr() and saved[1].data_ptr() == obuf.data_ptr()
        dqkv = ops.sliding_chunk_attn_bwd(dout, saved, B, L, nH, x["scale"], lay, dqkv=gbuf)
        assert dqkv.data_ptr() == gbuf.data_ptr()
        torch.cuda.synchronize()
        return obuf, saved[2], gbuf

    o1, l1, g1 = once()
    o2, l2, g2 = once()
    nan = _bits(torch.full((1,), float("nan"), dtype=BF16, device=DEV))
    m = R.metrics(case, BF16, "fused", R.unpack(case, out=o1, dqkv=g1, lse=l1))
    m["equal_finite"] = float(bool(torch.isfinite(o1[:B * L]).all()) and bool(torch.isfinite(g1[:B * L]).all()) and bool(torch.isfinite(l1).all()))
    m["equal_guard"] = float(bool((_bits(o1[B * L:]) == nan).all()) and bool((_bits(g1[B * L:]) == nan).all()))
    m["equal_repeat"] = float(torch.equal(_bits(o1), _bits(o2)) and torch.equal(l1, l2) and torch.equal(_bits(g1), _bits(g2)))
    R.check("fused", case, BF16, "fused", m, record=GU.record_parity, where="mi355x")


# ---- the dense route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [False, True], ids=["table", "span"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_dense_route_under_the_bounds(ops, case, dt, span):
    """out, P and dqkv per element; P exactly 0 wherever the mask forbids (the planted largest q.k of the stress cases is such a key) and
    on every pad row and pad column"""
    x = R.inputs(case, dt)
    B, nH, L = case["B"], case["nH"], case["L"]
    Np = R.pad_tokens(L)
    lay = R.layout(case, DEV, span=span)
    out, saved = ops.vit_attn_fwd(x["qkv"].to(DEV), B, L, nH, x["scale"], chunk=lay)
    dqkv = ops.vit_attn_bwd(x["dout"].to(DEV), saved, B, L, nH, x["scale"], chunk=lay)
    prob = saved[1]
    assert prob.shape == (B * nH, Np, Np) and prob.dtype == dt
    m = R.metrics(case, dt, "dense", R.unpack(case, out=out, dqkv=dqkv, attn=prob))
    forbidden = ~R.mask(case).to(DEV)
    m["equal_masked_zero"] = float(bool((prob[:, :L, :L][:, forbidden] == 0).all()))
    m["equal_pad_zero"] = float(bool((prob[:, L:, :] == 0).all()) and bool((prob[:, :, L:] == 0).all()))
    R.check("dense_span" if span else "dense_table", case, dt, "dense", m, record=GU.record_parity, where="mi355x")


# ---- the row-softmax kernels alone -------------------------------------------------------------------------------------------------
# N -> the grid behind one global token (N = 250: Np = 256, the last short row; N = 257: Np = 272, the first long row)
SOFTMAX_N = {5: (2, 2), 37: (6, 6), 197: (14, 14), 250: (3, 83), 257: (16, 16), 513: (16, 32), 785: (28, 28)}
SOFTMAX_Z = 3


def _softmax_case(N):
    nx, ny = SOFTMAX_N[N]
    return dict(name="softmax%d" % N, nx=nx, ny=ny, nglo=1, L=N, hd=0, B=1, nH=SOFTMAX_Z)


def _prepared(key, N, dt, std):
    """[Z, Np, Np] in dt: values in the live block, NaN in every pad row and pad column"""
    Np = R.pad_tokens(N)
    t = torch.full((SOFTMAX_Z, Np, Np), float("nan"), dtype=dt)
    t[:, :N, :N] = R.data(key, (SOFTMAX_Z, N, N), dt, std)
    return t


@pytest.mark.parametrize("form", ["none", "scan", "span"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.dt_name)
@pytest.mark.parametrize("N", sorted(SOFTMAX_N))
def test_softmax_rows_alone(ops, N, dt, form):
    """lib.esvit_softmax_rows_fwd / _bwd / _chunked_fwd / _chunked_bwd on a prepared S and dP against the fp64 softmax of the stored values.
    u = 2^-24, es = u (fp32) or 2^-9 (bf16), x = scale S - max, steps as in chunk_attn_ref:
      P    P (r + es), r = t + sum_k P_k t_k + (N + 3 + 4 steps) u, t = u |scale S| + (3 |x| + 2) u; or 3 x the error of torch's fp32 softmax
           over the same matrix (the device's __expf)
      dS   scale (P e_dot + 3 u P (|dP| + |dot|)) + es |dS|, e_dot = (N + 1) u sum_j P_j |dP_j|, of the P the device stored
    (bf16 doubles both); exactly 0 where the mask forbids and on every pad row and pad column, whatever the pads held"""
    case = _softmax_case(N)
    Np, Z, scale = R.pad_tokens(N), SOFTMAX_Z, 0.125
    bf = dt == BF16
    es, twice = (R.BF, 2.0) if bf else (R.U, 1.0)
    steps = -(-Np // (64 * (8 if bf else 4))) if Np > 256 else 0
    S = _prepared(("softmax", N, "s"), N, dt, 24.0)  # scale S of deviation 3: rows from flat to peaked
    dPm = _prepared(("softmax", N, "dp"), N, dt, 1.0)
    allowed = R.mask(case) if form != "none" else torch.ones(N, N, dtype=torch.bool)
    tab = R.table(case).to(DEV)
    nglo, rowtok = (1, R.W * case["ny"]) if form == "span" else (0, 0)
    lib, code = ops.lib, ops._code(dt)
    prob = S.to(DEV)
    if form == "none":
        ops.check(lib.esvit_softmax_rows_fwd(code, ops._p(prob), Z, N, Np, scale, ops._stream()), "softmax_rows_fwd")
    else:
        ops.check(lib.esvit_softmax_rows_chunked_fwd(code, ops._p(prob), Z, N, Np, scale, ops._p(tab), nglo, rowtok, ops._stream()), "softmax_rows_chunked_fwd")
    ds = dPm.to(DEV)
    if form == "span":
        ops.check(lib.esvit_softmax_rows_chunked_bwd(code, ops._p(prob), ops._p(ds), Z, N, Np, scale, ops._p(tab), nglo, rowtok, ops._stream()), "softmax_rows_chunked_bwd")
    else:
        ops.check(lib.esvit_softmax_rows_bwd(code, ops._p(prob), ops._p(ds), Z, N, Np, scale, ops._stream()), "softmax_rows_bwd")
    torch.cuda.synchronize()
    prob, ds = prob.cpu(), ds.cpu()
    # forward
    s64 = (scale * S[:, :N, :N].double()).masked_fill(~allowed, float("-inf"))
    mx = s64.max(-1, keepdim=True).values
    P = torch.softmax(s64, -1)
    xs = torch.where(allowed, (s64 - mx).abs(), 0.0)
    t = R.U * torch.where(allowed, s64.abs(), 0.0) + (3 * xs + 2) * R.U
    r = t + (P * t).sum(-1, keepdim=True) + (N + 3 + 4 * steps) * R.U
    p32 = torch.softmax((torch.tensor(scale, dtype=F32) * S[:, :N, :N].float()).masked_fill(~allowed, float("-inf")), -1).double()
    bd_P = torch.maximum(twice * P * (r + es), 3 * (p32 - P).abs().amax((1, 2), keepdim=True).expand_as(P)) + R.FLOOR
    got = prob.double()
    m = dict(ratio_attn=R.ratio(got[:, :N, :N], P, bd_P))
    m["equal_masked_zero"] = float(bool((got[:, :N, :N][:, ~allowed] == 0).all()))
    m["equal_pad_zero"] = float(bool((got[:, N:, :] == 0).all()) and bool((got[:, :, N:] == 0).all()))
    # backward, of the stored P
    Ps, dP = got[:, :N, :N], dPm[:, :N, :N].double()
    dot = (Ps * dP).sum(-1, keepdim=True)
    dS = scale * Ps * (dP - dot)
    e_dot = (N + 1) * R.U * (Ps * dP.abs()).sum(-1, keepdim=True)
    bd_dS = twice * (scale * (Ps * e_dot + 3 * R.U * Ps * (dP.abs() + dot.abs())) + es * dS.abs()) + R.FLOOR
    gds = ds.double()
    m["ratio_ds"] = R.ratio(gds[:, :N, :N], dS, bd_dS)
    m["equal_ds_pad_zero"] = float(bool((gds[:, N:, :] == 0).all()) and bool((gds[:, :, N:] == 0).all()) and bool((gds[:, :N, :N][:, ~allowed] == 0).all()))
    R.check("softmax_rows_" + form, case, dt, "dense", m, record=GU.record_parity, where="mi355x")
