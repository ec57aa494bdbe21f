"""Window attention on the MI355X (esvit_amd/csrc/window_attn.hip, window_attn_big.hip behind ops.window_attn_fwd / window_attn_bwd /
relpos_bias_bwd) against the fp64 statement of tests/window_attn_ref.py: the case table -- wave pairs that walk several windows with the
mask on, pads and an inactive tail in the last round, both head dims, 6 x 6 / 3 x 3 windows with dead key tiles, the 224-slot kernels,
scores beyond the range of fp32 exp, the partial grid with a non-zero table -- in both dtypes, every output compared per element under
bounds derived from the number formats (the module docstring of tests/window_attn_ref.py lists them and the case -> kernel table).
tests/test_window_attn_cpu.py proves the cases, the bounds and the mutants they catch without a GPU.  Every err / bound ratio goes to
golden_utils.record_parity; the device run is committed as profiles/window_attn_parity_observed.jsonl, a record only."""
import pytest
import torch

from tests import golden_utils as GU
from tests import window_attn_ref as WR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops


def _params(prefixes):
    ps = [p for p in WR.params() if p[0]["name"].startswith(prefixes)]
    return [pytest.param(c, dt, id="%s-%s" % (c["name"], WR.dt_name(dt))) for c, dt in ps]


def _check(entry, case, dt, m):
    WR.check(entry, case, dt, m, record=GU.record_parity, where="mi355x")


def _run_case(ops, case, dt):
    """the probability variant (with a second launch for the bits) and the training variant; on 14 x 14 windows also the separate
    bias-gradient kernel (bf16) and, at head_dim 64, the backward without slabs"""
    g = WR.geometry(case)
    got = WR.run_attention(ops, DEV, case, dt, want_attn=True, repeat=True)
    assert got["parts"] == WR.walk(case)["bwd"][0], (got["parts"], WR.walk(case))
    _check("probabilities", case, dt, WR.metrics(case, dt, got))
    got = WR.run_attention(ops, DEV, case, dt, want_attn=False)
    _check("training", case, dt, WR.metrics(case, dt, got))
    if g["N"] > 64 and dt == torch.bfloat16:
        got = WR.run_attention(ops, DEV, case, dt, want_attn=False, ws_flags=ops.ATTN_SPLIT_DBIAS)
        _check("split_dbias", case, dt, WR.metrics(case, dt, got))
        if case["hd"] == 64:
            got = WR.run_attention(ops, DEV, case, dt, want_attn=False, want_dbias=False)
            assert got["dtable"] is None
            _check("no_dbias", case, dt, WR.metrics(case, dt, got))


@pytest.mark.parametrize("case,dt", _params("walk"))
def test_walk_cases(ops, case, dt):
    """wave pairs that own several windows: mask, slot map, bias-gradient slabs and pad-row sums across the walk, with the tail of the
    last round inactive"""
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params("range"))
def test_range_cases(ops, case, dt):
    """scores beyond 89 (exp without the maximum overflows), masked keys that keep probability (-100 is not -inf), bias-dominated scores"""
    _run_case(ops, case, dt)


@pytest.mark.parametrize("case,dt", _params("partial_grid"))
def test_partial_grid(ops, case, dt):
    """N = 37 of a 7 x 7 grid with a non-zero table: forward, backward and the table gradient (relpos_bias_bwd is handed the full
    [49, 49] index and takes its [:N, :N] block)"""
    _run_case(ops, case, dt)


def test_relpos_bias_bwd_takes_the_block_of_the_full_index(ops):
    """the fold kernel reads index[q * N + key]: before the wrapper sliced, the full [ws^2, ws^2] buffer at N < ws^2 gave the gradient
    of other table rows without a word"""
    case = WR.BY_NAME["partial_grid"]
    g, ref = WR.geometry(case), WR.reference(case, torch.float32)
    N, nH = g["N"], case["nH"]
    from oracle import ops_ref
    slab = ops_ref.dense_to_frag(ref["dbias"].float()).unsqueeze(0).contiguous().to(DEV)
    full = ops.relpos_bias_bwd(slab, g["index"].to(DEV), N, g["trows"]).cpu().double()
    block = ops.relpos_bias_bwd(slab, g["index"][:N, :N].contiguous().to(DEV), N, g["trows"]).cpu().double()
    bound = N * WR.U * ref["ab_dtable"] + WR.U * ref["dtable"].abs() + WR.FLOOR  # the fp32 slab, then at most N atomics per row and head
    m = dict(ratio_full=WR.ratio(full, ref["dtable"], bound), ratio_block=WR.ratio(block, ref["dtable"], bound))
    _check("relpos_full_index", case, torch.float32, m)
    with pytest.raises(AssertionError):
        ops.relpos_bias_bwd(slab, g["index"][:N, :N].to(torch.int32).contiguous().to(DEV), N, g["trows"])


# ---- calling conventions of the training step, bit for bit against plain calls ------------------------------------------------------------------
def _conv_inputs(ops, ws, H, shift, nH, hd, nB, dt, seed):
    tok, reg = WR.window_geometry(H, H, ws, shift)
    N, L, nW, C = ws * ws, H * H, tok.shape[0], nH * hd
    return dict(qkv=WR.data(("conv", seed, "qkv"), (nB * L, 3 * C), dt).to(DEV), dout=WR.data(("conv", seed, "do"), (nB * L, C), dt).to(DEV),
                qb=WR.data(("conv", "qb"), (3 * C,), torch.float32, 0.5).to(DEV), table=WR.data(("conv", "tab"), ((2 * ws - 1) ** 2, nH), torch.float32, 0.5).to(DEV),
                w2t=tok.reshape(-1).to(torch.int32).to(DEV), reg=reg.reshape(-1).to(torch.int32).to(DEV), index=WR.rel_index(ws).to(DEV),
                N=N, L=L, nW=nW, C=C, nB=nB, nH=nH, ws=ws, scale=WR._f32(hd ** -0.5), trows=(2 * ws - 1) ** 2)


def _fwd(ops, x, table, **kw):
    return ops.window_attn_fwd(x["qkv"], x["qb"], x["w2t"], x["L"], table, x["ws"], x["reg"], x["nW"], x["N"], x["nH"], x["scale"], **kw)


def _bwd(ops, x, out, lse, table, **kw):
    return ops.window_attn_bwd(x["qkv"], x["qb"], x["w2t"], x["L"], x["dout"], out, lse, table, x["ws"], x["reg"], x["nW"], x["N"], x["nH"], x["scale"], **kw)


def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


CONV_GEOMS = [pytest.param(7, 12, 3, id="w7"), pytest.param(14, 24, 7, id="w14")]


@pytest.mark.parametrize("dt", WR.DTYPES, ids=WR.dt_name)
@pytest.mark.parametrize("ws,H,shift", CONV_GEOMS)
def test_prefilled_bias_fragment(ops, ws, H, shift, dt):
    """forward with the table and a caller's bias_frag, then forward and backward with rel_table=None: the bits of the plain calls, with the
    shared scratch the plain calls refill poisoned in between"""
    x = _conv_inputs(ops, ws, H, shift, 3, 32, 2, dt, 1)
    o0, l0 = _fwd(ops, x, x["table"])
    dq0, sl0, pad0 = (t.clone() for t in _bwd(ops, x, o0, l0, x["table"]))
    frag = ops.new_bias_frag(x["nH"], x["N"], DEV)
    o1, l1 = _fwd(ops, x, x["table"], bias_frag=frag)
    ops.workspace(2 * x["nH"] * ops.attn_frag_elems(x["N"]), DEV, slot=2).fill_(float("nan"))
    o2, l2 = _fwd(ops, x, None, bias_frag=frag)
    dq2, sl2, pad2 = _bwd(ops, x, o2, l2, None, bias_frag=frag)
    assert torch.equal(o0, o1) and torch.equal(o0, o2) and _same(l0, l1) and _same(l0, l2)
    assert torch.equal(dq0, dq2) and torch.equal(sl0, sl2) and torch.equal(pad0, pad2)


@pytest.mark.parametrize("dt", WR.DTYPES, ids=WR.dt_name)
@pytest.mark.parametrize("ws,H,shift", CONV_GEOMS)
def test_outputs_into_row_slices(ops, ws, H, shift, dt):
    """out= and dqkv_out= as row slices of larger NaN-filled buffers: the bits of the plain calls inside, the rows outside untouched"""
    x = _conv_inputs(ops, ws, H, shift, 3, 32, 2, dt, 2)
    rows, C, above = x["nB"] * x["L"], x["C"], 5
    o0, l0 = _fwd(ops, x, x["table"])
    dq0 = _bwd(ops, x, o0, l0, x["table"])[0].clone()
    obuf = torch.full((rows + 12, C), float("nan"), dtype=dt, device=DEV)
    gbuf = torch.full((rows + 12, 3 * C), float("nan"), dtype=dt, device=DEV)
    o1, l1 = _fwd(ops, x, x["table"], out=obuf[above:above + rows])
    dq1 = _bwd(ops, x, o1, l1, x["table"], dqkv_out=gbuf[above:above + rows])[0]
    assert o1.data_ptr() == obuf[above].data_ptr() and dq1.data_ptr() == gbuf[above].data_ptr()
    assert torch.equal(obuf[above:above + rows], o0) and torch.equal(gbuf[above:above + rows], dq0) and _same(l0, l1)
    for buf in (obuf, gbuf):
        assert bool(torch.isnan(buf[:above]).all()) and bool(torch.isnan(buf[above + rows:]).all())


@pytest.mark.parametrize("dt", WR.DTYPES, ids=WR.dt_name)
@pytest.mark.parametrize("ws,H,shift", CONV_GEOMS)
def test_two_backward_calls_into_one_slab_buffer(ops, ws, H, shift, dt):
    """two backward calls with different nB into attn_dbias_slabs: each writes the bits of its plain call into its slice; one
    relpos_bias_bwd over the buffer equals the sum of the two separate folds, accumulate=True adds onto a prefilled gradient and
    accumulate=False overwrites it.  The fold scatters with atomics, whose order is free: these three are held to
    (parts + N + 8) u of the folded |slabs|, both sides of the comparison counted"""
    xa, xb = _conv_inputs(ops, ws, H, shift, 3, 32, 2, dt, 3), _conv_inputs(ops, ws, H, shift, 3, 32, 5, dt, 4)
    N, nH, trows = xa["N"], xa["nH"], xa["trows"]
    plain = []
    for x in (xa, xb):
        o, l = _fwd(ops, x, x["table"])
        plain.append((o, l, _bwd(ops, x, o, l, x["table"])[1].clone()))
    buf, slices = ops.attn_dbias_slabs(N, [x["nB"] * x["nW"] for x in (xa, xb)], nH, DEV)
    buf.fill_(float("nan"))
    for x, (o, l, _), sl in zip((xa, xb), plain, slices):
        got = _bwd(ops, x, o, l, x["table"], dbias_out=sl)[1]
        assert got.data_ptr() == sl.data_ptr()
    assert buf.shape[0] == sum(p[2].shape[0] for p in plain) and torch.equal(buf, torch.cat([p[2] for p in plain]))
    both = ops.relpos_bias_bwd(buf, xa["index"], N, trows).double()
    parts = [ops.relpos_bias_bwd(p[2], xa["index"], N, trows).double() for p in plain]
    mag = ops.relpos_bias_bwd(buf.abs(), xa["index"], N, trows).double()
    bound = 2 * (buf.shape[0] + N + 8) * WR.U * mag + WR.FLOOR
    assert bool(((both - (parts[0] + parts[1])).abs() <= bound).all())
    base = WR.data(("conv", "base"), (trows, nH), torch.float32).to(DEV)
    acc = base.clone()
    assert ops.relpos_bias_bwd(buf, xa["index"], N, trows, out=acc, accumulate=True).data_ptr() == acc.data_ptr()
    assert bool(((acc.double() - (base.double() + both)).abs() <= bound + 2 * WR.U * base.double().abs()).all())
    ops.relpos_bias_bwd(buf, xa["index"], N, trows, out=acc, accumulate=False)
    assert bool(((acc.double() - both).abs() <= bound).all())
