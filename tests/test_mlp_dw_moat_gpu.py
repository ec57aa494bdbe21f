"""-m gpu: the on-chip weight-gradient mode of esvit_mlp_fused_bwd reads nothing but its operands.  x, gy and the two row-scale vectors
are contiguous row slices from the middle of larger buffers filled with NaN (offsets that keep the 16-byte alignment the kernel assumes):
a row read before or after the operand -- by the tile walk's clamp of the rows past M, or by a request for a tile the workgroup does not
have -- would reach a sum or an output.  Every output is finite and equals, bit for bit, that of the same call on plain tensors holding
the same values.  Row counts (G = workgroups of a full launch): one row; the tile edge 63 / 64 / 65; 64 G + 1, where one workgroup takes
a second tile holding a single valid row and no other has a next tile; 64 * 2G, two full tiles each; 64 * 2G + 67, a third ragged trip
for two workgroups."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 96
DT = torch.bfloat16
NAMES = ("gx", "gxa", "dW2", "db2", "G", "db1")
PAD_ROWS = 67   # rows of NaN before and after x / gy (67 * 384 bytes: 16-byte aligned)
PAD_VEC = 8     # floats of NaN before and after a row-scale vector (32 bytes)


@pytest.fixture(scope="module")
def ops(lib_built):
    from esvit_amd import ops
    return ops


def _grid(ops):
    G = ops.mlp_fused_dw_grid(DT, C, 1 << 40)
    assert G > 0
    return G


def _moated(t, pad):
    """a copy of t as a contiguous slice from the middle of a NaN-filled buffer"""
    buf = torch.full((t.shape[0] + 2 * pad,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=t.device)
    buf[pad:pad + t.shape[0]] = t
    view = buf[pad:pad + t.shape[0]]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return buf, view


_WEIGHTS = {}


def _weights(ops, dev):
    if not _WEIGHTS:
        g = torch.Generator().manual_seed(90)
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        W1f, W2f = (r(4 * C, C) * 0.08).to(dev), (r(C, 4 * C) * 0.05).to(dev)
        _WEIGHTS.update(gamma=(1.0 + 0.2 * r(C)).to(dev), beta=(0.1 * r(C)).to(dev), b1=(0.1 * r(4 * C)).to(dev),
                        K1=ops.mlp_fused_weight(ops.MLP_W1_BWD, W1f), K2T=ops.mlp_fused_weight(ops.MLP_W2T_BWD, W2f),
                        K1T=ops.mlp_fused_weight(ops.MLP_W1T_BWD, W1f))
    return _WEIGHTS


def _rows(case, G):
    return {"one": 1, "63": 63, "64": 64, "65": 65, "G+1row": 64 * G + 1, "2G": 64 * 2 * G, "2G+67": 64 * 2 * G + 67}[case]


@pytest.mark.parametrize("case", ["one", "63", "64", "65", "G+1row", "2G", "2G+67"])
def test_operands_inside_nan_buffers(ops, case):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dev = torch.device("cuda:0")
    M = _rows(case, _grid(ops))
    w = _weights(ops, dev)
    g = torch.Generator().manual_seed(91)
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(dev)
    gy = (torch.randn(M, C, generator=g) * 0.5).to(dev)
    rs_mlp = (torch.rand(M, generator=g) > 0.3).float().div(0.7).to(dev)
    rs_out = (torch.rand(M, generator=g) > 0.2).float().div(0.8).to(dev)

    def run(x_, gy_, rm, ro):
        outs = ops.mlp_fused_bwd_dw(x_, gy_, w["gamma"], w["beta"], 1e-6, w["K1"], w["K2T"], w["K1T"], w["b1"], rowscale_mlp=rm, rowscale_out=ro)
        return [t.clone() for t in outs]

    plain = run(x, gy, rs_mlp, rs_out)
    keep = [_moated(x, PAD_ROWS), _moated(gy, PAD_ROWS), _moated(rs_mlp, PAD_VEC), _moated(rs_out, PAD_VEC)]
    moated = run(*[view for _, view in keep])
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, moated, plain):
        assert bool(torch.isfinite(a.float()).all()), "%s: a non-finite value (M = %d): something outside the operands was read" % (name, M)
        assert bool(torch.isfinite(b.float()).all()), "%s: a non-finite value on plain tensors (M = %d)" % (name, M)
        assert torch.equal(a, b), "%s differs between operands inside NaN buffers and plain tensors (M = %d)" % (name, M)
    for buf, view in keep:  # the call wrote nothing around its inputs
        pad = (buf.shape[0] - view.shape[0]) // 2
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[-pad:]).all())
