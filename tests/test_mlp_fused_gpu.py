"""The fused MLP kernels on the MI355X (esvit_amd/csrc/mlp_fused.hip, mlp_fused16.hip, mlp_fused32p.hip, mlp_fused_dw.hip behind
esvit_mlp_fused_fwd / _fwd_train / _bwd, esvit_ln_fold_finish, esvit_cast_weight) against the fp64 statement of tests/mlp_fused_ref.py: all
twelve instantiations and the on-chip weight-gradient kernel at the row counts around a wave and a workgroup (one live wave in the last
workgroup among them), rows at mixed scales with row factors 0 on both sides of a wave boundary, selection-matrix weights that show every
hidden unit, channel and bias on its own, rows with |mean| = 100 std, constant rows, both eps, pre-activations over [-12, 12] -- every
element of every output under its bound and every 16-row group's rms error within 1.5 of the emulation's (the module docstring of
tests/mlp_fused_ref.py derives both and lists the case -> instantiation table).  The C ABI is called directly: every output is a slice of
a sentinel-filled buffer, every row-indexed input a slice of a NaN-filled one, every launch runs twice with the same bits.
tests/test_mlp_fused_cpu.py proves the statement, the bounds, the geometry and the mutants the cases catch without a GPU.  Every ratio
goes to golden_utils.record_parity; the device run is committed as profiles/mlp_fused_parity_observed.jsonl, a record only."""
import ctypes

import pytest
import torch

from tests import golden_utils as GU
from tests import mlp_fused_ref as MR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
PAD = 3
ERR_ARG, ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def env(lib_built):
    from esvit_amd import ops
    from esvit_amd._lib import lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ops, lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Moated:
    """a 16-byte-aligned slice of a larger buffer: at least PAD rows (elements of a vector) of `fill` on either side"""

    def __init__(self, shape, dt=torch.float32, fill=MR.SENTINEL, src=None):
        esz = torch.empty((), dtype=dt).element_size()
        row = esz * (shape[1] if len(shape) > 1 else 1)
        n, edge = shape[0], next(e for e in range(PAD, PAD + 17) if (e * row) % 16 == 0)
        self.buf = torch.full((n + 2 * edge,) + tuple(shape[1:]), fill, dtype=dt, device=DEV)
        self.t = self.buf[edge:edge + n]
        self.lo, self.hi, self.fill = edge, edge + n, fill
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()
        if src is not None:
            self.t.copy_(src)

    def intact(self):
        edge = torch.cat([self.buf[:self.lo].reshape(-1), self.buf[self.hi:].reshape(-1)])
        return bool((edge == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _rows_in(t):
    """a row-indexed input: the rows before 0 and from M on hold NaN"""
    return Moated(tuple(t.shape), t.dtype, float("nan"), src=t.to(DEV))


def _nan_edges(m):
    edge = torch.cat([m.buf[:m.lo].reshape(-1), m.buf[m.hi:].reshape(-1)])
    return bool(torch.isnan(edge).all())


def _launch(ops, lib, case, inp, dev):
    """one launch of the case's entry point into fresh sentinel buffers -> ({name: Moated}, the moated inputs)"""
    kind, C, M = case["kind"], case["C"], case["M"]
    H4 = 4 * C
    x, rs = _rows_in(inp["x"]), _rows_in(inp["rs"])
    ins = [x, rs]
    out = {}
    bf = BF16
    if kind in ("fwd", "train"):
        out["y"] = Moated((M, C))
        if kind == "fwd":
            nn = [None] * 5
            if case["nn"]:
                out.update(xw=Moated((M, C), bf), mean_n=Moated((M,)), rstd_n=Moated((M,)))
                nn = [dev["gamma_n"], dev["beta_n"], out["xw"].t, out["mean_n"].t, out["rstd_n"].t]
            rc = lib.esvit_mlp_fused_fwd(1, _p(x.t), _p(dev["gamma"]), _p(dev["beta"]), case["eps"], _p(dev["W1_FWD"]), _p(dev["b1"]), _p(dev["W2"]), _p(dev["b2"]),
                                         _p(rs.t), M, C, _p(out["y"].t), *[_p(t) for t in nn], _stream())
        else:
            out.update(a1=Moated((M, H4), bf), a1g=Moated((M, H4), bf), h=Moated((M, C), bf), mean=Moated((M,)), rstd=Moated((M,)))
            rc = lib.esvit_mlp_fused_fwd_train(1, _p(x.t), _p(dev["gamma"]), _p(dev["beta"]), case["eps"], _p(dev["W1_FWD"]), _p(dev["b1"]), _p(dev["W2"]),
                                               _p(dev["b2"]), _p(rs.t), M, C, *[_p(out[k].t) for k in ("y", "a1", "a1g", "h", "mean", "rstd")], _stream())
    else:
        gy, ro = _rows_in(inp["gy"]), _rows_in(inp["rs_out"])
        ins += [gy, ro]
        out.update(gx=Moated((M, C)), gx_act=Moated((M, C), bf))
        if kind == "bwd":
            out.update(xhat=Moated((M, C), bf), a1g=Moated((M, H4), bf), da1=Moated((M, H4), bf))
            tail, side = [None] * 5, [out[k].t for k in ("xhat", "a1g", "da1")]
        else:
            nws = ops.query(ops.Q_MLP_DW_WS, 1, C, M) // 4
            assert nws == MR.DW_PART * min(-(-M // MR.DW_T), MR.DW_CUS)
            ws = Moated((nws,))
            ws.t.fill_(float("nan"))  # (the partials need not be initialised)
            out.update(dW2=Moated((C, H4)), G=Moated((H4, C)), db1=Moated((H4,)), db2=Moated((C,)), ws=ws)
            tail, side = [out[k].t for k in ("dW2", "G", "db1", "db2", "ws")], [None] * 3
        rc = lib.esvit_mlp_fused_bwd(1, _p(x.t), _p(gy.t), _p(rs.t), _p(ro.t), _p(dev["gamma"]), _p(dev["beta"]), case["eps"], _p(dev["W1_BWD"]), _p(dev["W2T_BWD"]),
                                     _p(dev["W1T_BWD"]), _p(dev["b1"]), M, C, _p(out["gx"].t), _p(out["gx_act"].t), *[_p(t) for t in side], _stream(),
                                     *[_p(t) for t in tail])
    assert rc == 0, (case["name"], rc, lib.esvit_last_error())
    return out, ins


def run_device(ops, lib, case):
    """-> dict of fp64 CPU tensors (the statement's keys), equal_* flags and the ratios of the checks on the kernel's own outputs"""
    inp = MR.inputs(case)
    kind, C, M = case["kind"], case["C"], case["M"]
    dev = {k: inp[k].to(DEV) for k in ("gamma", "beta", "b1", "b2", "gamma_n", "beta_n")}
    W1f, W2f = inp["W1"].to(DEV), inp["W2"].to(DEV)
    if kind in ("fwd", "train"):
        dev["W1_FWD"], dev["W2"] = ops.mlp_fused_weight(ops.MLP_W1_FWD, W1f), ops.cast_weight(W2f)
        assert torch.equal(dev["W2"].cpu(), inp["W2"].to(BF16))
    else:
        for k in ("W1_BWD", "W2T_BWD", "W1T_BWD"):
            dev[k] = ops.mlp_fused_weight(getattr(ops, "MLP_" + k), W2f if k == "W2T_BWD" else W1f)
    out, ins = _launch(ops, lib, case, inp, dev)
    again, _ = _launch(ops, lib, case, inp, dev)
    torch.cuda.synchronize()
    flags = dict(equal_moat=float(all(m.intact() for m in out.values()) and all(m.intact() for m in again.values())),
                 equal_inputs_kept=float(all(_nan_edges(m) for m in ins)),
                 equal_repeat=float(all(torch.equal(out[k].t.view(torch.int16 if out[k].t.dtype == BF16 else torch.int32),
                                                    again[k].t.view(torch.int16 if again[k].t.dtype == BF16 else torch.int32)) for k in out if k != "ws")))
    raw = {k: m.t.detach().cpu() for k, m in out.items() if k != "ws"}
    got = {k: v.double() for k, v in raw.items()}
    rs, ro = inp["rs"], inp["rs_out"]
    if kind in ("fwd", "train"):
        z = rs == 0
        flags["equal_rowscale0_y_is_x"] = float(torch.equal(raw["y"][z].view(torch.int32), inp["x"][z].view(torch.int32)))  # bit for bit
        if case["nn"]:  # the triple against the LayerNorm of the kernel's own y
            own = MR.ln_stmt(got["y"], inp["gamma_n"].double(), inp["beta_n"].double(), MR._f32(case["eps"]), MR.ln_depth(kind, C))
            got["ratio_own_xw"] = MR.ratio(got["xw"], own["y"], 2.0 * (own["e_y"] + MR.BF * own["y"].abs()) + MR.FLOOR)
            got["ratio_own_mean_n"] = MR.ratio(got["mean_n"], own["mean"][:, 0], own["e_mean"][:, 0] + MR.FLOOR)
            got["ratio_own_rstd_n"] = MR.ratio(got["rstd_n"], own["rstd"][:, 0], own["e_rstd"][:, 0] + MR.FLOOR)
    else:
        z = rs == 0
        flags["equal_rowscale_mlp0_gx_is_gy"] = float(torch.equal(raw["gx"][z].view(torch.int32), inp["gy"][z].view(torch.int32)))  # bit for bit
        if kind == "bwd":
            flags["equal_rowscale_mlp0_da1_is_0"] = float(bool((raw["da1"][z] == 0).all()))
        flags["equal_rowscale_out0_gx_act_is_0"] = float(bool((raw["gx_act"][ro == 0] == 0).all()))
        v = (ro.view(M, 1) * raw["gx"]).double()  # one fp32 product, one bf16 rounding
        got["ratio_own_gx_act"] = MR.ratio(got["gx_act"], v, (2.0 ** -8 + 2 * MR.U) * v.abs() + 2.0 ** -126)
        if kind == "dw":
            got["ratio_db2_sum"] = MR.colsum_ratio(raw["db2"], (rs.view(M, 1) * inp["gy"]).to(BF16).float(), min(-(-M // MR.DW_T), MR.DW_CUS))
    got.update(flags)
    return got


def _params(kind, pick=None):
    return [pytest.param(c, id=c["name"]) for c in MR.CASES if c["kind"] == kind and (pick is None or pick(c))]


def _run_case(env, case):
    ops, lib = env
    if case["kind"] == "dw":
        assert ops.mlp_fused_dw_grid(BF16, 96, 1 << 40) == MR.DW_CUS  # the row counts of the table were made for this grid
    got = run_device(ops, lib, case)
    MR.check("device", case, MR.metrics(case, got, MR.reference(case)), record=GU.record_parity, where="mi355x")


@pytest.mark.parametrize("case", _params("fwd", lambda c: c["C"] != 384))
def test_forward_narrow(env, case):
    """fwd16_kernel<96 / 128 / 256, 8> and mlp_fused_fwd_kernel<192>, with and without the next LayerNorm"""
    _run_case(env, case)


@pytest.mark.parametrize("case", _params("fwd", lambda c: c["C"] == 384) + _params("train"))
def test_forward_wide(env, case):
    """mlp32p_fwd_kernel<384, SIDE>: the inference pass and the training pass with a1, a1g, h, mean, rstd; live hidden units in each
    peeled iteration of the software pipeline"""
    _run_case(env, case)


@pytest.mark.parametrize("case", _params("bwd"))
def test_backward(env, case):
    """bwd16_kernel<96,6,3> / <128,6,3> / <192,4,2> / <256,8,2>: gx, gx_act, xhat, a1g, da1"""
    _run_case(env, case)


@pytest.mark.parametrize("case", _params("dw"))
def test_backward_on_chip(env, case):
    """mlp_dw_kernel + mlp_dw_reduce_kernel: gx, gx_act and the four sums, from one tile to three tiles in one workgroup"""
    _run_case(env, case)


# ---- esvit_cast_weight, esvit_ln_fold_finish --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S,transpose,perm", [(37, 45, 0, 0), (37, 45, 1, 0), (37, 96, 0, 1), (64, 45, 1, 1), (288, 300, 1, 1)])
def test_cast_weight_is_the_documented_permutation_bit_for_bit(env, R, S, transpose, perm):
    _, lib = env
    assert (R * S) % 256  # the last pass of the grid-stride loop is ragged
    src = MR.data(("cast", R, S), (R, S))
    dst = Moated((S, R) if transpose else (R, S), BF16)
    assert lib.esvit_cast_weight(_p(src.to(DEV)), _p(dst.t), R, S, transpose, perm, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.t.cpu().view(torch.int16), MR.cast_weight_stmt(src, bool(transpose), bool(perm)).view(torch.int16)) and dst.intact()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("J,C", MR.FOLD_SHAPES)
def test_ln_fold_finish(env, J, C, accumulate):
    _, lib = env
    inp = MR.fold_inputs(J, C)
    d = {k: v.double() for k, v in inp.items() if k != "prev"}
    ref = MR.fold_stmt(d["G"], d["db"], d["W"], d["gamma"], d["beta"], prev=tuple(p.double() for p in inp["prev"]) if accumulate else None)
    runs = []
    for _ in range(2):
        Gm, dg, db = Moated((J, C), src=inp["G"].to(DEV)), Moated((C,), src=inp["prev"][0].to(DEV)), Moated((C,), src=inp["prev"][1].to(DEV))
        assert lib.esvit_ln_fold_finish(_p(Gm.t), _p(inp["db"].to(DEV)), _p(inp["W"].to(DEV)), _p(inp["gamma"].to(DEV)), _p(inp["beta"].to(DEV)), J, C, _p(dg.t),
                                        _p(db.t), accumulate, _stream()) == 0
        torch.cuda.synchronize()
        assert Gm.intact() and dg.intact() and db.intact()
        runs.append(dict(dW=Gm.t.cpu(), dgamma=dg.t.cpu(), dbeta=db.t.cpu()))
    m = {"ratio_" + k: MR.ratio(runs[0][k].double(), ref[k], ref["bd_" + k]) for k in ("dW", "dgamma", "dbeta")}
    m["equal_repeat"] = float(all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]))
    MR.check("ln_fold_finish", dict(name="fold_j%d_c%d_acc%d" % (J, C, accumulate)), m, record=GU.record_parity, where="mi355x")


# ---- refusals: argument checks on the host, nothing is launched and nothing is written ------------------------------------------------
def _small(ops, C, M=17):
    g = lambda *k, **kw: MR.data(("refuse", C) + k, **kw).to(DEV)  # noqa: E731
    H4 = 4 * C
    return dict(x=g("x", shape=(M + 1, C)), gy=g("gy", shape=(M + 1, C)), gamma=g("g", shape=(C + 4,)), beta=g("b", shape=(C,)), b1=g("b1", shape=(H4,)),
                b2=g("b2", shape=(C,)), W1=g("W1", shape=(H4, C), dt=BF16), W2=g("W2", shape=(C, H4), dt=BF16), W1T=g("W1T", shape=(C, H4), dt=BF16))


def _sentinels(C, M=17):
    H4 = 4 * C
    return dict(y=Moated((M, C)), xw=Moated((M, C), BF16), mean=Moated((M,)), rstd=Moated((M,)), a1=Moated((M, H4), BF16), a1g=Moated((M, H4), BF16),
                h=Moated((M, C), BF16), da1=Moated((M, H4), BF16))


def _off4(t):
    return ctypes.c_void_p(t.data_ptr() + 4)


def test_forward_refusals_launch_nothing(env):
    ops, lib = env
    C, M = 96, 17
    i, o = _small(ops, C), _sentinels(C)

    def call(dtype=1, x=None, b1=None, M_=M, C_=C, nn=(None,) * 5):
        return lib.esvit_mlp_fused_fwd(dtype, _p(i["x"]) if x is None else x, _p(i["gamma"]), _p(i["beta"]), 1e-6, _p(i["W1"]), b1 if b1 is not None else _p(i["b1"]),
                                       _p(i["W2"]), _p(i["b2"]), None, M_, C_, _p(o["y"].t), *nn, _stream())
    full = (_p(i["gamma"]), _p(i["beta"]), _p(o["xw"].t), _p(o["mean"].t), _p(o["rstd"].t))
    assert call(C_=160) == ERR_ARG and lib.esvit_last_error()
    assert call(dtype=0) == ERR_ARG
    assert call(M_=0) == ERR_ARG
    assert call(b1=ctypes.c_void_p(0)) == ERR_ARG
    assert call(x=_off4(i["x"])) == ERR_ARG
    assert call(nn=(_off4(i["gamma"]),) + full[1:]) == ERR_ARG
    for k in range(1, 5):  # a partial set of next-norm pointers
        assert call(nn=full[:k] + (None,) + full[k + 1:]) == ERR_ARG
    i3 = _small(ops, 384)
    o3 = _sentinels(384)
    assert lib.esvit_mlp_fused_fwd(1, _p(i3["x"]), _p(i3["gamma"]), _p(i3["beta"]), 1e-6, _p(i3["W1"]), _p(i3["b1"]), _p(i3["W2"]), _p(i3["b2"]), None, M, 384,
                                   _p(o3["y"].t), _p(i3["gamma"]), _p(i3["beta"]), _p(o3["xw"].t), _p(o3["mean"].t), _p(o3["rstd"].t), _stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert all(m.untouched() for m in o.values()) and all(m.untouched() for m in o3.values())


def test_training_pass_refusals_launch_nothing(env):
    ops, lib = env
    C, M = 384, 17
    i, o = _small(ops, C), _sentinels(C)

    def call(dtype=1, x=None, b1=None, M_=M, C_=C):
        return lib.esvit_mlp_fused_fwd_train(dtype, _p(i["x"]) if x is None else x, _p(i["gamma"]), _p(i["beta"]), 1e-6, _p(i["W1"]),
                                             b1 if b1 is not None else _p(i["b1"]), _p(i["W2"]), _p(i["b2"]), None, M_, C_,
                                             *[_p(o[k].t) for k in ("y", "a1", "a1g", "h", "mean", "rstd")], _stream())
    assert call(C_=160) == ERR_ARG and call(C_=192) == ERR_ARG
    assert call(dtype=0) == ERR_ARG
    assert call(M_=0) == ERR_ARG
    assert call(b1=ctypes.c_void_p(0)) == ERR_ARG
    assert call(x=_off4(i["x"])) == ERR_ARG
    first = -(-0x7ff00000 // (4 * C * 2))  # the first M whose side outputs pass the 32-bit offsets of the kernel's buffer stores
    assert (first - 1) * 4 * C * 2 < 0x7ff00000 <= first * 4 * C * 2
    assert call(M_=first) == ERR_UNSUPPORTED
    assert not ops.mlp_fused_train_supported(BF16, C, first) and ops.mlp_fused_train_supported(BF16, C, first - 1)
    torch.cuda.synchronize()
    assert all(m.untouched() for m in o.values())


def test_backward_refusals_launch_nothing(env):
    ops, lib = env
    C, M = 96, 17
    i, o = _small(ops, C), _sentinels(C)
    gx, gxa = Moated((M, C)), Moated((M, C), BF16)

    def call(dtype=1, x=None, b1=None, M_=M, C_=C):
        return lib.esvit_mlp_fused_bwd(dtype, _p(i["x"]) if x is None else x, _p(i["gy"]), None, None, _p(i["gamma"]), _p(i["beta"]), 1e-6, _p(i["W1"]), _p(i["W1"]),
                                       _p(i["W1T"]), b1 if b1 is not None else _p(i["b1"]), M_, C_, _p(gx.t), _p(gxa.t), _p(o["h"].t), _p(o["a1g"].t), _p(o["da1"].t),
                                       _stream(), None, None, None, None, None)
    assert call(C_=160) == ERR_ARG and call(C_=384) == ERR_ARG
    assert call(dtype=0) == ERR_ARG
    assert call(M_=0) == ERR_ARG
    assert call(b1=ctypes.c_void_p(0)) == ERR_ARG
    assert call(x=_off4(i["x"])) == ERR_ARG
    torch.cuda.synchronize()
    assert all(m.untouched() for m in o.values()) and gx.untouched() and gxa.untouched()


def test_cast_weight_refuses_a_permuted_length_off_the_32_block(env):
    _, lib = env
    src = MR.data(("refuse", "cast"), (64, 48)).to(DEV)
    dst = Moated((64, 48), BF16)
    assert lib.esvit_cast_weight(_p(src), _p(dst.t), 64, 48, 0, 1, _stream()) == ERR_ARG
    assert lib.esvit_cast_weight(_p(src), _p(dst.t), 48, 64, 1, 1, _stream()) == ERR_ARG
    assert lib.esvit_cast_weight(None, _p(dst.t), 64, 48, 0, 0, _stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert dst.untouched()
