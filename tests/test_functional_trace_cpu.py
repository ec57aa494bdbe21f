"""Which kernels esvit_amd.functional launches, on which shapes, in which order -- pinned for every block family and every DINO head
on the CPU restatement of the kernels (oracle/ops_ref.py) -- and the launch policy all of them share: weight gradients on the side
stream behind one join, every parameter gradient written into its bucket slot.

tests/golden/functional_trace.json holds the ordered trace of one forward + backward per case.  `python -m
tests.test_functional_trace_cpu` rewrites it from the working tree: do that only for a change that is MEANT to launch other kernels."""
import json
import os

import pytest
import torch

from oracle import ops_ref
from tests.test_composition_cpu import cpu_ops  # noqa: F401  (fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "functional_trace.json")
OUTPUT_BUFFERS = ("out", "db_out", "gb_out", "dv_out", "dqkv_out", "dbias_out")
# not launches: shape predicates and host-side tables
HOST = ("act_dtype", "set_act_dtype", "window_maps", "shift_region_ids", "relative_position_index", "conv_out_size")
WIDE_C = 384
CPU = torch.device("cpu")


def _sig(v):
    if isinstance(v, torch.Tensor):
        return "%s%s" % (str(v.dtype)[6:], list(v.shape))
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(_sig(e) for e in v) + ")"
    if isinstance(v, float):
        return "%.9g" % v
    if v is None or isinstance(v, (bool, int, str)):
        return repr(v)
    return type(v).__name__


class Recorder:
    """the ops module behind a proxy that notes every launch: name, dtype and shape of the tensor arguments, the scalars; keywords
    that only name an output buffer are dropped, and so are keywords left at None / False (the default of every such keyword of the
    ops).  `side`: was the call made inside functional._side_run.  `muted`: inside params.cached_cast / params.cached -- the
    activation-dtype copies of the parameters are cache fills, made whenever a forward first asks for one, and not part of the trace"""

    def __init__(self, base, over=None):
        self._base, self._over, self.trace, self.side, self.muted = base, over or {}, [], False, 0

    def __getattr__(self, name):
        attr = self._over[name] if name in self._over else getattr(self._base, name)
        if not callable(attr) or name.endswith("_supported") or name in HOST:
            return attr

        def call(*a, **k):
            kw = ["%s=%s" % (n, _sig(k[n])) for n in sorted(k) if n not in OUTPUT_BUFFERS and k[n] is not None and k[n] is not False]
            if not self.muted:
                self.trace.append(("%s(%s%s)" % (name, ", ".join(_sig(v) for v in a), "; " + ", ".join(kw) if kw else ""), self.side))
            return attr(*a, **k)
        return call


class Session:
    """functional (and head, params, loss) on a Recorder, the route switches pinned to their defaults, _side_run / _side_join and
    every Function's backward wrapped: `unjoined` lists the nodes that returned with side-stream work nobody had joined"""

    def __init__(self, mp, Fn, wide=False, route=None):
        import esvit_amd.loss as L
        import esvit_amd.params as P
        self.Fn, self.P = Fn, P
        over = {"mlp_fused_train_supported": lambda dt, Cc, rows=0: dt == torch.bfloat16 and Cc == WIDE_C} if wide else {}
        over.update(STUBS[route]() if route else {})
        self.rec = rec = Recorder(ops_ref, over)
        for mod in (Fn, L, P):
            mp.setattr(mod, "ops", rec)
        for name, val in (("ATTN_FUSED", True), ("ATTN_BWD_FUSED", False), ("MLP_FUSED_TRAIN", True), ("MLP_WIDE_FUSED", True),
                          ("MLP_WIDE_TRAIN", wide), ("MLP_DW_ONCHIP", True), ("VIT_LONG_ATTENTION", "flash" if route == "flash" else "gemm")):
            mp.setattr(Fn, name, val)
        for name in ("cached_cast", "cached"):
            mp.setattr(P, name, self._muted(getattr(P, name)))
        self.pending, self.unjoined = False, []
        run0, join0 = Fn._side_run, Fn._side_join

        def side_run(fn, *keep):
            rec.side, self.pending = True, True
            try:
                return run0(fn, *keep)
            finally:
                rec.side = False

        def side_join(*a, **k):
            self.pending = False
            return join0(*a, **k)
        mp.setattr(Fn, "_side_run", side_run)
        mp.setattr(Fn, "_side_join", side_join)
        for name, cls in vars(Fn).items():
            if isinstance(cls, type) and issubclass(cls, torch.autograd.Function):
                mp.setattr(cls, "backward", staticmethod(self._checked(name, cls.backward)))
        self.reset()

    def _muted(self, fill):
        def run(*a, **k):
            self.rec.muted += 1
            try:
                return fill(*a, **k)
            finally:
                self.rec.muted -= 1
        return run

    def _checked(self, name, backward):
        def run(*a):
            out = backward(*a)
            if self.pending:
                self.unjoined.append(name)
                self.pending = False
            return out
        return run

    def reset(self):
        self.P.clear()
        self.Fn._GEOM.clear()
        del self.rec.trace[:]
        del self.unjoined[:]


# ---- attention routes the restatement does not have: stand-ins over its dense route, handed to the Recorder as `over`.  What such a
# route's forward returns for the backward is a contract of its own: every stand-in's backward insists on the very tensors its forward
# returned ------------------------------------------------------------------------------------------------------------------------------
def _returned(kept, saved):
    assert any(len(k) == len(saved) and all(a is b for a, b in zip(k, saved)) for k in kept), [_sig(t) for t in saved]


def _dense_stubs(fwd_name, bwd_name, sup_name, with_chunk):
    """`fwd_name` -> (ao, (qkv, ao, lse [nB, nH, N])) and `bwd_name` of it, computed by ops_ref.vit_attn_fwd / _bwd"""
    kept, dense = [], {}

    def fwd(qkv, nB, N, nH, scale, *chunk, out=None):
        assert len(chunk) == with_chunk
        ao, att = ops_ref.vit_attn_fwd(qkv, nB, N, nH, scale, *chunk)
        if out is not None:
            out.copy_(ao)
            ao = out
        lse = torch.zeros(nB, nH, N)
        kept.append((qkv, ao, lse))
        dense[id(lse)] = att
        return ao, kept[-1]

    def bwd(dao, saved, nB, N, nH, scale, *chunk, dqkv=None):
        assert len(chunk) == with_chunk
        _returned(kept, saved)
        dq = ops_ref.vit_attn_bwd(dao, dense[id(saved[2])], nB, N, nH, scale, *chunk)
        if dqkv is not None:
            dqkv.copy_(dq)
            dq = dqkv
        return dq
    return {fwd_name: fwd, bwd_name: bwd, sup_name: lambda *a: True}


def _window_lse_stubs():
    """the 224-slot kernels' log-sum-exp: windows of more than 64 tokens return one, and the backward is handed that tensor"""
    kept = []

    def fwd(qkv, qkv_bias, win2tok, L, table, ws, region_ids, nW, N, nH, scale, **k):
        ao = ops_ref.window_attn_fwd(qkv, qkv_bias, win2tok, L, table, ws, region_ids, nW, N, nH, scale, **k)[0]
        lse = torch.zeros(qkv.shape[0] // L * nW, nH, N) if N > 64 else None
        kept.append((qkv, ao, lse, k.get("bias_frag")))
        return ao, lse

    def bwd(qkv, qkv_bias, win2tok, L, dout, fwd_out, lse, *a, **k):
        assert (lse is not None) == (a[4] > 64)
        _returned(kept, (qkv, fwd_out, lse, k.get("bias_frag")))
        return ops_ref.window_attn_bwd(qkv, qkv_bias, win2tok, L, dout, fwd_out, lse, *a, **k)
    return {"window_attn_fwd": fwd, "window_attn_bwd": bwd}


STUBS = {"flash": lambda: _dense_stubs("global_attn_fwd", "global_attn_bwd", "global_attn_supported", 0),
         "chunk_fused": lambda: _dense_stubs("sliding_chunk_attn_fwd", "sliding_chunk_attn_bwd", "sliding_chunk_attn_supported", 1),
         "window lse": _window_lse_stubs}


def _route(name):
    """the stand-ins a case asks for by its name"""
    return next((r for r in STUBS if r in name), None)


# ---- the cases: name -> run(Fn) -> (outputs, parameters); every case draws its inputs from its own seeded generator -------------------
def _rand(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g)


def _param(*ts):
    return [None if t is None else torch.nn.Parameter(t) for t in ts]


def _drop(r, n, per):
    """DropPath factors of n samples at keep 0.7 (the first sample dropped), one per row of `per` rows each"""
    f = (r(n) > -0.5).float() / 0.7
    f[0] = 0.0
    return f, f.repeat_interleave(per)


def _finish(ys, xs, prm, r, grad):
    y = torch.cat([t.reshape(-1, t.shape[-1]) for t in ys])
    if grad:
        (y.float() * r(*y.shape)).sum().backward()
    return [y.detach()] + [x.grad for x in xs if grad], [p for p in prm if p is not None]


def _mlp_prm(r, C, H):
    return (1 + 0.1 * r(C), 0.1 * r(C), r(H, C) * C ** -0.5, 0.1 * r(H), r(C, H) * H ** -0.5, 0.1 * r(C))


def _attn_prm(r, C, rows=3):
    return (1 + 0.1 * r(C), 0.1 * r(C), r(rows * C, C) * C ** -0.5, 0.1 * r(rows * C))


SWIN_GROUPS = ((2, 14, 3), (2, 7, 0))  # (images, token grid side, shift): 14x14 shifted and 7x7, window 7


def swin_case(multi, C, nH, dt, dp, grad, groups=SWIN_GROUPS):
    def run(Fn, arm=None):
        ops_ref.set_act_dtype(dt)
        r = _rand(C + 2 * multi + 4 * dp)
        a, m = _attn_prm(r, C), _mlp_prm(r, C, 4 * C)
        prm = _param(a[0], a[1], 0.2 * r(169, nH), a[2], a[3], r(C, C) * C ** -0.5, 0.1 * r(C), *m)
        arm and arm(prm)
        index = torch.from_numpy(ops_ref.relative_position_index(7))
        xs = [r(nB, S * S, C).requires_grad_(grad) for nB, S, _ in groups]
        geoms = [Fn.geometry(S, S, 7, sh, CPU) for _, S, sh in groups]
        dps = [(_drop(r, nB, S * S), _drop(r, nB, S * S)) for nB, S, _ in groups] if dp else None
        with torch.set_grad_enabled(grad):
            if multi:
                segs, r0 = [], 0
                for (nB, S, _), geom in zip(groups, geoms):
                    segs.append((r0, nB, S * S, geom))
                    r0 += nB * S * S
                dp_rows = tuple(torch.cat([d[k][1] for d in dps]) for k in (0, 1)) if dp else None
                ys = [Fn.swin_block_multi(torch.cat([x.view(-1, C) for x in xs]), tuple(segs), nH, index, dp_rows, prm)[0]]
            else:
                ys = [Fn.swin_block(x, geom, nH, index, (dps[i][0][0], dps[i][1][0]) if dp else None, prm) for i, (x, geom) in enumerate(zip(xs, geoms))]
            return _finish(ys, xs, prm, r, grad)
    return run


VIT_GROUPS = ((2, 5), (2, 10))  # (images, tokens)


def vit_case(multi, dt, grad, groups=VIT_GROUPS, C=192, nH=3):
    def run(Fn, arm=None):
        ops_ref.set_act_dtype(dt)
        r = _rand(7 + multi)
        a = _attn_prm(r, C)
        prm = _param(*a, r(C, C) * C ** -0.5, 0.1 * r(C), *_mlp_prm(r, C, 4 * C))
        arm and arm(prm)
        xs = [r(nB, N, C).requires_grad_(grad) for nB, N in groups]
        dps = [(_drop(r, nB, N), _drop(r, nB, N)) for nB, N in groups]
        with torch.set_grad_enabled(grad):
            if multi:
                segs, r0 = [], 0
                for nB, N in groups:
                    segs.append((r0, nB, N))
                    r0 += nB * N
                dp_rows = tuple(torch.cat([d[k][1] for d in dps]) for k in (0, 1))
                ys = [Fn.vit_block_multi(torch.cat([x.view(-1, C) for x in xs]), tuple(segs), nH, dp_rows, prm)]
            else:
                ys = [Fn.vit_block(x, nH, (dps[i][0][0], dps[i][1][0]), prm) for i, x in enumerate(xs)]
            return _finish(ys, xs, prm, r, grad)
    return run


def vil_case(split, dt, grad, C=96, nH=3, nB=2, fused=False):
    """one global token and a 4 x 4 grid of local tokens in 2 x 2 chunks; split: query | kv Linears and the dense chunk route, or
    with `fused` the 4-tuple that asks for the fused sliding-chunk kernels"""
    def run(Fn, arm=None):
        ops_ref.set_act_dtype(dt)
        r = _rand(11 + split)
        N = 17
        if split:
            q, kv = _attn_prm(r, C, 1), _attn_prm(r, C, 2)
            attn = (q[0], q[1], q[2], q[3], kv[2], kv[3])
            chunk = torch.tensor([-1] + [((i // 4 // 2) << 16) | (i % 4 // 2) for i in range(16)], dtype=torch.int32)
            chunk = (chunk, 1, 2 * 4, 2) if fused else chunk
        else:
            attn, chunk = _attn_prm(r, C) + (None, None), None
        prm = _param(*attn, r(C, C) * C ** -0.5, 0.1 * r(C), *_mlp_prm(r, C, 4 * C))
        arm and arm(prm)
        x = r(nB, N, C).requires_grad_(grad)
        dp = (_drop(r, nB, N)[0], _drop(r, nB, N)[0])
        with torch.set_grad_enabled(grad):
            return _finish([Fn.vil_block(x, nH, dp, chunk, prm)], [x], prm, r, grad)
    return run


CVT_GROUPS = ((2, 16), (2, 9))  # (images, tokens)


def cvt_ffn_case(multi, dt, grad, groups=CVT_GROUPS, C=64):
    def run(Fn, arm=None):
        ops_ref.set_act_dtype(dt)
        r = _rand(17 + multi)
        m = _mlp_prm(r, C, 4 * C)
        prm = _param(m[0], m[1], m[2].view(4 * C, C, 1, 1), m[3], m[4].view(C, 4 * C, 1, 1), m[5])
        arm and arm(prm)
        xs = [r(nB, N, C).requires_grad_(grad) for nB, N in groups]
        dps = [_drop(r, nB, N) for nB, N in groups]
        with torch.set_grad_enabled(grad):
            if multi:
                ys = [Fn.CvtFfnMultiFn.apply(torch.cat([x.view(-1, C) for x in xs]), torch.cat([d[1] for d in dps]), *prm)]
            else:
                ys = [Fn.CvtFfnFn.apply(x, d[0], *prm) for x, d in zip(xs, dps)]
            return _finish(ys, xs, prm, r, grad)
    return run


HEAD_ROWS, HEAD_IN, HEAD_HIDDEN, HEAD_NECK, HEAD_OUT = 128, 32, 64, 32, 128  # (rows and outputs the statistics epilogue covers)


def head_case(L, bn, stats, grad=True):
    def run(Fn, arm=None):
        from esvit_amd import head as H
        ops_ref.set_act_dtype(torch.bfloat16)
        r = _rand(23 + L)
        head = H.DINOHead(HEAD_IN, HEAD_OUT, use_bn=bn, nlayers=L, hidden_dim=HEAD_HIDDEN, bottleneck_dim=HEAD_NECK).train()
        with torch.no_grad():
            for p in head.parameters():
                if p is not head.last_layer.weight_g:
                    p.copy_(r(*p.shape) * (0.1 if p.dim() == 1 else p.shape[-1] ** -0.5) + (1.0 if (bn and p.dim() == 1 and p.shape[0] == HEAD_HIDDEN) else 0.0))
        arm and arm(list(head.parameters()))
        if stats:
            head.logit_stats = (25.0, 0.1 * r(HEAD_OUT), "token")
        x = r(HEAD_ROWS, HEAD_IN).requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            y = head(x)
            assert (getattr(y, "esvit_row_stats", None) is not None) == stats
            outs, prm = _finish([y], [x], list(head.parameters()), r, grad)
        return outs + [b.detach().clone().float() for b in head.buffers()], prm
    return run


VIT_LONG_GROUPS = ((2, 5), (1, 230))  # 5 tokens: the 64-slot windowed route; 230: beyond the windowed kernels (batched GEMM, or flash)
VIT_LSE_GROUPS = ((2, 5), (1, 65))     # 65 tokens: the windowed route that carries a log-sum-exp


def cases():
    """name -> (run, wide route forced).  Names: family / shape / dtype / mode; a name that holds a key of STUBS runs on those
    stand-ins (_route)"""
    out = {}
    for multi in (False, True):
        fam = "swin_block_multi" if multi else "swin_block"
        for C, nH, dt, tag in ((96, 3, torch.float32, "fp32 plain"), (96, 3, torch.bfloat16, "bf16 fused"), (WIDE_C, 12, torch.bfloat16, "bf16 wide")):
            for dp in (False, True):
                for grad in (True, False):
                    out["%s C=%d %s%s %s" % (fam, C, tag, " droppath" if dp else "", "grad" if grad else "no_grad")] = (
                        swin_case(multi, C, nH, dt, dp, grad), C == WIDE_C)
        for dt in (torch.bfloat16, torch.float32):
            for grad in (True, False):
                mode = "%s %s" % (str(dt)[6:], "grad" if grad else "no_grad")
                vit = "vit_block_multi" if multi else "vit_block"
                out["%s C=192 %s" % (vit, mode)] = (vit_case(multi, dt, grad), False)
                out["%s C=48 gemm %s" % (vit, mode)] = (vit_case(multi, dt, grad, C=48), False)  # head_dim 16: no fused kernel takes it
                if grad:
                    out["%s C=96 window+gemm %s" % (vit, mode)] = (vit_case(multi, dt, grad, VIT_LONG_GROUPS, C=96), False)
                if dt == torch.bfloat16:
                    out["%s C=96 window+flash %s" % (vit, mode)] = (vit_case(multi, dt, grad, VIT_LONG_GROUPS, C=96), False)
                    if grad:
                        out["%s C=96 window lse %s" % (vit, mode)] = (vit_case(multi, dt, grad, VIT_LSE_GROUPS, C=96), False)
                out["%s %s" % ("CvtFfnMultiFn" if multi else "CvtFfnFn", mode)] = (cvt_ffn_case(multi, dt, grad), False)
                if multi:
                    continue
                for split in (False, True):
                    out["vil_block %s %s" % ("query|kv chunked" if split else "qkv", mode)] = (vil_case(split, dt, grad), False)
                    if grad:  # head_dim 16: "gemm" and "chunk_gemm"
                        out["vil_block C=48 %s %s" % ("query|kv chunked" if split else "qkv", mode)] = (vil_case(split, dt, grad, C=48), False)
                if dt == torch.bfloat16:
                    out["vil_block query|kv chunk_fused %s" % mode] = (vil_case(True, dt, grad, fused=True), False)
    for L in (1, 2, 3, 4):
        for bn in (False, True):
            for stats in (False, True):
                out["dino_head L=%d%s%s grad" % (L, " bn" if bn else "", " stats" if stats else "")] = (head_case(L, bn, stats), False)
    return out


def record(name, mp=None):
    """-> (trace, Session) of one case, on esvit_amd.functional as it stands"""
    import esvit_amd.functional as Fn
    run, wide = cases()[name]
    own = mp is None
    mp = pytest.MonkeyPatch() if own else mp
    try:
        s = Session(mp, Fn, wide, _route(name))
        run(Fn)
        return list(s.rec.trace), s
    finally:
        ops_ref.set_act_dtype(torch.float32)
        if own:
            mp.undo()


def generate():
    return {name: [entry for entry, _ in record(name)[0]] for name in cases()}


def _is_bn_head(name):
    """a head that has BatchNorm layers (one Linear has none, whatever use_bn says)"""
    return name.startswith("dino_head") and " bn" in name and "L=1" not in name


# ---- 1: the same kernels on the same shapes in the same order -----------------------------------------------------------------------------
def golden(_cache={}):
    if not _cache:
        with open(GOLDEN) as f:
            _cache.update(json.load(f))
    return _cache


def test_golden_covers_every_case():
    assert sorted(golden()) == sorted(cases())


@pytest.mark.parametrize("name", sorted(cases()))
def test_launch_sequence_matches_the_golden(name, cpu_ops, monkeypatch):  # noqa: F811
    trace, _ = record(name, monkeypatch)
    got, want = [entry for entry, _ in trace], golden()[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "launch %d of %r" % (i, name)
    assert len(got) == len(want), (name, got[len(want):], want[len(got):])


# ---- 2: weight gradients on the side stream, one join per node ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in cases() if n.endswith(" grad") and not _is_bn_head(n)))
def test_weight_gradients_run_on_the_side_stream_and_are_joined(name, cpu_ops, monkeypatch):  # noqa: F811
    trace, s = record(name, monkeypatch)
    leaves = [(entry, side) for entry, side in trace if entry.startswith(("linear_wgrad(", "ln_fold_finish("))]
    assert leaves, name
    inline = [entry for entry, side in leaves if not side]
    assert not inline, (name, inline)
    assert not s.unjoined, (name, s.unjoined)


# ---- 3: every parameter gradient goes into its bucket slot -----------------------------------------------------------------------------------
ONE_CALL = {  # one contribution per parameter: the ragged Functions over two groups, the per-group ones over ONE group
    "swin_block_multi fp32": swin_case(True, 96, 3, torch.float32, True, True),
    "swin_block_multi bf16 fused": swin_case(True, 96, 3, torch.bfloat16, True, True),
    "swin_block_multi bf16 wide": swin_case(True, WIDE_C, 12, torch.bfloat16, True, True),
    "swin_block fp32": swin_case(False, 96, 3, torch.float32, True, True, SWIN_GROUPS[:1]),
    "swin_block bf16 fused": swin_case(False, 96, 3, torch.bfloat16, True, True, SWIN_GROUPS[:1]),
    "swin_block bf16 wide": swin_case(False, WIDE_C, 12, torch.bfloat16, True, True, SWIN_GROUPS[:1]),
    "vit_block_multi": vit_case(True, torch.bfloat16, True),
    "vit_block": vit_case(False, torch.bfloat16, True, VIT_GROUPS[:1]),
    "vil_block qkv": vil_case(False, torch.bfloat16, True),
    "vil_block query|kv": vil_case(True, torch.bfloat16, True),
    "vit_block_multi gemm": vit_case(True, torch.bfloat16, True, C=48),
    "vit_block gemm": vit_case(False, torch.bfloat16, True, VIT_GROUPS[:1], C=48),
    "vit_block_multi window+gemm": vit_case(True, torch.bfloat16, True, VIT_LONG_GROUPS, C=96),
    "vit_block_multi window+flash": vit_case(True, torch.bfloat16, True, VIT_LONG_GROUPS, C=96),
    "vit_block flash": vit_case(False, torch.bfloat16, True, VIT_LONG_GROUPS[1:], C=96),
    "vit_block_multi window lse": vit_case(True, torch.bfloat16, True, VIT_LSE_GROUPS, C=96),
    "vit_block window lse": vit_case(False, torch.bfloat16, True, VIT_LSE_GROUPS[1:], C=96),
    "vil_block gemm qkv": vil_case(False, torch.bfloat16, True, C=48),
    "vil_block chunk_gemm query|kv": vil_case(True, torch.bfloat16, True, C=48),
    "vil_block query|kv chunk_fused": vil_case(True, torch.bfloat16, True, fused=True),
    "CvtFfnMultiFn": cvt_ffn_case(True, torch.bfloat16, True),
    "CvtFfnFn": cvt_ffn_case(False, torch.bfloat16, True, CVT_GROUPS[:1]),
    "dino_head L=1": head_case(1, False, False), "dino_head L=2": head_case(2, False, True), "dino_head L=3": head_case(3, False, False),
    "dino_head L=4": head_case(4, False, True),
}


@pytest.mark.parametrize("name", sorted(ONE_CALL))
def test_every_gradient_is_written_into_its_bucket_slot(name, cpu_ops, monkeypatch):  # noqa: F811
    """with a gradient sink armed every weight, bias and LayerNorm parameter of a block, and every weight and bias of the plain head,
    is handed its slot exactly once per backward, and the gradient autograd stores is a fresh alias of the slot"""
    import esvit_amd.functional as Fn
    import esvit_amd.params as P
    s = Session(monkeypatch, Fn, "wide" in name, _route(name))
    handed, slots, g0 = {}, {}, P.grad_out

    def counting(p, shape2d=None):
        v = g0(p, shape2d)
        if v is not None:
            handed[id(p)] = handed.get(id(p), 0) + 1
        return v
    monkeypatch.setattr(P, "grad_out", counting)

    def arm(prm):
        slots.update({id(p): torch.full_like(p, float("nan")) for p in prm if p is not None})
        P.set_grad_sink(slots)
    try:
        _, prm = ONE_CALL[name](Fn, arm)
    finally:
        P.set_grad_sink(None)
        ops_ref.set_act_dtype(torch.float32)
        s.reset()
    assert len(prm) >= 4
    for i, p in enumerate(prm):
        if name.startswith("dino_head") and not p.requires_grad:
            continue  # (the frozen weight_g of the last layer)
        assert handed.get(id(p), 0) == 1, (name, i, tuple(p.shape), handed.get(id(p), 0))
        slot = slots[id(p)]
        assert p.grad is not slot and p.grad.data_ptr() == slot.data_ptr(), (name, i, tuple(p.shape))
        assert not torch.isnan(slot).any(), (name, i)


# ---- the plain head's inference pass keeps nothing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_plain_head_without_grad_writes_no_preactivations(L, cpu_ops, monkeypatch):  # noqa: F811
    import esvit_amd.functional as Fn
    s = Session(monkeypatch, Fn)
    try:
        head_case(L, False, False, grad=False)(Fn)
    finally:
        ops_ref.set_act_dtype(torch.float32)
    entries = [entry for entry, _ in s.rec.trace]
    s.reset()
    assert sum(e.startswith("linear_fwd(") for e in entries) == L + 1
    assert not any("want_preact" in e for e in entries), entries


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(generate(), f, indent=0, sort_keys=True)
        f.write("\n")
