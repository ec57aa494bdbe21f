"""-m "not gpu": the fused sliding-chunk attention without a GPU -- the slot -> token arithmetic of the kernels (csrc/chunk_geom.h compiled
for the host) against the mask of the dense route, a per-chunk torch restatement of the algorithm the kernels implement (forward with
the log-sum-exp, backward with delta) against oracle/ops_ref.vit_attn_fwd / _bwd, the save / restore plumbing of vil_block on that
restatement against the reference's fixture, and the argument checks of the C entry."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import ops_ref
from tests.test_composition_cpu import cpu_ops  # noqa: F401  (fixture: the host code on oracle.ops_ref in fp32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 7
GRIDS = [(5, 5), (7, 7), (8, 15), (12, 12), (24, 24), (28, 28), (21, 35), (56, 56)]


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("chunkgeom") / "chunk_geom_host.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-I", os.path.join(ROOT, "esvit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "chunk_geom_host.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def _table(nglo, nx, ny, w=W):
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return torch.from_numpy(np.concatenate([np.full(nglo, -1), ((ix // w) << 16 | (iy // w)).reshape(-1)]).astype(np.int32))


def _units(geom, nglo, nx, ny, w=W):
    """-> [(own tokens, neighbourhood tokens)] of every chunk, live slots only, in slot order"""
    ncx, ncy = C.c_int(0), C.c_int(0)
    n = geom.cg_t_chunks(nglo, nx, ny, w, C.byref(ncx), C.byref(ncy))
    assert n == ncx.value * ncy.value == -(-nx // w) * -(-ny // w)
    own = np.empty(geom.cg_t_own_slots(), np.int32)
    nb = np.empty(geom.cg_t_nb_slots(), np.int32)
    out = []
    for cr in range(ncx.value):
        for cc in range(ncy.value):
            geom.cg_t_maps(nglo, nx, ny, w, cr, cc, own.ctypes.data_as(C.c_void_p), nb.ctypes.data_as(C.c_void_p))
            out.append((own[own >= 0].copy(), nb[nb >= 0].copy()))
    return out


@pytest.mark.parametrize("nglo", [1, 2])
@pytest.mark.parametrize("grid", GRIDS)
def test_slot_maps_equal_the_chunk_mask(geom, grid, nglo):
    """the live neighbourhood slots of every chunk are exactly the row of ops_ref.chunk_mask of each of its queries; every local token
    is an own slot of exactly one chunk; 64 own and 448 neighbourhood slots suffice"""
    nx, ny = grid
    N = nglo + nx * ny
    assert (geom.cg_t_own_slots(), geom.cg_t_nb_slots(), geom.cg_t_max_nglo()) == (64, 448, 7)
    assert geom.cg_t_supported(nglo, nx, ny, W) == 1
    mask = ops_ref.chunk_mask(_table(nglo, nx, ny)).numpy()
    seen = np.zeros(N, np.int64)
    for own, nb in _units(geom, nglo, nx, ny):
        assert 0 < len(own) <= 49 and len(nb) <= nglo + 441
        assert len(set(nb.tolist())) == len(nb) and (own >= nglo).all()
        row = np.zeros(N, bool)
        row[nb] = True
        assert (mask[own] == row[None, :]).all()
        seen[own] += 1
    assert (seen[:nglo] == 0).all() and (seen[nglo:] == 1).all()


def test_geometry_limits(geom):
    assert geom.cg_t_supported(7, 56, 56, 7) == 1 and geom.cg_t_supported(8, 56, 56, 7) == 0
    assert geom.cg_t_supported(1, 56, 56, 8) == 0 and geom.cg_t_supported(1, 0, 56, 7) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the algorithm of csrc/chunk_attn.hip restated per chunk in torch (fp32): same units of work, same saved tensors
# ---------------------------------------------------------------------------------------------------------------------
def make_restatement(geom, calls=None):
    RANGE = 512

    def grid_of(chunk, N):
        tab, nglo, rowtok = chunk[:3]
        ny = rowtok // W
        nx = (N - nglo) // ny
        assert rowtok == W * ny and nglo + nx * ny == N
        return nglo, nx, ny

    def fwd(qkv, B, N, nH, scale, chunk):
        if calls is not None:
            calls["fwd"] += 1
        nglo, nx, ny = grid_of(chunk, N)
        q, k, v = ops_ref._vit_heads(qkv, B, N, nH, 3)
        o = torch.zeros_like(q)
        lse = torch.zeros(q.shape[:3])
        for own, nb in _units(geom, nglo, nx, ny):  # local queries: one unit per chunk
            s = scale * q[:, :, own] @ k[:, :, nb].transpose(-2, -1)
            l = torch.logsumexp(s, -1)
            o[:, :, own] = torch.exp(s - l[..., None]) @ v[:, :, nb]
            lse[:, :, own] = l
        if nglo:  # global queries: streaming over key ranges, online max / sum
            m = torch.full(q.shape[:2] + (nglo,), -float("inf"))
            den = torch.zeros_like(m)
            num = torch.zeros(q.shape[:2] + (nglo, q.shape[-1]))
            for t0 in range(0, N, RANGE):
                s = scale * q[:, :, :nglo] @ k[:, :, t0:t0 + RANGE].transpose(-2, -1)
                m2 = torch.maximum(m, s.amax(-1))
                e = torch.exp(s - m2[..., None])
                den = den * torch.exp(m - m2) + e.sum(-1)
                num = num * torch.exp(m - m2)[..., None] + e @ v[:, :, t0:t0 + RANGE]
                m = m2
            o[:, :, :nglo] = num / den[..., None]
            lse[:, :, :nglo] = m + den.log()
        out = o.transpose(1, 2).reshape(B * N, -1).to(qkv.dtype).contiguous()
        return out, (qkv, out, lse)

    def bwd(dout, saved, B, N, nH, scale, chunk):
        if calls is not None:
            calls["bwd"] += 1
        qkv, out, lse = saved
        nglo, nx, ny = grid_of(chunk, N)
        q, k, v = ops_ref._vit_heads(qkv, B, N, nH, 3)
        do = ops_ref._vit_heads(dout, B, N, nH, 1)[0]
        o = ops_ref._vit_heads(out, B, N, nH, 1)[0]
        delta = (do * o).sum(-1)
        dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
        for own, nb in _units(geom, nglo, nx, ny):
            # dQ of the chunk's queries from its key neighbourhood
            p = torch.exp(scale * q[:, :, own] @ k[:, :, nb].transpose(-2, -1) - lse[:, :, own, None])
            ds = p * (do[:, :, own] @ v[:, :, nb].transpose(-2, -1) - delta[:, :, own, None])
            dq[:, :, own] = scale * ds @ k[:, :, nb]
            # dK, dV of the chunk's keys from [global queries | the queries of its neighbourhood]
            p = torch.exp(scale * q[:, :, nb] @ k[:, :, own].transpose(-2, -1) - lse[:, :, nb, None])
            dv[:, :, own] = p.transpose(-2, -1) @ do[:, :, nb]
            ds = p * (do[:, :, nb] @ v[:, :, own].transpose(-2, -1) - delta[:, :, nb, None])
            dk[:, :, own] = scale * ds.transpose(-2, -1) @ q[:, :, nb]
        for t0 in range(0, N, RANGE):  # the global tokens, per range
            r = slice(t0, t0 + RANGE)
            p = torch.exp(scale * q[:, :, r] @ k[:, :, :nglo].transpose(-2, -1) - lse[:, :, r, None])   # range as queries of the global keys
            dv[:, :, :nglo] += p.transpose(-2, -1) @ do[:, :, r]
            ds = p * (do[:, :, r] @ v[:, :, :nglo].transpose(-2, -1) - delta[:, :, r, None])
            dk[:, :, :nglo] += scale * ds.transpose(-2, -1) @ q[:, :, r]
            p = torch.exp(scale * q[:, :, :nglo] @ k[:, :, r].transpose(-2, -1) - lse[:, :, :nglo, None])  # range as keys of the global queries
            ds = p * (do[:, :, :nglo] @ v[:, :, r].transpose(-2, -1) - delta[:, :, :nglo, None])
            dq[:, :, :nglo] += scale * ds @ k[:, :, r]
        C_ = dout.shape[1]
        return torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * C_).to(dout.dtype).contiguous()

    return fwd, bwd


def _close(name, got, ref, tol):
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e (rel %.3e > tol %.1e)" % (name, err, scale, err / scale, tol)


@pytest.mark.parametrize("grid,nglo,hd", [((28, 28), 1, 48), ((24, 24), 1, 48), ((12, 12), 1, 32), ((5, 5), 1, 32), ((7, 7), 1, 32), ((8, 15), 1, 32),
                                          ((21, 35), 2, 64), ((56, 56), 1, 32)])
def test_per_chunk_restatement_equals_dense_route(geom, grid, nglo, hd):
    """fp32, at the fp32 tolerances of tests/test_kernels_gpu.py::test_sliding_chunk_attention (2e-5 forward, 5e-5 backward)"""
    nx, ny = grid
    N = nglo + nx * ny
    B, nH = (1, 1) if N > 2000 else (2, 2)
    g = torch.Generator().manual_seed(90)
    qkv = torch.randn(B * N, 3 * nH * hd, generator=g)
    dout = torch.randn(B * N, nH * hd, generator=g)
    tab = _table(nglo, nx, ny)
    lay = (tab, nglo, W * ny)
    scale = hd ** -0.5
    fwd, bwd = make_restatement(geom)
    out, saved = fwd(qkv, B, N, nH, scale, lay)
    outr, savedr = ops_ref.vit_attn_fwd(qkv, B, N, nH, scale, chunk=lay)
    _close("out", out, outr, 2e-5)
    _close("dqkv", bwd(dout, saved, B, N, nH, scale, lay), ops_ref.vit_attn_bwd(dout, savedr, B, N, nH, scale, chunk=lay), 5e-5)


def test_vil_block_plumbing_on_the_restatement(cpu_ops, geom, monkeypatch):  # noqa: F811
    """CHUNK_ATTENTION = "fused" with the per-chunk restatement in the place of the kernels: the save / restore of (qkv, lse) in
    the block body (functional.VitBodyFn) reproduces the reference's fixture within the bounds of test_vil_full_width_composition_matches_reference_golden"""
    from esvit_amd.models import vision_longformer as vil
    from tests.test_step_gpu import check_full_vil_case
    calls = {"fwd": 0, "bwd": 0, "sup": 0}
    fwd, bwd = make_restatement(geom, calls)

    def supported(dtype, hd, w, nglo):
        calls["sup"] += 1
        return dtype == torch.float32 and w == W and nglo <= 7

    monkeypatch.setattr(cpu_ops, "sliding_chunk_attn_fwd", fwd, raising=False)
    monkeypatch.setattr(cpu_ops, "sliding_chunk_attn_bwd", bwd, raising=False)
    monkeypatch.setattr(cpu_ops, "sliding_chunk_attn_supported", supported, raising=False)
    monkeypatch.setattr(vil, "CHUNK_ATTENTION", "fused")
    check_full_vil_case("vil_tiny_k8192_b2", torch.device("cpu"), True, (1e-4, 1e-4, 2e-3, 5e-3))
    assert calls["fwd"] > 0 and calls["bwd"] > 0 and calls["sup"] > 0, calls
    assert calls["bwd"] <= calls["fwd"]


def test_default_route_is_dense():
    from esvit_amd.models import vision_longformer as vil
    assert vil.CHUNK_ATTENTION == os.environ.get("ESVIT_VIL_CHUNK_ATTN", "dense")


def test_mode_is_refused_where_it_must_be(lib_built):
    """fp32, head_dim 40, eight global tokens, another chunk side: ESVIT_ERR_ARG before any launch (a launch on this GPU-less host
    would come back as ESVIT_ERR_HIP); and the library exports exactly what the header declares -- the mode added no symbol"""
    from esvit_amd import _lib, ops
    lib = _lib.lib
    fake = C.c_void_p(0x1000)  # never dereferenced: the argument checks come first
    nx = ny = 14

    def fwd(dtype, hd, nglo, w=7):
        L = nglo + nx * ny
        return lib.esvit_window_attn_fwd(dtype, fake, None, fake, L, None, w | ops.ATTN_SLIDING_CHUNK, fake, None, nx, 2, ny, 2, hd, 0.125, fake, fake, None, None)

    def bwd(dtype, hd, nglo, w=7):
        L = nglo + nx * ny
        return lib.esvit_window_attn_bwd(dtype, fake, None, fake, L, fake, fake, fake, None, w | ops.ATTN_SLIDING_CHUNK, fake, None, nx, 2, ny, 2, hd, 0.125, fake,
                                         None, None, None)
    for f in (fwd, bwd):
        assert f(ops.F32, 32, 1) == -1 and b"bf16" in lib.esvit_last_error()
        assert f(ops.BF16, 40, 1) == -1 and b"head_dim 40" in lib.esvit_last_error()
        assert f(ops.BF16, 32, 8) == -1 and b"global tokens" in lib.esvit_last_error()
        assert f(ops.BF16, 32, 1, w=8) == -1 and b"chunk side" in lib.esvit_last_error()
    assert not ops.sliding_chunk_attn_supported(torch.float32, 32, 7, 1) and not ops.sliding_chunk_attn_supported(torch.bfloat16, 40, 7, 1)
    assert not ops.sliding_chunk_attn_supported(torch.bfloat16, 32, 7, 8) and not ops.sliding_chunk_attn_supported(torch.bfloat16, 32, 14, 1)
    assert all(ops.sliding_chunk_attn_supported(torch.bfloat16, hd, 7, g) for hd in (32, 48, 64) for g in (0, 1, 7))
    # scratch sizes of the mode: linear in the tokens
    a, b = ops.query(ops.Q_CHUNK_ATTN_WS, 6, 3137, 1), ops.query(ops.Q_CHUNK_ATTN_WS, 6, 12545, 1)
    assert 0 < a < b < 4.5 * a and ops.query(ops.Q_CHUNK_ATTN_WS, 6, 3137, 0) > 0
    hdr = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "ESVIT_ATTN_SLIDING_CHUNK 0x%x" % ops.ATTN_SLIDING_CHUNK in hdr and "ESVIT_Q_CHUNK_ATTN_WS %d" % ops.Q_CHUNK_ATTN_WS in hdr
    declared = set(re.findall(r"\b(esvit_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert len(declared) == 60 and declared == set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {s for s in exported if s.startswith("esvit_")} == declared, sorted(exported ^ declared)
