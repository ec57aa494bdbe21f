"""-m "not gpu": the global (flash attention) mode of esvit_window_attn_fwd / _bwd without a GPU -- the argument checks of the C entry,
its constants and scratch size, the routing switch of functional.vit_attention and its fall-back on an ops module without the entry."""
import ctypes as C
import importlib
import importlib.util
import os

import pytest
import torch

from oracle import ops_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mode_is_refused_where_it_must_be(lib_built):
    """fp32, head_dim 40 / 48, L = 0, a NULL lse, both mode flags: ESVIT_ERR_ARG before any launch (a launch on this GPU-less host would
    come back as ESVIT_ERR_HIP), and the message names the cause"""
    from esvit_amd import _lib, ops
    lib = _lib.lib
    fake = C.c_void_p(0x1000)  # never dereferenced: the argument checks come first

    def fwd(dtype=ops.BF16, hd=64, L=785, lse=fake, ws=ops.ATTN_GLOBAL):
        return lib.esvit_window_attn_fwd(dtype, fake, None, None, L, None, ws, None, None, 1, 2, L, 3, hd, 0.125, fake, lse, None, None)

    def bwd(dtype=ops.BF16, hd=64, L=785, lse=fake, ws=ops.ATTN_GLOBAL):
        return lib.esvit_window_attn_bwd(dtype, fake, None, None, L, fake, fake, lse, None, ws, fake, None, 1, 2, L, 3, hd, 0.125, fake,
                                         None, None, None)
    for f in (fwd, bwd):
        assert f(dtype=ops.F32) == -1 and b"bf16" in lib.esvit_last_error()
        assert f(hd=40) == -1 and b"head_dim 40" in lib.esvit_last_error()
        assert f(hd=48) == -1 and b"head_dim 48" in lib.esvit_last_error()
        assert f(L=0) == -1 and b"L=0" in lib.esvit_last_error()
        assert f(lse=None) == -1 and b"lse" in lib.esvit_last_error()
        assert f(ws=ops.ATTN_GLOBAL | ops.ATTN_SLIDING_CHUNK) == -1 and b"both mode flags" in lib.esvit_last_error()
        assert f(ws=ops.ATTN_GLOBAL | ops.ATTN_SLIDING_CHUNK | 7) == -1 and b"both mode flags" in lib.esvit_last_error()
    assert ops.global_attn_supported(torch.bfloat16, 32) and ops.global_attn_supported(torch.bfloat16, 64)
    assert not ops.global_attn_supported(torch.float32, 64) and not ops.global_attn_supported(torch.bfloat16, 48)
    assert "global_attn_fwd" not in _lib.SIGNATURES and not any("flash" in s or "global" in s for s in _lib.SIGNATURES)


def test_constants_and_scratch(lib_built):
    from esvit_amd import ops
    hdr = open(os.path.join(ROOT, "include", "esvit_hip.h")).read()
    assert "#define ESVIT_ATTN_GLOBAL 0x%x" % ops.ATTN_GLOBAL in hdr
    assert "#define ESVIT_Q_GLOBAL_ATTN_WS %d\n" % ops.Q_GLOBAL_ATTN_WS in hdr
    assert ops.ATTN_GLOBAL & ops.ATTN_SLIDING_CHUNK == 0 and 0 < ops.ATTN_GLOBAL < 2 ** 31
    a, b = ops.query(ops.Q_GLOBAL_ATTN_WS, 6, 785, 1), ops.query(ops.Q_GLOBAL_ATTN_WS, 6, 3140, 1)
    assert 0 < a < b < 4.5 * a, (a, b)           # linear in the tokens
    assert a >= 6 * 785                          # delta: one float per (image, head, token)
    assert ops.query(ops.Q_GLOBAL_ATTN_WS, 6, 785, 0) >= 0


def test_routing_switch(monkeypatch):
    import esvit_amd.functional as Fn
    assert Fn.VIT_LONG_ATTENTION == os.environ.get("ESVIT_VIT_LONG_ATTN", "gemm")
    # a bad value raises at import: a second, private copy of the module is executed (the imported one stays as it is)
    for value, ok in (("fast", False), ("flash", True)):
        monkeypatch.setenv("ESVIT_VIT_LONG_ATTN", value)
        spec = importlib.util.spec_from_file_location("esvit_amd._functional_copy", Fn.__file__)
        copy = importlib.util.module_from_spec(spec)
        if ok:
            spec.loader.exec_module(copy)
            assert copy.VIT_LONG_ATTENTION == "flash"
        else:
            with pytest.raises(ValueError, match="ESVIT_VIT_LONG_ATTN"):
                spec.loader.exec_module(copy)
    monkeypatch.undo()
    assert Fn.VIT_LONG_ATTENTION == os.environ.get("ESVIT_VIT_LONG_ATTN", "gemm")


def test_ops_module_without_the_entry_keeps_the_gemm_route(monkeypatch):
    """the CPU restatement has no global_attn_fwd: under "flash" vit_attention still returns the batched-GEMM route's 2-tuple, and
    vit_attention_bwd takes it"""
    import esvit_amd.functional as Fn
    monkeypatch.setattr(Fn, "VIT_LONG_ATTENTION", "flash")
    assert not hasattr(ops_ref, "global_attn_fwd")
    B, N, nH, hd = 2, 230, 2, 32
    Cc = nH * hd
    g = torch.Generator().manual_seed(5)
    qkv, dout = torch.randn(B * N, 3 * Cc, generator=g), torch.randn(B * N, Cc, generator=g)
    ops_ref.set_act_dtype(torch.float32)
    ao, att = Fn.vit_attention(ops_ref, qkv, torch.zeros(3 * Cc), B, N, nH, hd ** -0.5, True)
    assert att.route == "gemm" and ao.shape == (B * N, Cc)
    want, saved = ops_ref.vit_attn_fwd(qkv, B, N, nH, hd ** -0.5)
    assert torch.equal(ao, want)
    d = Fn.vit_attention_bwd(ops_ref, dout, att, torch.zeros(3 * Cc), B, N, nH, hd ** -0.5)
    assert torch.equal(d, ops_ref.vit_attn_bwd(dout, saved, B, N, nH, hd ** -0.5))
