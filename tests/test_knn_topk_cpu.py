"""Fused k-NN scoring, the parts that need no GPU: the host branch of esvit_amd.eval.knn_classifier_multi / knn_topk_streamed
against the reference's golden numbers, the oracle and tests/knn_ref.py; the layout of the descriptor's new field; the workspace
question and the argument checks of the library (cross-compiled, nothing launched)."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from oracle import esvit_oracle as O
from tests import golden_utils as GU
from tests import knn_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KS = (10, 20, 100, 200)


def test_multi_on_host_equals_reference_golden(lib_built):
    from esvit_amd import eval as E
    gold = torch.load(os.path.join(GOLD, "knn.pt"), weights_only=False)
    for c, want in zip(GU.KNN_CASES, gold["top"]):
        xtr, ytr, xte, yte = GU.make_knn_set(c["seed"], noise=c["noise"])
        got = E.knn_classifier_multi(xtr, ytr, xte, yte, (c["k"],), c["T"], num_classes=10)[c["k"]]
        assert got == pytest.approx(want, abs=1e-4), (c, got, want)


def test_fused_route_of_knn_classifier_on_host(lib_built, monkeypatch):
    """KNN_ROUTE = "fused" sends knn_classifier through knn_classifier_multi; "gemm" never touches the top-k kernel"""
    from esvit_amd import eval as E
    gold = torch.load(os.path.join(GOLD, "knn.pt"), weights_only=False)
    c, want = GU.KNN_CASES[0], gold["top"][0]
    xtr, ytr, xte, yte = GU.make_knn_set(c["seed"], noise=c["noise"])
    assert E.KNN_ROUTE == os.environ.get("ESVIT_KNN_ROUTE", "gemm")
    monkeypatch.setattr(E, "KNN_ROUTE", "fused")
    assert E.knn_classifier(xtr, ytr, xte, yte, c["k"], c["T"], num_classes=10) == pytest.approx(want, abs=1e-4)
    monkeypatch.setattr(E, "KNN_ROUTE", "nonsense")
    with pytest.raises(ValueError):
        E.knn_classifier(xtr, ytr, xte, yte, c["k"], c["T"], num_classes=10)


def test_multi_on_host_equals_oracle_for_four_k_in_one_call(lib_built):
    from esvit_amd import eval as E
    xtr, ytr, xte, yte = GU.make_knn_set(11, n_train=20000, n_test=3000, dim=384, classes=100, noise=6.0)
    got = E.knn_classifier_multi(xtr, ytr, xte, yte, KS, 0.07, num_classes=100)
    assert sorted(got) == sorted(KS)
    for k in KS:
        want = O.knn_classifier(xtr, ytr, xte, yte, k, 0.07, num_classes=100)
        assert got[k] == pytest.approx(want, abs=1e-4), (k, got[k], want)


def test_vote_equals_the_row_by_row_restatement(lib_built):
    from esvit_amd import eval as E
    xtr, ytr, xte, yte = GU.make_knn_set(3, n_train=700, n_test=90, dim=24, classes=7, noise=3.0)
    got = E.knn_classifier_multi(xtr, ytr, xte, yte, (1, 5, 33), 0.07, num_classes=7, num_chunks=4)
    vals, idx = KR.topk_host(xte, xtr, 33)
    for k in (1, 5, 33):
        assert got[k] == pytest.approx(KR.vote(vals, idx, ytr, yte, k, 0.07, 7), abs=1e-9)


def test_prefix_property(lib_built):
    from esvit_amd import eval as E
    xtr, _, xte, _ = GU.make_knn_set(4, n_train=900, n_test=64, dim=32, classes=5, noise=2.0)
    vmax, imax = E._knn_topk(xte, xtr, 200)
    for k in (1, 10, 20, 100):
        v, i = E._knn_topk(xte, xtr, k)
        assert torch.equal(v, vmax[:, :k]) and torch.equal(i, imax[:, :k])


def test_streaming_equals_one_shot(lib_built):
    from esvit_amd import eval as E
    xtr, _, xte, _ = GU.make_knn_set(8, n_train=1000, n_test=77, dim=40, classes=5, noise=2.0)
    pieces = [xtr[:333], xtr[333:390], xtr[390:]]
    for k in (1, 20, 57):
        vals, idx = E.knn_topk_streamed(xte, pieces, k)
        want_v, want_i = KR.topk_host(xte, xtr, k)
        assert idx.dtype == torch.int32
        assert torch.equal(vals, want_v) and torch.equal(idx, want_i)
    with pytest.raises(ValueError):
        E.knn_topk_streamed(xte, [xtr[:5], xtr[5:]], 20)
    with pytest.raises(ValueError):
        E.knn_classifier_multi(xtr[:15], torch.zeros(15, dtype=torch.long), xte, torch.zeros(77, dtype=torch.long), (20,), 0.07, num_classes=5)


def test_exact_ties_come_back_in_ascending_row_order(lib_built):
    from esvit_amd import eval as E
    xtr, _, xte, _ = GU.make_knn_set(9, n_train=300, n_test=20, dim=16, classes=3, noise=1.0)
    xtr = torch.cat([xtr, xtr[:100], xtr[:50]])  # rows r, 300 + r (and 400 + r for r < 50) are the same vector
    vals, idx = E._knn_topk(xte, xtr, 60)
    ties = 0
    for r in range(vals.shape[0]):
        same = vals[r, 1:] == vals[r, :-1]
        assert bool((idx[r, 1:][same] > idx[r, :-1][same]).all())
        ties += int(same.sum())
    assert ties > 0
    sv, si = E.knn_topk_streamed(xte, [xtr[:120], xtr[120:301], xtr[301:]], 60)
    assert torch.equal(sv, vals) and torch.equal(si, idx)


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "esvit_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(esvit_gemm_desc), offsetof(esvit_gemm_desc, topk), offsetof(esvit_gemm_desc, colstat),
           sizeof(esvit_gemm_topk), offsetof(esvit_gemm_topk, merge), offsetof(esvit_gemm_topk, vals), offsetof(esvit_gemm_topk, idx),
           offsetof(esvit_gemm_topk, idx_base), offsetof(esvit_gemm_topk, workspace), offsetof(esvit_gemm_topk, workspace_bytes));
    return 0;
}
"""


def test_descriptor_layout_matches_the_header(lib_built, tmp_path):
    from esvit_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    D, T = _lib.GemmDesc, _lib.GemmTopk
    assert got == [ctypes.sizeof(D), D.topk.offset, D.colstat.offset, ctypes.sizeof(T), T.merge.offset, T.vals.offset, T.idx.offset, T.idx_base.offset,
                   T.workspace.offset, T.workspace_bytes.offset]
    assert D.topk.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(D)  # the trailing field


def test_workspace_question(lib_built):
    from esvit_amd import ops
    prev = 0
    for M in (1, 128, 129, 400, 2176, 2177, 2304, 3000, 4096, 5000, 50000, 65536, 70000):
        for N, k in ((257, 1), (20000, 200), (300000, 200), (1280000, 256)):
            assert ops.query(ops.Q_TOPK_WS, M, N, k) > 0
        ws = ops.query(ops.Q_TOPK_WS, M, 300000, 200)
        assert ws >= prev, (M, ws, prev)
        prev = ws
    for M in range(1, 9000, 37):  # monotone in M, step by step
        assert ops.query(ops.Q_TOPK_WS, M, 300000, 200) <= ops.query(ops.Q_TOPK_WS, M + 37, 300000, 200)
    # the scratch does not follow the length of the scan once the splits saturate, and is far below the dense block
    assert ops.query(ops.Q_TOPK_WS, 4096, 300000, 200) == ops.query(ops.Q_TOPK_WS, 4096, 1280000, 200)
    assert ops.query(ops.Q_TOPK_WS, 4096, 300000, 200) < 4096 * 300000 * 4 // 10
    for bad_k in (0, 257):
        assert ops.query(ops.Q_TOPK_WS, 4096, 300000, bad_k) < 0


def _desc(k, dtype_ok=True, **over):
    """a descriptor with plausible (never dereferenced) addresses: the checks run before any device call"""
    from esvit_amd import _lib
    t = _lib.GemmTopk(k=k, merge=0, vals=0x1000, idx=0x2000, idx_base=0, workspace=0x4000, workspace_bytes=1 << 40)
    d = _lib.GemmDesc(A=0x10000, B=0x20000, C=None, M=256, N=1024, K=64, lda=64, ldb=64, ldc=1024, batch=1, alpha=1.0)
    for name, v in over.items():
        setattr(t if hasattr(t, name) and name != "k" else d, name, v)
    d.topk = ctypes.pointer(t)
    return d, t


def test_argument_checks_come_before_any_device_call(lib_built):
    from esvit_amd import _lib
    lib = _lib.lib

    def rc_of(dtype, d):
        return lib.esvit_gemm(dtype, ctypes.byref(d), None), lib.esvit_last_error().decode()

    d, t = _desc(20)
    rc, msg = rc_of(_lib.BF16, d)
    assert rc == -1 and "fp32" in msg, (rc, msg)
    for k in (0, 257, -3):
        d, t = _desc(k)
        rc, msg = rc_of(_lib.F32, d)
        assert rc == -1 and "k=" in msg, (k, rc, msg)
    d, t = _desc(200, N=100)  # k > N without a list to merge
    assert rc_of(_lib.F32, d)[0] == -1
    for over in (dict(splitk=2), dict(batch=2), dict(epilogue=_lib.EPI_GELU), dict(bias=0x8000), dict(residual=0x8000), dict(rowmap=0x8000),
                 dict(b_kstrided=1), dict(K=66), dict(workspace_bytes=64), dict(alpha=2.0), dict(kernel=_lib.GEMM_DMA4)):
        d, t = _desc(20, **over)
        rc, msg = rc_of(_lib.F32, d)
        assert rc == -1 and "topk" in msg, (over, rc, msg)
    # esvit_gemm_select reports the tile of the new loop for such a descriptor
    d, t = _desc(20)
    tm, tn, slots = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    kern = lib.esvit_gemm_select(_lib.F32, ctypes.byref(d), ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(slots))
    assert (kern, tm.value, tn.value, slots.value) == (_lib.GEMM_REGSTAGE, 128, 128, 512)
    d.A = d.B = None  # (a pure function of the shape: no buffers needed) ...
    assert lib.esvit_gemm_select(_lib.F32, ctypes.byref(d), None, None, None) == _lib.GEMM_REGSTAGE
    t.k = 300         # ... but the same argument checks
    assert lib.esvit_gemm_select(_lib.F32, ctypes.byref(d), None, None, None) == -1
    # a descriptor without the field is what it was: the dense fp32 GEMM's own checks answer (null C)
    d, t = _desc(20)
    d.topk = None
    rc, msg = rc_of(_lib.F32, d)
    assert rc == -1 and "null operand" in msg and "topk" not in msg
