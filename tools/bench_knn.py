"""eval_knn.py consumer on one MI355X: features/s of extract_features (Swin-T backbone, 224^2, eval mode) and the k-NN scoring
rate (test rows/s against N_train stored features), then the A/B of the two k-NN routes: the dense "gemm" route
called once per k against ONE knn_classifier_multi call on the fused top-k kernel, and the two routes at a single k -- alternated
over ROUNDS rounds, warm-up excluded.  usage: bench_knn.py [N_train] [N_test] [C] [ROUNDS] [--profile]
--profile: only a warm-up and one fused four-k call, for `rocprofv3 --kernel-trace --stats -- python tools/bench_knn.py --profile`
(knn_scan_kernel = phase 1, knn_merge_kernel = phase 2, everything else of the second call = the vote)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import esvit_amd
from esvit_amd import config as CFG
from esvit_amd import eval as E

profile = "--profile" in sys.argv
sys.argv = [a for a in sys.argv if a != "--profile"]
dev = torch.device("cuda:0")
ntr = int(sys.argv[1]) if len(sys.argv) > 1 else 320000
nte = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
C = int(sys.argv[3]) if len(sys.argv) > 3 else 768
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
esvit_amd.set_precision("bf16")
if not profile:
    model = esvit_amd.build_model(CFG.swin_config("swin_tiny_w7", DROP_PATH_RATE=0.0), is_teacher=True).to(dev).eval()
    x = torch.randn(256, 3, 224, 224, device=dev)
    with torch.no_grad():
        for _ in range(2):
            model(x)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(5):
            f = model(x)
        torch.cuda.synchronize()
        dt = (time.time() - t0) / 5
    print("extract_features: %.0f images/s (Swin-T, 224^2, batch 256, bf16)" % (256 / dt))
g = torch.Generator(device=dev).manual_seed(0)
xtr = torch.nn.functional.normalize(torch.randn(ntr, C, device=dev, generator=g), dim=1)
xte = torch.nn.functional.normalize(torch.randn(nte, C, device=dev, generator=g), dim=1)
ytr = torch.randint(0, 1000, (ntr,), device=dev, generator=g)
yte = torch.randint(0, 1000, (nte,), device=dev, generator=g)
if not profile:
    E.knn_classifier(xtr, ytr, xte[:200], yte[:200], 20, 0.07, num_chunks=2)
    torch.cuda.synchronize()
    t0 = time.time()
    E.knn_classifier(xtr, ytr, xte, yte, 20, 0.07)
    torch.cuda.synchronize()
    dt = time.time() - t0
    print("knn_classifier: %d test x %d train x %d: %.2f s, %.0f test rows/s, similarity %.1f TFLOP/s fp32-equivalent of wall" %
          (nte, ntr, C, dt, nte / dt, 2.0 * nte * ntr * C / dt / 1e12))


# ---- the two routes, alternated ---------------------------------------------------------------------------------------
KS = (10, 20, 100, 200)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    return time.time() - t0, out


def gemm_route(ks):
    E.KNN_ROUTE = "gemm"
    return {k: E.knn_classifier(xtr, ytr, xte, yte, k, 0.07) for k in ks}


def fused_route(ks):
    return E.knn_classifier_multi(xtr, ytr, xte, yte, ks, 0.07)


def topk_only():
    return esvit_amd.ops.knn_topk(xte, xtr, max(KS))


def spread(ts):
    return "median %.4f s  min %.4f  max %.4f" % (sorted(ts)[len(ts) // 2], min(ts), max(ts))


fused_route(KS if profile else (20,))  # warm-up of the fused route (the gemm route ran above)
if profile:
    dt, _ = timed(lambda: fused_route(KS))
    print("fused, one call for the four k: %.4f s" % dt)
    sys.exit(0)
legs = {"gemm x4 (k = 10, 20, 100, 200, one call each)": lambda: gemm_route(KS), "fused, one call for the four k": lambda: fused_route(KS),
        "gemm, k = 20": lambda: gemm_route((20,)), "fused, k = 20": lambda: fused_route((20,)), "knn_topk alone, k = 200": topk_only}
times = {name: [] for name in legs}
result = {}
for _ in range(rounds):
    for name, fn in legs.items():  # alternated: every round runs every leg once
        dt, result[name] = timed(fn)
        times[name].append(dt)
print("k-NN routes, %d test x %d train x %d, %d alternated rounds" % (nte, ntr, C, rounds))
for name, ts in times.items():
    print("  %-48s %s" % (name, spread(ts)))
med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
flop = 2.0 * nte * ntr * C
print("  four k: fused / gemm = %.3f (acceptance: <= 0.5)" % (med["fused, one call for the four k"] / med["gemm x4 (k = 10, 20, 100, 200, one call each)"]))
print("  one k:  fused / gemm = %.3f" % (med["fused, k = 20"] / med["gemm, k = 20"]))
print("  fused pass (scan + merge, k = 200): %.1f TFLOP/s fp32 of wall against the 155 TFLOP/s of v_mfma_f32_16x16x4_f32; gemm route at k = 20: %.1f" %
      (flop / med["knn_topk alone, k = 200"] / 1e12, flop / med["gemm, k = 20"] / 1e12))
a, b = result["gemm x4 (k = 10, 20, 100, 200, one call each)"], result["fused, one call for the four k"]
print("  top-1 / top-5 per k, gemm | fused: " + "; ".join("k=%d %.2f/%.2f | %.2f/%.2f" % (k, a[k][0], a[k][1], b[k][0], b[k][1]) for k in KS))
