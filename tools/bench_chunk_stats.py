"""Sliding-chunk attention statistics micro-benchmark: the statistics mode of the fused per-chunk kernels (csrc/chunk_attn.hip,
ops.chunk_attn_stats: entropy of every row, and the same with five listed rows) against the fused forward of the same shape
(ops.sliding_chunk_attn_fwd, which does strictly more: V staging, the second MFMA, the out store) and against the fall-back
(functional.vil_attention_stats without the kernels: P of the dense route for a slice of the batch at a time, reduced in torch), at the
stage shapes of one Vision Longformer pre-training step and at vil_small's first stage at 448^2 (run on the MI355X).

    python tools/bench_chunk_stats.py [--batch 64] [--rounds 3] [--out FILE]   (default: profiles/chunk_stats_bench.json)

Per shape: microseconds per call of every arm -- device events around at least 0.5 s of work after a warm-up, the arms alternated in
this one process for `rounds` rounds, median and range over the rounds (the same-arm spread) -- and torch.cuda.max_memory_allocated of
one call above the live inputs.  Inputs are random."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import esvit_amd.functional as Fn
from esvit_amd import ops

dev = torch.device("cuda:0")
W = 7
WINDOW_MS = 500.0


def table(nglo, nx, ny):
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return torch.from_numpy(np.concatenate([np.full(nglo, -1), ((ix // W) << 16 | (iy // W)).reshape(-1)]).astype(np.int32)).to(dev)


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # milliseconds per call


def peak_of(fn):
    fn()  # (warm-up: code objects loaded, the shared scratch sized)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


class _NoKernels:
    """the ops module without the statistics entry: functional.vil_attention_stats takes its fall-back"""

    def __getattr__(self, name):
        if name.startswith("chunk_attn_stats"):
            raise AttributeError(name)
        return getattr(ops, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64, help="images per step: 2 x batch 224^2 crops, 8 x batch 96^2 crops")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "chunk_stats_bench.json"))
    a = ap.parse_args()
    B = a.batch
    shapes = [("vil_tiny s1 224", 56, 48, 1, 2 * B), ("vil_tiny s2 224", 28, 32, 3, 2 * B), ("vil_tiny s1 96", 24, 48, 1, 8 * B),
              ("vil_tiny s2 96", 12, 32, 3, 8 * B), ("vil_small s1 224", 56, 32, 3, 2 * B), ("vil_small s2 224", 28, 64, 3, 2 * B),
              ("vil_small s1 448", 112, 32, 3, 2)]
    ops.workspace(1, dev, slot=3)
    fallback_ops = _NoKernels()
    recs = []
    for name, side, hd, nH, nimg in shapes:
        nglo = 1
        N = nglo + side * side
        lay = (table(nglo, side, side), nglo, W * side, W)
        qkv = torch.randn(nimg * N, 3 * nH * hd, generator=torch.Generator().manual_seed(0)).to(dev).to(torch.bfloat16)
        queries = [0, nglo, N - 1, nglo + (W - 1) * side + W, nglo + (W + 3) * side + W + 2]
        scale = hd ** -0.5
        arms = {
            "stats": lambda: ops.chunk_attn_stats(qkv, nimg, N, nH, scale, lay),
            "stats_rows5": lambda: ops.chunk_attn_stats(qkv, nimg, N, nH, scale, lay, queries=queries),
            "fused_fwd": lambda: ops.sliding_chunk_attn_fwd(qkv, nimg, N, nH, scale, lay[:3]),
            "fallback": lambda: Fn.vil_attention_stats(fallback_ops, qkv, nimg, N, nH, scale, lay),
        }
        peaks = {k: peak_of(fn) for k, fn in arms.items()}
        iters = {k: max(1, int(WINDOW_MS / max(window(fn, 2), 1e-3)) + 1) for k, fn in arms.items()}  # (a second warm-up; sizes the window)
        times = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():  # alternated: every round visits every arm
                times[k].append(window(fn, iters[k]) * 1e3)
        e_k, _ = arms["stats"]()
        e_f, _ = arms["fallback"]()
        rec = dict(shape=name, grid=side, hd=hd, nH=nH, images=nimg, tokens=N, rounds=a.rounds, max_abs_entropy_diff_vs_fallback=round((e_k - e_f).abs().max().item(), 5))
        for k in arms:
            rec[k + "_us"] = round(statistics.median(times[k]), 1)
            rec[k + "_us_range"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
            rec[k + "_iters"] = iters[k]
            rec[k + "_peak_MB"] = round(peaks[k] / 1e6, 1)
        rec["stats_over_fused_fwd"] = round(rec["stats_us"] / rec["fused_fwd_us"], 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del qkv, e_k, e_f
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(recs, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
