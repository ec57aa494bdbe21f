"""Attention-entropy benchmark: the entropy of all 12 blocks of deit_small through esvit_amd.analysis.attention_entropy (the statistics
kernels of csrc/flash_attn.hip: no attention matrix exists) against the route it replaces -- forward_selfattention(n=2), which returns
P fp32 [B, nH, N, N] of every block, reduced with torch -- at 197 tokens (224^2 at patch 16) and 785 tokens (224^2 at patch 8), 16 and 64
images per call, bf16 (run on the MI355X).

    python tools/bench_attn_stats.py [--batches 16,64] [--out FILE]   (default: profiles/bench_attn_stats.jsonl)

One JSON line per (tokens, images): time of one call and torch.cuda.max_memory_allocated above what was live before it, both routes
in this one process on the same images and weights (random); each route is measured in a fresh allocator state."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import esvit_amd
from esvit_amd import analysis
from esvit_amd.models import vision_transformer as V

dev = torch.device("cuda:0")


def timeit(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # milliseconds


def measure(fn, iters):
    """-> (ms per call, peak bytes of one call above what was live before it, the result)"""
    fn()  # (weights cast, scratch allocated)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return timeit(fn, iters), peak, out


def maps_route(model, x):
    with torch.no_grad():
        maps = model.forward_selfattention(x, n=2)
        return torch.stack([torch.special.entr(p.float()).sum(-1) for p in maps]) / 0.6931471805599453


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64", help="images per call, comma-separated")
    ap.add_argument("--patches", default="16,8", help="patch sizes at 224^2: 16 -> 197 tokens, 8 -> 785 tokens")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_attn_stats.jsonl"))
    a = ap.parse_args()
    esvit_amd.set_precision("bf16")
    fh = open(a.out, "w") if a.out else None
    for patch in [int(x) for x in a.patches.split(",")]:
        torch.manual_seed(0)
        model = V.deit_small(patch_size=patch).to(dev).eval()
        N = (224 // patch) ** 2 + 1
        for B in [int(x) for x in a.batches.split(",")]:
            x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev)
            t_new, peak_new, e_new = measure(lambda: analysis.attention_entropy(model, x), a.iters)
            t_old, peak_old, e_old = measure(lambda: maps_route(model, x), a.iters)
            rec = dict(model="deit_small", blocks=len(model.blocks), tokens=N, images=B,
                       stats_ms=round(t_new, 2), stats_peak_MB=round(peak_new / 1e6, 1),
                       maps_ms=round(t_old, 2), maps_peak_MB=round(peak_old / 1e6, 1),
                       max_abs_diff_bits=round((e_new - e_old).abs().max().item(), 5))
            line = json.dumps(rec)
            print(line, flush=True)
            if fh:
                fh.write(line + "\n")
                fh.flush()
            del x, e_new, e_old
        del model
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
