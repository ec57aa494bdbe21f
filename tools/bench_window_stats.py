"""Swin attention-entropy benchmark: the two routes of esvit_amd.analysis.attention_entropy on a SwinTransformer -- "maps"
(forward_selfattention(n=2): every block's fp32 window maps [B * nW, nH, N, N], reduced with torch) and "fused" (the window-statistics
mode of csrc/window_attn.hip / window_attn_big.hip, block by block: no map) -- for Swin-T W7 and Swin-T W14 at 64 images of 224^2,
bf16 (run on the MI355X).

    python tools/bench_window_stats.py [--batch 64] [--rounds 5] [--out FILE]   (default: profiles/window_stats_bench.json)

Both routes run in this one process on the same images and weights (random).  After a warm-up of each (weights cast, scratch sized) the
routes alternate, `rounds` times; the figure of a route is the median of its calls.  The peak allocation of one call above what was live
before it is taken in a fresh allocator state.  One JSON document: a record per model."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import esvit_amd
from esvit_amd import analysis
from esvit_amd import config as CFG

dev = torch.device("cuda:0")
ROUTES = ("maps", "fused")


def one_call(model, x, route):
    """-> milliseconds of one attention_entropy call on that route"""
    analysis.SWIN_STATS = route
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    out = analysis.attention_entropy(model, x)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def peak_of(model, x, route):
    analysis.SWIN_STATS = route
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = analysis.attention_entropy(model, x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--archs", default="swin_tiny_w7,swin_tiny_w14")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "window_stats_bench.json"))
    a = ap.parse_args()
    esvit_amd.set_precision("bf16")
    old = analysis.SWIN_STATS
    recs = []
    try:
        for arch in a.archs.split(","):
            torch.manual_seed(0)
            model = esvit_amd.build_model(CFG.model_config(arch), is_teacher=True, use_dense_prediction=False).to(dev).eval()
            x = torch.randn(a.batch, 3, 224, 224, generator=torch.Generator().manual_seed(a.batch)).to(dev)
            ent = {}
            for r in ROUTES:  # warm-up of each
                ent[r] = one_call(model, x, r)[1]
            diff = max(float((p - q).abs().max()) for p, q in zip(ent["maps"], ent["fused"]))
            del ent
            ms = {r: [] for r in ROUTES}
            for _ in range(a.rounds):  # the routes alternate
                for r in ROUTES:
                    ms[r].append(one_call(model, x, r)[0])
            peaks = {r: peak_of(model, x, r) for r in ROUTES}
            rec = dict(model=arch, images=a.batch, image_size=224, blocks=sum(len(l.blocks) for l in model.layers), rounds=a.rounds,
                       maps_ms=round(statistics.median(ms["maps"]), 2), fused_ms=round(statistics.median(ms["fused"]), 2),
                       maps_ms_all=[round(v, 2) for v in ms["maps"]], fused_ms_all=[round(v, 2) for v in ms["fused"]],
                       maps_peak_MB=round(peaks["maps"] / 1e6, 1), fused_peak_MB=round(peaks["fused"] / 1e6, 1),
                       max_abs_diff_bits=round(diff, 6))
            print(json.dumps(rec), flush=True)
            recs.append(rec)
            del model, x
    finally:
        analysis.SWIN_STATS = old
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), dtype="bf16", records=recs), fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
