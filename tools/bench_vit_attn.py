"""Long-crop ViT attention micro-benchmark: the batched-GEMM route (ops.vit_attn_fwd / _bwd: head split, score GEMM, row softmax, P V
GEMM, head merge; P kept for the backward) against the flash kernels (csrc/flash_attn.hip, ops.global_attn_fwd / _bwd) at the token
counts beyond the one-window kernels: 401 / 577 / 785 tokens (320^2 / 384^2 / 448^2 at patch 16; 785 is also 224^2 at patch 8), head_dim
64, the 6 heads of deit_small (run on the MI355X).

    python tools/bench_vit_attn.py [--batches 32,128,256] [--out FILE]

One JSON line per (tokens, batch): forward and backward time of both routes and torch.cuda.max_memory_allocated above the live inputs
of each route (forward + backward), both routes in this one process on the same inputs.  Inputs are random; each route is measured
in a fresh allocator state."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from esvit_amd import ops

dev = torch.device("cuda:0")


def timeit(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # microseconds


def measure(fwd, bwd, qkv, dout, args):
    """-> (forward us, backward us, peak bytes of one forward + backward above what was live before it)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, saved = fwd(qkv, *args)
    dq = bwd(dout, saved, *args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out, dq
    t_f = timeit(lambda: fwd(qkv, *args))
    t_b = timeit(lambda: bwd(dout, saved, *args))
    del saved
    return t_f, t_b, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,128,256", help="images per call, comma-separated")
    ap.add_argument("--tokens", default="401,577,785")
    ap.add_argument("--heads", type=int, default=6)
    ap.add_argument("--head-dim", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nH, hd = a.heads, a.head_dim
    fh = open(a.out, "w") if a.out else None
    for N in [int(x) for x in a.tokens.split(",")]:
        for B in [int(x) for x in a.batches.split(",")]:
            ops.workspace(ops.query(ops.Q_GLOBAL_ATTN_WS, B * nH, N, 1), dev, slot=3)  # (the shared scratch exists before the measurement)
            g = torch.Generator().manual_seed(0)
            qkv = torch.randn(B * N, 3 * nH * hd, generator=g).to(dev).to(torch.bfloat16)
            dout = torch.randn(B * N, nH * hd, generator=g).to(dev).to(torch.bfloat16)
            args = (B, N, nH, hd ** -0.5)
            d = measure(ops.vit_attn_fwd, ops.vit_attn_bwd, qkv, dout, args)
            f = measure(ops.global_attn_fwd, ops.global_attn_bwd, qkv, dout, args)
            rec = dict(tokens=N, images=B, nH=nH, hd=hd,
                       gemm_fwd_us=round(d[0], 1), gemm_bwd_us=round(d[1], 1), gemm_peak_MB=round(d[2] / 1e6, 1),
                       flash_fwd_us=round(f[0], 1), flash_bwd_us=round(f[1], 1), flash_peak_MB=round(f[2] / 1e6, 1),
                       speedup_fwd=round(d[0] / f[0], 2), speedup_bwd=round(d[1] / f[1], 2))
            line = json.dumps(rec)
            print(line, flush=True)
            if fh:
                fh.write(line + "\n")
                fh.flush()
            del qkv, dout
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
