"""Sliding-chunk attention micro-benchmark: the dense route (batched score GEMMs + chunked row softmax, ops.vit_attn_fwd / _bwd) against
the fused kernels (csrc/chunk_attn.hip, ops.sliding_chunk_attn_fwd / _bwd) at the stage shapes of one Vision Longformer pre-training
step and at vil_small's first stage at 448^2 (run on the MI355X).

    python tools/bench_chunk_attn.py [--batch 64] [--out FILE]

One JSON line per shape: forward and backward time of both routes and torch.cuda.max_memory_allocated above the live inputs of each
route (forward + backward).  Inputs are random; each route is measured in a fresh allocator state."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from esvit_amd import ops

dev = torch.device("cuda:0")
W = 7


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


def table(nglo, nx, ny):
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return torch.from_numpy(np.concatenate([np.full(nglo, -1), ((ix // W) << 16 | (iy // W)).reshape(-1)]).astype(np.int32)).to(dev)


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
    ap.add_argument("--batch", type=int, default=64, help="images per step: 2 x batch 224^2 crops, 8 x batch 96^2 crops")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.batch
    shapes = [("vil_tiny s1 224", 56, 48, 1, 2 * B), ("vil_tiny s2 224", 28, 32, 3, 2 * B), ("vil_tiny s1 96", 24, 48, 1, 8 * B),
              ("vil_tiny s2 96", 12, 32, 3, 8 * B), ("vil_small s1 224", 56, 32, 3, 2 * B), ("vil_small s2 224", 28, 64, 3, 2 * B),
              ("vil_small s1 448", 112, 32, 3, 2)]
    fh = open(a.out, "w") if a.out else None
    ops.workspace(1, dev, slot=3)  # (the shared scratch of the fused route exists before the first measurement)
    for name, side, hd, nH, nimg in shapes:
        nglo = 1
        N = nglo + side * side
        lay = (table(nglo, side, side), nglo, W * side)
        g = torch.Generator().manual_seed(0)
        qkv = torch.randn(nimg * N, 3 * nH * hd, generator=g).to(dev).to(torch.bfloat16)
        dout = torch.randn(nimg * N, nH * hd, generator=g).to(dev).to(torch.bfloat16)
        args = (nimg, N, nH, hd ** -0.5, lay)
        d = measure(lambda q, *r: ops.vit_attn_fwd(q, *r[:4], chunk=r[4]), lambda do, s, *r: ops.vit_attn_bwd(do, s, *r[:4], chunk=r[4]), qkv, dout, args)
        f = measure(ops.sliding_chunk_attn_fwd, ops.sliding_chunk_attn_bwd, qkv, dout, args)
        rec = dict(shape=name, grid=side, hd=hd, nH=nH, images=nimg, tokens=N,
                   dense_fwd_us=round(d[0], 1), dense_bwd_us=round(d[1], 1), dense_peak_MB=round(d[2] / 1e6, 1),
                   fused_fwd_us=round(f[0], 1), fused_bwd_us=round(f[1], 1), fused_peak_MB=round(f[2] / 1e6, 1),
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
