"""Tail of the stage-0 attention-branch backward: ops.attn_tail_bwd (one pass + reduce) against the launches it replaces (qkv weight
gradient with its split-K reduce, qkv data gradient, norm1's backward with its partial reduce) at the B = 128 row count of Swin-T's
stage 0, with and without the activation-dtype copy of dL/dx.

    python tools/bench_attn_tail.py                       both arms, event-timed in one process (us per call, interleaved rounds)
    python tools/bench_attn_tail.py --arm fused           one arm only: the command a kernel trace runs,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_attn_tail.py --arm chain --iters 10
    python tools/bench_attn_tail.py --fold A_kernel_stats.csv B_kernel_stats.csv   the two traces' kernel times per call, side by side

The chain arm runs on ONE stream: its weight gradient, which the training step puts on the side stream, is counted in full -- the
trace's kernel times are what each launch costs, not what the step hides of it."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(M, C, dev):
    import torch
    from esvit_amd import ops
    g = torch.Generator(device=dev).manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    x = r(M, C) * 1.5 + 0.3
    a = dict(x=x, dqkv=(r(M, 3 * C) * 0.2).bfloat16(), g_in=r(M, C) * 0.5, gamma=1.0 + 0.2 * r(C), beta=0.1 * r(C), Wqkv=(r(3 * C, C) * 0.08).bfloat16(),
             rowscale=(torch.rand(M, generator=g, device=dev) > 0.1).float() / 0.9)
    a["xw"], _, a["mean"], a["rstd"] = ops.layernorm_fwd(x, a["gamma"], a["beta"], 1e-6, dtype=torch.bfloat16)
    return a


def chain(ops, a, act):
    dW, db = ops.linear_wgrad(a["dqkv"], a["xw"], want_bias=True)
    dxw = ops.linear_dgrad(a["dqkv"], a["Wqkv"])
    if act:
        return ops.layernorm_bwd_cast(dxw, a["x"], a["mean"], a["rstd"], a["gamma"], g_in=a["g_in"], rowscale=a["rowscale"], rows_per_sample=1)
    return ops.layernorm_bwd(dxw, a["x"], a["mean"], a["rstd"], a["gamma"], g_in=a["g_in"])


def fused(ops, a, act):
    return ops.attn_tail_bwd(a["dqkv"], a["x"], a["mean"], a["rstd"], a["gamma"], a["beta"], a["Wqkv"], a["g_in"], rowscale=a["rowscale"] if act else None,
                             rows_per_sample=1, want_act=act)


def fold(paths):
    """kernel_stats.csv of one trace per arm -> us per call of every kernel above 1 us, and the arms' sums"""
    for p in paths:
        rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(p))]
        print("# %s" % os.path.basename(p))
        for name, calls, ns in sorted(rows, key=lambda t: -t[2]):
            if ns / calls >= 1000.0:
                print("%10.1f us x %4d  %s" % (ns / calls / 1e3, calls, name[:110]))
        print("%10.1f us in all kernels" % (sum(t[2] for t in rows) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1392640)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--arm", choices=("both", "chain", "fused"), default="both")
    ap.add_argument("--fold", nargs="+")
    o = ap.parse_args()
    if o.fold:
        return fold(o.fold)
    import torch
    from esvit_amd import ops
    dev = torch.device("cuda:0")
    C = 96
    a = make(o.rows, C, dev)
    arms = [n for n in ("chain", "fused") if o.arm in ("both", n)]
    fns = dict(chain=chain, fused=fused)
    res = {}
    for act in (False, True):
        for n in arms:  # warm-up (allocator, LDS attribute, weight caches)
            for _ in range(2):
                fns[n](ops, a, act)
        for rnd in range(o.rounds):
            for n in arms:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(o.iters):
                    fns[n](ops, a, act)
                e1.record()
                torch.cuda.synchronize()
                res.setdefault("%s_%s_us" % (n, "act" if act else "plain"), []).append(round(e0.elapsed_time(e1) * 1e3 / o.iters, 1))
    tc = o.rows * C
    out = dict(C=C, rows=o.rows, iters=o.iters, **res)
    for act, nb in (("plain", 18), ("act", 20)):
        k = "fused_%s_us" % act
        if k in res:
            out["fused_%s_GBs" % act] = round(nb * tc / (min(res[k]) * 1e-6) / 1e9)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
