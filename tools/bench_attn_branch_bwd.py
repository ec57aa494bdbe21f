"""backward mode of the fused attention branch (kernel + partial reduce + bias fold) vs the present chain (proj weight- and data-gradient
GEMMs, window_attn_bwd, relpos_bias_bwd, qkv weight gradient + pad-row column sums, qkv data gradient, layernorm_bwd_cast) on the stage-0
row counts of one Swin-T W7 step, and the forward with / without the side outputs the chain needs (run on the MI355X):
    python tools/bench_attn_branch_bwd.py [--batch 128] [--reps 9] [--iters 20] [--only both|fused|chain] [--maps 56,24] [--out FILE.jsonl]
What it prints is EVENT TIME PER CALL SEQUENCE (device events around --iters back-to-back Python-level calls, divided by --iters; warm; the
arms alternated window by window; median [min, max] over --reps windows): it includes the gaps between the launches of a sequence and
the allocator.  Kernel time comes from a trace run of this same command (rocprofv3 --kernel-trace --stats -- python tools/... --only ...),
hardware counters from a counter run of its own."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from esvit_amd import ops

dev = torch.device("cuda:0")
C, nH, ws, N = 96, 3, 7, 49
DT = torch.bfloat16


ITERS = 20


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / ITERS  # us per call sequence


def alternate(fns, reps, warm=2):
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            t[i].append(once(f))
    return [(statistics.median(v), min(v), max(v)) for v in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="both", choices=("both", "fused", "chain"))
    ap.add_argument("--maps", default="56,24")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    global ITERS
    ITERS = a.iters
    maps = [int(m) for m in a.maps.split(",")]
    B = a.batch
    ops.set_act_dtype(DT)
    scale = 32 ** -0.5
    recs = []
    for H, nB, who in ((56, 2 * B, "224 crops"), (24, 8 * B, "96 crops")):
        if H not in maps:
            continue
        for shift in (0, 3):
            L = H * H
            M = nB * L
            w2t = torch.from_numpy(ops.window_maps(H, H, ws, shift)[0]).to(dev)
            nW = w2t.numel() // N
            reg = torch.from_numpy(ops.shift_region_ids(H, H, ws, shift)).to(dev) if shift else None
            x, gin = torch.randn(M, C, device=dev), torch.randn(M, C, device=dev) * 0.5
            g1, b1 = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            Wqkv, bqkv = torch.randn(3 * C, C, device=dev) * C ** -0.5, torch.randn(3 * C, device=dev) * 0.1
            Wproj, bproj = torch.randn(C, C, device=dev) * C ** -0.5, torch.randn(C, device=dev) * 0.1
            table = torch.randn((2 * ws - 1) ** 2, nH, device=dev) * 0.5
            index = torch.from_numpy(ops.relative_position_index(ws)).to(dev)
            rs = ((torch.rand(nB, device=dev) > 0.1).float() / 0.9).repeat_interleave(L)
            Wq16, Wp16 = Wqkv.to(DT), Wproj.to(DT)
            Wqp, Wpp = ops.cast_weight(Wqkv, perm32=True), ops.cast_weight(Wproj, perm32=True)
            weights = ops.attn_branch_bwd_weights(Wqkv, Wproj)
            frag = ops.new_bias_frag(nH, N, dev)
            y = torch.empty_like(x)
            _, side = ops.attn_branch_fwd(x, g1, b1, 1e-6, Wqp, bqkv, Wpp, bproj, w2t, L, table, ws, reg, nW, N, nH, scale, rowscale=rs, out=y, bias_frag=frag, save=True)
            xw, mean, rstd, qkv, ao = side
            dyw = (gin * rs[:, None]).to(DT)
            wsp = ops.attn_branch_bwd_workspaces([nB * nW], nH, dev)[:2]
            gx_o, gxa_o = torch.empty_like(x), torch.empty((M, C), dtype=DT, device=dev)
            dqkv_o = torch.empty_like(qkv)

            def chain():
                ops.linear_wgrad(dyw, ao, want_bias=True)
                dao = ops.linear_dgrad(dyw, Wp16)
                _, dws, pad = ops.window_attn_bwd(qkv, bqkv, w2t, L, dao, ao, None, None, ws, reg, nW, N, nH, scale, dqkv_out=dqkv_o, bias_frag=frag)
                ops.relpos_bias_bwd(dws, index, N, table.shape[0])
                _, dbq = ops.linear_wgrad(dqkv_o, xw, want_bias=True)
                ops.colsum(pad, out=dbq[C:], accumulate=True)
                dxw = ops.linear_dgrad(dqkv_o, Wq16)
                ops.layernorm_bwd_cast(dxw, x, mean, rstd, g1, g_in=gin, rowscale=rs, rows_per_sample=1)

            def fused():
                ops.attn_branch_bwd(x, gin, g1, b1, 1e-6, weights, bqkv, w2t, L, ws, reg, nW, N, nH, scale, bias_frag=frag, rowscale=rs, rowscale_out=rs,
                                    workspaces=wsp, gx_out=gx_o, gx_act_out=gxa_o, index=index, table_rows=table.shape[0])

            def fwd_save():
                ops.attn_branch_fwd(x, g1, b1, 1e-6, Wqp, bqkv, Wpp, bproj, w2t, L, None, ws, reg, nW, N, nH, scale, rowscale=rs, out=y, bias_frag=frag, save=side)

            def fwd_plain():
                ops.attn_branch_fwd(x, g1, b1, 1e-6, Wqp, bqkv, Wpp, bproj, w2t, L, None, ws, reg, nW, N, nH, scale, rowscale=rs, out=y, bias_frag=frag)

            if a.only != "both":  # a profiler run of one arm alone
                (t1,) = alternate([fused if a.only == "fused" else chain], a.reps)
                print(json.dumps(dict(map=H, shift=shift, rows=M, only=a.only, us=[round(v, 1) for v in t1])), flush=True)
                del x, gin, y, xw, qkv, ao, dyw, gx_o, gxa_o, dqkv_o, side
                torch.cuda.empty_cache()
                continue
            (tc, tf), (ts, tp) = alternate([chain, fused], a.reps), alternate([fwd_save, fwd_plain], a.reps)
            grid = ops.attn_branch_bwd_grid(DT, C, nB * nW)
            rec = dict(map=H, shift=shift, rows=M, windows=nB * nW, who=who, grid=grid, chain_us=[round(v, 1) for v in tc], fused_us=[round(v, 1) for v in tf],
                       fwd_save_us=[round(v, 1) for v in ts], fwd_plain_us=[round(v, 1) for v in tp],
                       bytes_written_fused=M * C * 6 + grid * (ops.ATTN_BWD_PARTIAL_FLOATS + nH * 4096) * 4)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
            del x, gin, y, xw, qkv, ao, dyw, gx_o, gxa_o, dqkv_o, side
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
