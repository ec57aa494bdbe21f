"""Cost of the training-health monitor (esvit_amd/monitor.py) on the MI355X.

  kernel   the row-statistics kernel (ops.dist_stats: entropy, argmax, column sums of the probabilities) against
           esvit_teacher_row_stats on the same [12544, 65536] bf16 rows -- the region-level teacher logits of the B = 128 step; that
           kernel reads the same bytes and is the yardstick
  step     the Swin-T B = 128 training step with the monitor off, at period 10 and at period 1

The legs alternate within one process (measuring-on-mi355x: compare two versions in the same call, alternating them); the medians
over the rounds are reported.   python tools/bench_monitor.py [--out profiles/monitor_bench.json] [--no-step]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_leg(R, K, rounds, iters):
    from esvit_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    t = (torch.randn(R, K, device="cuda", generator=g) * 0.25).bfloat16()
    center = torch.randn(K, device="cuda", generator=g) * 0.05
    stats = ops.teacher_row_stats(t, center, 25.0)
    buf = torch.empty(ops.query(ops.Q_DIST_STATS, R, K), dtype=torch.float32, device="cuda")
    legs = {"teacher_row_stats": lambda: ops.teacher_row_stats(t, center, 25.0), "dist_stats": lambda: ops.dist_stats(t, center, 25.0, stats, buf=buf)}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn, iters))
    med = {k: statistics.median(v) for k, v in ms.items()}
    read = R * K * 2
    ws = 2 * (buf.numel() - K) * 4
    ent = ops.dist_stats(t, center, 25.0, stats, buf=buf)[0]
    return {"rows": R, "K": K, "dtype": "bf16", "rounds": rounds, "iters_per_round": iters, "ms_all": ms, "ms_median": med,
            "ratio_dist_stats_over_teacher_row_stats": med["dist_stats"] / med["teacher_row_stats"],
            "row_bytes": read, "workspace_bytes_written_and_read": ws,
            "GBps_rows_only": {k: read / v / 1e6 for k, v in med.items()}, "mean_entropy": float(ent.mean())}


def step_leg(B, rounds, steps):
    import bench
    import esvit_amd
    from esvit_amd.engine import EsvitTrainer
    from esvit_amd.monitor import TrainingMonitor
    dev = torch.device("cuda", 0)
    esvit_amd.set_precision("bf16")
    torch.manual_seed(0)
    student, teacher, loss_fn = bench.build(dev, 0.1, "swin_tiny_w7")
    trainer = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=1)
    crops = [c.to(dev) for c in bench.synthetic_crops(B, seed=1234)]
    lr = 5e-4 * B / 256.0
    legs = {"off": None, "period_10": 10, "period_1": 1}

    def run(period, n):
        loss_fn.monitor = None if period is None else TrainingMonitor(period=period)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            trainer.step(crops, lr, 0.04, 0.996, 1)
        if loss_fn.monitor is not None:
            seen = loss_fn.monitor.compute()  # the one synchronisation of a look
        else:
            seen = {}
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, seen

    for p in legs.values():  # warm every leg's shapes
        run(p, 3)
    ms, last = {k: [] for k in legs}, {}
    for _ in range(rounds):
        for k, p in legs.items():
            t, seen = run(p, steps)
            ms[k].append(t)
            last[k] = seen
    loss_fn.monitor = None
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"arch": "swin_tiny_w7", "batch": B, "rounds": rounds, "steps_per_round": steps, "ms_per_step_all": ms, "ms_per_step_median": med,
            "look_ms": med["period_1"] - med["off"], "period_10_overhead_pct": 100.0 * (med["period_10"] - med["off"]) / med["off"],
            "period_1_overhead_pct": 100.0 * (med["period_1"] - med["off"]) / med["off"], "monitor_values_period_1": last["period_1"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitor_bench.json"))
    ap.add_argument("--rows", type=int, default=12544)
    ap.add_argument("--K", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_monitor.py measures on the GPU"
    out = {"device": torch.cuda.get_device_name(0), "kernel": kernel_leg(args.rows, args.K, args.rounds, 10)}
    if not args.no_step:
        out["step"] = step_leg(args.batch, max(3, args.rounds - 2), 20)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if not kk.endswith("_all")}) for k, v in out.items()}))


if __name__ == "__main__":
    main()
