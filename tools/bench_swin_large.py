"""One figure for Swin-L (config.model_config("swin_large_w7")): images/s of EsvitTrainer.step on one MI355X, the workload of bench.py
(2 x 224^2 + 8 x 96^2 synthetic crops, V+R heads, DDINOLoss, per-parameter clip 3.0 + AdamW + teacher EMA, bf16) at B = 64 and
out_dim 65536 -- bench.py is the project's yardstick for the flagship workload and has no choice of this name.

    python tools/bench_swin_large.py [--batch 64] [--steps 10] [--warmup 3] [--out profiles/swin_large_bench.json]

Prints one JSON line and writes it to --out.  One process, one timing loop, nothing to compare against: a record, not a claim."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT_DIM = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--drop-path", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin_large_bench.json"))
    args = ap.parse_args()
    import esvit_amd
    from esvit_amd import config as CFG
    from esvit_amd.data import synthetic_crops
    from esvit_amd.engine import EsvitTrainer
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    esvit_amd.set_precision("bf16")
    torch.manual_seed(0)
    cfg = CFG.model_config("swin_large_w7", DROP_PATH_RATE=args.drop_path)
    nets = []
    for is_teacher in (False, True):
        m = esvit_amd.build_model(cfg, is_teacher=is_teacher, use_dense_prediction=True)
        m.head, m.head_dense = esvit_amd.DINOHead(m.num_features, OUT_DIM), esvit_amd.DINOHead(m.num_features, OUT_DIM)
        nets.append(m.to(dev))
    student, teacher = nets
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    loss_fn = esvit_amd.DDINOLoss(OUT_DIM, 10, 0.04, 0.04, 0, 100).to(dev)
    trainer = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=1)
    B = args.batch
    crops = [c.to(dev) for c in synthetic_crops(B, seed=1234)]
    lr, wd, mom, epoch = 5e-4 * B / 256.0, 0.04, 0.996, 1
    for _ in range(args.warmup):
        trainer.step(crops, lr, wd, mom, epoch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = [trainer.step(crops, lr, wd, mom, epoch) for _ in range(args.steps)]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"metric": "images/sec (global+local crops) Swin-L W=7 V+R", "value": B * args.steps / dt, "unit": "images/s", "ms_per_step": 1e3 * dt / args.steps,
           "n_gpus": 1, "batch": B, "steps": args.steps, "warmup": args.warmup, "dtype": "bf16", "data": "synthetic", "out_dim": OUT_DIM,
           "drop_path": args.drop_path, "parameters_student": sum(p.numel() for p in student.parameters()),
           "final_loss": float(losses[-1]), "losses_finite": all(bool(torch.isfinite(l)) for l in losses), "refused_updates": int(trainer.updater.take_skipped()),
           "peak_memory_gib": torch.cuda.max_memory_allocated() / 2.0 ** 30,
           "note": "one box, one run, nothing to compare against"}
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
