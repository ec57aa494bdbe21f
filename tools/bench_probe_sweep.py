"""Linear-probe sweep on one MI355X: what G classifiers on one frozen-feature pass cost.  Fixed shapes: Swin-T
features with n_last_blocks = 4 (bf16 backbone, 224^2), batch 128, 1000 classes.  For G in {1, 4, 16}, timed with device events in one
process, every leg warmed, the legs alternated round by round, medians reported:
  (i)   the backbone forward (forward_return_n_last_blocks) of the batch;
  (ii)  the classifier side of one LinearProbeSweep.step: forward GEMM, class-index CE, weight-gradient GEMM, per-member update;
  (iii) G sequential steps of the stock path on the same features: LinearClassifier + F.cross_entropy + torch.optim.SGD.
Writes the numbers to --out (default profiles/probe_sweep_bench.json).  usage: bench_probe_sweep.py [--rounds N] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import esvit_amd
from esvit_amd import config as CFG
from esvit_amd import eval as E

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "probe_sweep_bench.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_probe_sweep.py measures on the GPU: no device found")
dev = torch.device("cuda:0")
B, C, N_LAST, GS = 128, 1000, 4, (1, 4, 16)
esvit_amd.set_precision("bf16")
cfg = CFG.swin_config("swin_tiny_w7", DROP_PATH_RATE=0.0)
depths = [2, 2, 6, 2]  # swin_tiny_w7
model = esvit_amd.build_model(cfg, is_teacher=True).to(dev).eval()
gen = torch.Generator(device=dev).manual_seed(0)
images = torch.randn(B, 3, 224, 224, device=dev, generator=gen)
target = torch.randint(0, C, (B,), device=dev, generator=gen)


def backbone():
    with torch.no_grad():
        return model.forward_return_n_last_blocks(images, N_LAST, False, depths).float()


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median(ts):
    return sorted(ts)[len(ts) // 2]


feats = backbone().contiguous()
D = feats.shape[1]
legs = {"backbone": backbone}
for G in GS:
    lrs = [1e-3 * (i + 1) for i in range(G)]
    sweep = E.LinearProbeSweep(D, C, lrs).to(dev)
    clfs = [E.LinearClassifier(D, C).to(dev) for _ in range(G)]
    opts = [torch.optim.SGD(c.parameters(), lr, momentum=0.9, weight_decay=0) for c, lr in zip(clfs, lrs)]

    def stock(clfs=clfs, opts=opts):
        for clf, opt in zip(clfs, opts):
            loss = torch.nn.functional.cross_entropy(clf(feats), target)
            opt.zero_grad()
            loss.backward()
            opt.step()

    legs["sweep_G%d" % G] = lambda sweep=sweep: sweep.step(feats, target)
    legs["stock_G%d" % G] = stock
for fn in legs.values():  # warm every shape the timed window uses
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {name: [] for name in legs}
for _ in range(args.rounds):
    for name, fn in legs.items():  # alternated: every round runs every leg once
        times[name].append(timed_ms(fn))
med = {name: median(ts) for name, ts in times.items()}
out = {"device": torch.cuda.get_device_name(0), "batch": B, "classes": C, "feature_dim": D, "n_last_blocks": N_LAST, "rounds": args.rounds,
       "unit": "ms, device events, median of the rounds (min, max beside it)",
       "legs": {name: {"median": med[name], "min": min(ts), "max": max(ts)} for name, ts in times.items()},
       "classifier_side_sweep_over_stock": {"G%d" % G: med["sweep_G%d" % G] / med["stock_G%d" % G] for G in GS},
       "whole_step_sweep_G_over_sweep_G1": {"G%d" % G: (med["backbone"] + med["sweep_G%d" % G]) / (med["backbone"] + med["sweep_G1"]) for G in GS},
       "whole_sweep_step_over_G_stock_runs": {"G%d" % G: (med["backbone"] + med["sweep_G%d" % G]) / (G * (med["backbone"] + med["stock_G1"])) for G in GS},
       "acceptance_sweep_G16_not_slower_than_stock_G16": bool(med["sweep_G16"] <= med["stock_G16"])}
for name in legs:
    print("%-12s median %8.3f ms  min %8.3f  max %8.3f" % (name, med[name], min(times[name]), max(times[name])))
print(json.dumps({k: out[k] for k in ("classifier_side_sweep_over_stock", "whole_step_sweep_G_over_sweep_G1", "whole_sweep_step_over_G_stock_runs",
                                      "acceptance_sweep_G16_not_slower_than_stock_G16")}))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
