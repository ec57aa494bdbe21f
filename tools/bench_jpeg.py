"""GPU JPEG decode of an ImageNet-like batch against Pillow on the same host, one JSON line.

    python tools/bench_jpeg.py [--batches 50] [--warmup 5] [--batch 128] [--threads 16] [--with-step]

Corpus: 128 images with sides 300-520 px, quality 75-95, mostly 4:2:0 with some 4:4:4 and grayscale, plus a few progressive
(host fallback) files, encoded by Pillow from a seed (the fixtures of tests/golden/jpeg_pil.npz when Pillow is missing).
Reports the event-timed warm GPU decode per batch (parallel and serial entropy modes), its entropy-decode throughput over the scan
bytes, the worker's parse cost per image and Pillow's decode per image / per batch across `--threads` threads.

--with-step: the Swin-T step of bench.py (B = the batch) trained from ``data.GpuAugmentedLoader`` over the in-memory encoded corpus
(``collate_encoded``: GPU decode + crops on the loader's side stream) against the same loop over the pre-decoded images
(``collate``: upload + crops), the two legs alternating in one call, free-running and with a ``loss.item()`` read every step as the
reference's loop does.  The workers' collate is done before the timed region in both legs (it runs in DataLoader processes).
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def corpus(n, seed=0):
    try:
        from PIL import Image
    except ImportError:
        z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
        files = [z[k].tobytes() for k in z.files if k.endswith(".file") and str(z[k[:-5] + ".kind"]) == "gpu"]
        return [files[i % len(files)] for i in range(n)]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_jpeg_golden import content
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = (int(v) for v in rng.integers(300, 521, 2))
        a = content(rng, h, w)
        b = io.BytesIO()
        kind = rng.random()
        q = int(rng.integers(75, 96))
        if i % 40 == 39:
            Image.fromarray(a).save(b, "JPEG", quality=q, progressive=True)  # a host fallback
        elif kind < 0.1:
            Image.fromarray(a[:, :, 0]).save(b, "JPEG", quality=q)
        elif kind < 0.25:
            Image.fromarray(a).save(b, "JPEG", quality=q, subsampling=0)
        else:
            Image.fromarray(a).save(b, "JPEG", quality=q, subsampling=2)
        out.append(b.getvalue())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--with-step", action="store_true")
    ap.add_argument("--step-steps", type=int, default=12)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    from esvit_amd import jpeg
    files = corpus(args.batch)
    res = {"batch": args.batch, "file_mb": sum(map(len, files)) / 1e6}
    # the worker half
    t = time.perf_counter()
    reps = 3
    for _ in range(reps):
        batch = jpeg.prepare(files)
    res["worker_prepare_us_per_image"] = (time.perf_counter() - t) / reps / len(files) * 1e6
    t = time.perf_counter()
    for f in files:
        jpeg.parse(f)
    res["worker_parse_us_per_image"] = (time.perf_counter() - t) / len(files) * 1e6
    res["gpu_images"] = int(sum(r.gpu for r in batch.records))
    res["scan_mb"] = batch.scan_bytes / 1e6
    res["lanes"], res["segments"] = batch.n_lanes, batch.n_segments
    try:
        from PIL import Image

        def pil(f):
            return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        t = time.perf_counter()
        for f in files:
            pil(f)
        res["pillow_ms_per_image_1thread"] = (time.perf_counter() - t) / len(files) * 1e3
        with ThreadPoolExecutor(args.threads) as ex:
            list(ex.map(pil, files))
            t = time.perf_counter()
            for _ in range(3):
                list(ex.map(pil, files))
        res["pillow_ms_per_batch_%dthreads" % args.threads] = (time.perf_counter() - t) / 3 * 1e3
    except ImportError:
        pass
    # the device half: the upload + one esvit_jpeg_decode (host fallbacks excluded: a batch of the GPU-path files)
    gpu_files = [f for f, r in zip(files, batch.records) if r.gpu]
    gb = jpeg.prepare(gpu_files)
    for mode, name in ((jpeg.MODE_PARALLEL, "parallel"), (jpeg.MODE_SERIAL, "serial")):
        nb = args.batches if mode == jpeg.MODE_PARALLEL else max(5, args.batches // 10)
        for _ in range(args.warmup):
            jpeg.decode(gb, "cuda", mode=mode)
        torch.cuda.synchronize()
        times = []
        for _ in range(nb):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            jpeg.decode(gb, "cuda", mode=mode)
            e1.record()
            times.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in times)
        res["gpu_decode_ms_%s_median" % name] = ms[len(ms) // 2]
        res["gpu_decode_ms_%s_min" % name] = ms[0]
        res["entropy_MBps_%s" % name] = gb.scan_bytes / 1e6 / (ms[len(ms) // 2] / 1e3)
    res["gpu_images_in_timed_batch"] = len(gpu_files)
    res["worker_prepare_ms_per_batch"] = res["worker_prepare_us_per_image"] * len(files) / 1e3
    if args.with_step:
        res["with_step"] = with_step(files, args.step_steps, 3, args.step_rounds)
    print(json.dumps(res))


def with_step(files, steps, warmup, rounds):
    import torch

    import esvit_amd
    from esvit_amd import data as D
    from esvit_amd import jpeg
    from esvit_amd.engine import EsvitTrainer
    import bench
    dev = torch.device("cuda:0")
    esvit_amd.set_precision("bf16")
    torch.manual_seed(0)
    student, teacher, loss_fn = bench.build(dev, 0.1)
    trainer = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=1)
    B = len(files)
    packed, _ = jpeg.decode(files, dev, check=True)  # Pillow's pixels (the decoder is bit-exact): the pre-decoded leg's images
    decoded = [jpeg.pixels(packed, k).cpu().numpy() for k in range(B)]
    n = warmup + steps
    aug_e = D.DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), (8,), (96,), seed=1)
    aug_d = D.DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), (8,), (96,), seed=1)
    enc = [aug_e.collate_encoded([(f, 0) for f in files]) for _ in range(n)]
    dec = [aug_d.collate([(x, 0) for x in decoded]) for _ in range(n)]
    lr, wd, mom, epoch = 5e-4 * B / 256.0, 0.04, 0.996, 1

    def leg(batches, aug, read_loss):
        t0 = None
        for i, (crops, _) in enumerate(D.GpuAugmentedLoader(batches, aug)):
            if i == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            loss = trainer.step(crops, lr, wd, mom, epoch)
            if read_loss:
                loss.item()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    out = {}
    for read_loss in (False, True):
        key = "loss_item_each_step" if read_loss else "free_running"
        legs = {"decoded_ms": [], "encoded_ms": []}
        for _ in range(rounds):
            legs["decoded_ms"].append(leg(dec, aug_d, read_loss))
            legs["encoded_ms"].append(leg(enc, aug_e, read_loss))
        med = {k: sorted(v)[len(v) // 2] for k, v in legs.items()}
        out[key] = dict(legs, decoded_median=med["decoded_ms"], encoded_median=med["encoded_ms"],
                        encoded_over_decoded=med["encoded_ms"] / med["decoded_ms"])
    return out


if __name__ == "__main__":
    main()
