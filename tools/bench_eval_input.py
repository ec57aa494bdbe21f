"""Evaluation input on one MI355X, one JSON line.

    python tools/bench_eval_input.py [--batch 256] [--reps 20] [--batches 4 x workers] [--passes 3] [--workers 16] [--out FILE]

Corpus: ``tools/bench_jpeg.corpus`` (sides 300-520 px, q 75-95, a few progressive host fallbacks), ``--batch`` files per batch.
(a) the evaluation mode of esvit_aug_crops alone: ResizeCenterCrop(256, 224) of the decoded batch, event-timed, warm, median of ``--reps``;
(b) GPU decode + the transform of a prepared batch, the same way;
(c) extract_features (Swin-T, bf16, NUM_CLASSES 0) images/s from the encoded corpus through GpuEvalLoader over a DataLoader whose
    ``--workers`` workers run collate_encoded;
(d) the same model fed by Pillow in ``--workers`` DataLoader workers (decode, Resize(256, BICUBIC), CenterCrop(224), ToTensor +
    Normalize in numpy: the reference's arithmetic without torchvision).
(c) and (d) are steady-state rates: every pass runs ``--batches`` batches (at least 4 per worker, so every worker stays busy and
the time to fill the pipeline is a small part of a pass), after one warm pass; the median of ``--passes`` timed passes is reported
with every pass's rate.
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MEAN, STD = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)


class PillowEval:
    """dataset of (bytes, index) -> (Pillow-transformed fp32 [3, 224, 224], index)"""

    def __init__(self, files):
        self.files = files

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        import torch
        from PIL import Image
        im = Image.open(io.BytesIO(self.files[i])).convert("RGB")
        w, h = im.size
        short, long = (w, h) if w <= h else (h, w)
        if short != 256:
            nl = int(256 * long / short)
            im = im.resize((256, nl) if w <= h else (nl, 256), Image.BICUBIC)
        w, h = im.size
        oy, ox = int(round((h - 224) / 2.0)), int(round((w - 224) / 2.0))
        x = np.asarray(im.crop((ox, oy, ox + 224, oy + 224)), np.float32) / np.float32(255)
        return torch.from_numpy(((x - MEAN) / STD).transpose(2, 0, 1).copy()), i


def timed(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=0, help="batches per pass (default: 4 per worker)")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    args.batches = args.batches or 4 * args.workers
    import torch

    import esvit_amd
    from bench_jpeg import corpus
    from esvit_amd import config as CFG
    from esvit_amd import eval as E
    from esvit_amd import jpeg
    from esvit_amd import transforms as T
    files = corpus(args.batch)
    tf = T.ResizeCenterCrop()
    res = {"batch": args.batch, "workers": args.workers, "batches_per_pass": args.batches, "passes": args.passes}
    enc = jpeg.prepare(files)
    rows = tf.rows(enc.H, enc.W)
    packed, _ = jpeg.decode(enc, "cuda", check=True)
    res["a_resize_crops_ms"] = timed(lambda: tf(packed, draws=rows), args.reps)
    res["b_decode_plus_transform_ms"] = timed(lambda: tf(jpeg.decode(enc, "cuda")[0], draws=rows), args.reps)
    res["b_decode_alone_ms"] = timed(lambda: jpeg.decode(enc, "cuda"), args.reps)
    t = time.perf_counter()
    tf.collate_encoded([(f, i) for i, f in enumerate(files)])
    res["worker_collate_encoded_ms_per_batch"] = (time.perf_counter() - t) * 1e3
    # (c) / (d): extract_features over args.batches batches of the corpus
    esvit_amd.set_precision("bf16")
    model = esvit_amd.build_model(CFG.swin_config("swin_tiny_w7", DROP_PATH_RATE=0.0), is_teacher=True).cuda().eval()
    items = [(files[i % len(files)], i) for i in range(args.batch * args.batches)]
    dl_kw = dict(batch_size=args.batch, num_workers=args.workers, multiprocessing_context="spawn", persistent_workers=True, prefetch_factor=2)
    for key in ("c_gpu_loader", "d_pillow_workers"):  # one leg's workers at a time (each leg gets the CPUs)
        if key == "c_gpu_loader":
            loader = T.GpuEvalLoader(torch.utils.data.DataLoader(items, collate_fn=tf.collate_encoded, **dl_kw), tf)
        else:
            loader = torch.utils.data.DataLoader(PillowEval([f for f, _ in items]), pin_memory=True, **dl_kw)
        E.extract_features(model, loader)  # warm: workers started, kernels loaded
        torch.cuda.synchronize()
        rates = []
        for _ in range(args.passes):
            t = time.perf_counter()
            E.extract_features(model, loader)
            torch.cuda.synchronize()
            rates.append(len(items) / (time.perf_counter() - t))
        res[key + "_images_per_s_passes"] = rates
        res[key + "_images_per_s"] = sorted(rates)[len(rates) // 2]
        del loader  # shuts the persistent workers down
    x = torch.randn(args.batch, 3, 224, 224, device="cuda")
    with torch.no_grad():
        res["backbone_alone_images_per_s"] = args.batch / (timed(lambda: model(x), 5, 2) / 1e3)
    res["c_over_d"] = res["c_gpu_loader_images_per_s"] / res["d_pillow_workers_images_per_s"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
