"""Generate tests/golden/jpeg_pil.npz: JPEG (and a few non-JPEG) files encoded by Pillow from seeded synthetic content, with
Pillow's decodes as the expected output.

    python tools/gen_jpeg_golden.py [out.npz]

Per case NAME the archive holds ``NAME.file`` (the encoded bytes, uint8) and either ``NAME.rgb`` (Pillow's
``np.asarray(Image.open(f).convert("RGB"))``) or, for the large images, ``NAME.sha`` (the SHA-256 of those pixels, as uint8 [32])
and ``NAME.shape``.  ``NAME.kind`` is "gpu", "host" (a fallback input), "truncated" or "corrupt".  The GPU tests read only this
archive; they need no Pillow.
"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def content(rng, h, w, kind="mixed"):
    """shading + edges + texture + noise"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "flat":
        return np.full((h, w, 3), (90, 160, 200), np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    base = np.stack([128 + 100 * np.sin(x / (7 + w / 20)) * np.cos(y / (9 + h / 25)),
                     255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1)], -1)
    edges = np.where(((x // 23 + y // 17) % 2)[..., None] == 1, 60.0, -60.0)
    tex = 30 * np.sin(x * 1.7 + y * 0.9)[..., None]
    noise = rng.normal(0, 12, (h, w, 3)) if kind == "mixed" else 0
    if kind == "smooth":
        tex = tex / 4
    return np.clip(base + edges + tex + noise, 0, 255).astype(np.uint8)


def encode(a, fmt="JPEG", mode=None, **kw):
    im = Image.fromarray(a)
    if mode:
        im = im.convert(mode)
    b = io.BytesIO()
    im.save(b, fmt, **kw)
    return b.getvalue()


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


SUB = {"444": 0, "422": 1, "420": 2}


def cases():
    rng = np.random.default_rng(20261016)
    out = []
    small = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 33)]
    qs = [1, 10, 35, 60, 75, 90, 100]
    n = 0
    for h, w in small:
        for samp in ("444", "422", "420", "gray"):
            q = qs[n % len(qs)]
            opt = n % 2 == 1
            a = content(rng, h, w)
            if samp == "gray":
                f = encode(a[:, :, 1], quality=q, optimize=opt)
            else:
                f = encode(a, quality=q, subsampling=SUB[samp], optimize=opt)
            out.append(("s%dx%d_%s_q%d%s" % (h, w, samp, q, "_opt" if opt else ""), f, "gpu"))
            n += 1
    a = content(rng, 333, 501)
    out += [("m420_q75", encode(a, quality=75, subsampling=2), "gpu"),
            ("m444_q95_opt", encode(a[:160, :240], quality=95, subsampling=0, optimize=True), "gpu"),
            ("m422_q50", encode(a, quality=50, subsampling=1), "gpu"),
            ("mgray_q85", encode(a[:200, :, 0], quality=85), "gpu"),
            ("m420_q1", encode(a, quality=1, subsampling=2), "gpu"),
            ("m420_q100", encode(a[:120, :200], quality=100, subsampling=2), "gpu"),
            ("m420_rst_blocks5", encode(a[:, :300], quality=90, subsampling=2, restart_marker_blocks=5), "gpu"),
            ("m444_rst_rows2", encode(a, quality=80, subsampling=0, restart_marker_rows=2, optimize=True), "gpu"),
            ("m422_rst_blocks1", encode(a[:40, :70], quality=70, subsampling=1, restart_marker_blocks=1), "gpu"),
            ("flat_dc_only", encode(content(rng, 64, 96, "flat"), quality=90), "gpu"),
            ("noise_q100", encode(content(rng, 64, 96, "noise"), quality=100, subsampling=0), "gpu"),
            ("noise_q100_420_opt", encode(content(rng, 80, 72, "noise"), quality=100, subsampling=2, optimize=True), "gpu"),
            ("sof1_qt16", encode(content(rng, 48, 80), qtables=[list(range(250, 314)), list(range(300, 364))], subsampling=2), "gpu"),
            ("big_2000x1500", encode(content(rng, 1500, 2000, "smooth"), quality=30, subsampling=2), "gpu"),
            ("prog", encode(content(rng, 64, 64), quality=80, progressive=True), "host"),
            ("cmyk", encode(content(rng, 40, 48), mode="CMYK", quality=85), "host"),
            ("png", encode(content(rng, 20, 30), fmt="PNG"), "host")]
    f = encode(content(rng, 64, 64), quality=75)
    out.append(("truncated", f[:int(len(f) * 0.6)], "truncated"))
    out.append(("corrupt", corrupt(encode(content(rng, 64, 72), quality=75)), "corrupt"))
    return out


def corrupt(f):
    """overwrite 12 bytes in the middle of the scan with six stuffed FF bytes (FF 00): 48 one-bits, and no Huffman code is all
    ones, so the entropy data cannot decode (libjpeg warns and goes on, Pillow returns an image without raising); the restatement
    (tests/jpeg_ref.py) must notice it, as the GPU's status bit must"""
    import jpeg_ref
    start = f.index(b"\xff\xda")
    i = (start + len(f)) // 2
    while b"\xff" in f[i - 1:i + 13]:
        i += 1
    g = f[:i] + b"\xff\x00" * 6 + f[i + 12:]
    try:
        jpeg_ref.decode(g)
    except jpeg_ref.CorruptData:
        return g
    raise RuntimeError("the corruption is not detectable")


def main(path):
    arrays = {}
    for name, f, kind in cases():
        arrays[name + ".file"] = np.frombuffer(f, np.uint8)
        arrays[name + ".kind"] = np.array(kind)
        if kind == "truncated":
            continue
        px = pil_rgb(f)
        if px.size > 200_000:
            arrays[name + ".sha"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest(), np.uint8)
            arrays[name + ".shape"] = np.array(px.shape, np.int64)
        else:
            arrays[name + ".rgb"] = px
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", sum(1 for k in arrays if k.endswith(".file")), "files")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
