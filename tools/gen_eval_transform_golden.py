"""Generate tests/golden/eval_transform_pil.npz: the evaluation transforms of eval_knn.py / eval_linear.py rendered by Pillow, as
torchvision's PIL back end calls it, on the decoded files of tests/golden/jpeg_pil.npz and on synthetic images at edge sizes.

    python tools/gen_eval_transform_golden.py [out.npz]

Inputs: ``NAME.src`` is "jpeg" (the Pillow decode stored as ``NAME.rgb`` in jpeg_pil.npz) or "synth" (``tests/eval_transform_ref.
synthetic(h, w, seed)`` with ``NAME.hws`` = (h, w, seed)).  Outputs, uint8 HWC as Pillow leaves them before ToTensor:
  NAME.cc_small     Resize(32, BICUBIC) -> CenterCrop(24)          NAME.cc_small_bl  the same with BILINEAR
  NAME.rrc_small    crop(NAME.rrc_box) -> resize((24, 24), BILINEAR) -> flip if the box says so
  NAME.cc224.sha / NAME.rrc224.sha   SHA-256 of Resize(256, BICUBIC) -> CenterCrop(224) / the RandomResizedCrop(224) of the box
``NAME.rrc_box`` = (top, left, h, w, flip): RandomResizedCrop.get_params + RandomHorizontalFlip of seeded uniforms (the geometry
is torchvision's, restated in tests/eval_transform_ref.py: torchvision is not needed).
"""
import hashlib
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_transform_ref as R  # noqa: E402

PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
# (name, h, w): shorter side exactly 256 / 32, below 224 (upsampling), extreme aspect ratios, large, and centre offsets
# (size - crop) / 2 = k + 0.5 with k even (rounds down) and odd (rounds up) for both crop sizes
SYNTH = [("short256_a", 256, 341), ("short256_b", 256, 343), ("short256_c", 345, 256), ("up_150x200", 150, 200), ("up_100x90", 100, 90),
         ("up_37x41", 37, 41), ("wide_150x2000", 150, 2000), ("tall_2000x150", 2000, 150), ("large_2000x3000", 2000, 3000),
         ("short32_a", 32, 41), ("short32_b", 32, 43), ("square_224", 224, 224), ("odd_375x500", 375, 500)]
SMALL, SMALL_RESIZE, BIG, BIG_RESIZE = 24, 32, 224, 256


def pil_resize_center_crop(img, resize, crop, filt):
    im = Image.fromarray(img)
    rh, rw = R.resize_geometry(img.shape[0], img.shape[1], resize)
    if (rh, rw) != img.shape[:2]:  # torchvision returns the image untouched when the shorter side already is `resize`
        im = im.resize((rw, rh), PIL_FILTER[filt])
    oy, ox = R.center_offsets(rh, rw, crop)
    return np.asarray(im.crop((ox, oy, ox + crop, oy + crop)))


def pil_rrc(img, box, size):
    top, left, h, w, flip = box
    im = Image.fromarray(img).crop((left, top, left + w, top + h)).resize((size, size), Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


def inputs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    out = []
    for k in z.files:
        if k.endswith(".rgb") and str(z[k[:-4] + ".kind"]) in ("gpu", "host"):
            out.append((k[:-4], "jpeg", z[k], None))
    for seed, (name, h, w) in enumerate(SYNTH):
        out.append((name, "synth", R.synthetic(h, w, seed), (h, w, seed)))
    return out


def main(path):
    rng = np.random.default_rng(20261016)
    arrays = {}
    for name, src, img, hws in inputs():
        arrays[name + ".src"] = np.array(src)
        if hws is not None:
            arrays[name + ".hws"] = np.array(hws, np.int64)
        u = rng.random(23)
        top, left, h, w = R.rrc_get_params(u, img.shape[0], img.shape[1])
        box = (top, left, h, w, int(u[22] < 0.5))
        arrays[name + ".rrc_box"] = np.array(box, np.int64)
        arrays[name + ".cc_small"] = pil_resize_center_crop(img, SMALL_RESIZE, SMALL, "bicubic")
        arrays[name + ".cc_small_bl"] = pil_resize_center_crop(img, SMALL_RESIZE, SMALL, "bilinear")
        arrays[name + ".rrc_small"] = pil_rrc(img, box, SMALL)
        for key, a in (("cc224", pil_resize_center_crop(img, BIG_RESIZE, BIG, "bicubic")), ("rrc224", pil_rrc(img, box, BIG))):
            arrays[name + "." + key + ".sha"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", sum(1 for k in arrays if k.endswith(".src")), "inputs")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "eval_transform_pil.npz"))
