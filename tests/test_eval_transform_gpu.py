"""Evaluation input on the MI355X (the evaluation mode of esvit_aug_crops through esvit_amd.transforms): both transforms against Pillow's output
(tests/golden/eval_transform_pil.npz, tolerance 0: the fp32 crop is ToTensor + Normalize of Pillow's bytes) and against the numpy
restatement on a random mixed batch; large and over-limit calls; encoded bytes end to end; the loader; extract_features + k-NN."""
import os

import numpy as np
import pytest
import torch

from tests import eval_transform_ref as R
from tests.test_eval_transform_cpu import gold_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = np.stack([R.to_tensor_normalize(np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, 2))[c, :, 0] for c in range(3)])  # [3, 256]


def to_bytes(x):
    """fp32 [3, S, S] -> the uint8 HWC image it normalises, asserting every value is exactly ToTensor + Normalize of a byte"""
    x = np.asarray(x)
    u8 = np.stack([np.clip(np.searchsorted(LUT[c], x[c]), 0, 255) for c in range(3)])
    assert all(np.array_equal(LUT[c][u8[c]], x[c]) for c in range(3)), "a value is not a normalised byte"
    return np.ascontiguousarray(u8.transpose(1, 2, 0).astype(np.uint8))


def rrc_rows(boxes, S):
    rows = np.zeros((len(boxes), 16), np.int32)
    rows[:, 0] = np.arange(len(boxes))
    rows[:, 1:6] = boxes
    rows[:, 6], rows[:, 7], rows[:, 10] = S, S, 1
    return rows


def test_both_transforms_equal_pillow_fixtures(lib_built):
    from esvit_amd import data as D, transforms as T
    g, imgs = gold_inputs()
    names = list(imgs)
    packed = D.PackedImages([torch.from_numpy(imgs[n]) for n in names])
    boxes = np.stack([g[n + ".rrc_box"] for n in names])
    for key, out in [("cc_small", T.ResizeCenterCrop(32, 24)(packed)), ("cc_small_bl", T.ResizeCenterCrop(32, 24, "bilinear")(packed)),
                     ("rrc_small", T.RandomResizedCropFlip(24)(packed, draws=rrc_rows(boxes, 24))),
                     ("cc224.sha", T.ResizeCenterCrop()(packed)), ("rrc224.sha", T.RandomResizedCropFlip()(packed, draws=rrc_rows(boxes, 224)))]:
        out = out.cpu().numpy()
        for k, n in enumerate(names):
            got = to_bytes(out[k])
            if key.endswith(".sha"):
                assert R.sha256(got) == g[n + "." + key].tobytes().hex(), (key, n)
            else:
                assert np.array_equal(got, g[n + "." + key]), (key, n, int((got != g[n + "." + key]).sum()))


def test_random_mixed_batch_of_128_equals_restatement(lib_built):
    from esvit_amd import data as D, transforms as T
    rng = np.random.default_rng(7)
    B = 128
    shapes = list(zip(rng.integers(20, 640, B), rng.integers(20, 640, B)))
    shapes[:4] = [(256, 341), (200, 200), (1, 1), (700, 90)]
    imgs = [R.synthetic(int(h), int(w), i) for i, (h, w) in enumerate(shapes)]
    packed = D.PackedImages([torch.from_numpy(im) for im in imgs])
    cc = T.ResizeCenterCrop()(packed).cpu().numpy()
    rrc_tf = T.RandomResizedCropFlip(seed=3)
    rows = rrc_tf.rows(packed.H, packed.W)
    rows[::3, 10] = 0  # some crops bicubic, in the same call
    rrc = rrc_tf(packed, draws=rows).cpu().numpy()
    for k, im in enumerate(imgs):
        assert np.array_equal(cc[k], R.to_tensor_normalize(R.resize_center_crop(im, 256, 224))), ("center", k, shapes[k])
        r = rows[k]
        want = R.resized_crop_flip(im, r[1], r[2], r[3], r[4], 224, r[5], "bilinear" if r[10] else "bicubic")
        assert np.array_equal(rrc[k], R.to_tensor_normalize(want)), ("rrc", k, shapes[k], r[:6].tolist())
    one = T.ResizeCenterCrop()(imgs[5])  # the per-sample call: [3, S, S], the batch's row
    assert one.shape == (3, 224, 224) and np.array_equal(one.cpu().numpy(), cc[5])


def test_large_image_and_over_limit_refusal(lib_built):
    from esvit_amd import data as D, ops, transforms as T
    big = R.synthetic(2000, 3000, 9)
    tall = R.synthetic(2600, 140, 10)
    packed = D.PackedImages([torch.from_numpy(big), torch.from_numpy(tall)])
    out = T.ResizeCenterCrop()(packed).cpu().numpy()
    assert np.array_equal(out[0], R.to_tensor_normalize(R.resize_center_crop(big, 256, 224)))
    assert np.array_equal(out[1], R.to_tensor_normalize(R.resize_center_crop(tall, 256, 224)))
    rows = rrc_rows(np.array([[0, 0, 2000, 3000, 1], [0, 0, 2600, 140, 0]]), 96)  # scales 20.8 / 31.3 and 27: the small tiles
    out = T.RandomResizedCropFlip(96)(packed, draws=rows).cpu().numpy()
    assert np.array_equal(out[0], R.to_tensor_normalize(R.resized_crop_flip(big, 0, 0, 2000, 3000, 96, True)))
    assert np.array_equal(out[1], R.to_tensor_normalize(R.resized_crop_flip(tall, 0, 0, 2600, 140, 96, False)))
    assert ops.resize_fits((3000, 96), (3000, 96)) and not ops.resize_fits((1 << 20, 224), (100, 224))
    params = torch.from_numpy(rrc_rows(np.array([[0, 0, 10, 10, 0]]), 224)).cuda()
    with pytest.raises(RuntimeError, match="beyond esvit_query"):
        ops.resize_crops(packed.data, packed.table, params, 224, (1 << 20, 224), (100, 224))


def _jpeg_fixtures():
    j = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    return {k[:-5]: (j[k].tobytes(), str(j[k[:-5] + ".kind"]), j[k[:-5] + ".rgb"] if k[:-5] + ".rgb" in j.files else None)
            for k in j.files if k.endswith(".file")}


def pil_transform(data, row, S):
    """Pillow decode -> the Pillow calls torchvision's PIL back end makes for one evaluation-mode row -> uint8 HWC"""
    import io

    from PIL import Image
    im = Image.open(io.BytesIO(data)).convert("RGB")
    top, left, h, w, flip, rh, rw, oy, ox, filt = (int(v) for v in row[1:11])
    if (top, left, h, w) != (0, 0, im.size[1], im.size[0]):
        im = im.crop((left, top, left + w, top + h))
    if (rw, rh) != im.size:  # (torchvision leaves an image whose shorter side already is the size untouched)
        im = im.resize((rw, rh), Image.BILINEAR if filt else Image.BICUBIC)
    im = im.crop((ox, oy, ox + S, oy + S))
    return np.asarray(im.transpose(Image.FLIP_LEFT_RIGHT) if flip else im)


def test_encoded_end_to_end_with_host_fallbacks(lib_built):
    """GPU decode -> GPU transform == Pillow decode -> Pillow transform, with progressive / CMYK / PNG files (decoded by Pillow in
    the worker) in the same batch"""
    from esvit_amd import jpeg, transforms as T
    fx = _jpeg_fixtures()
    names = [n for n, (_, kind, rgb) in fx.items() if kind in ("gpu", "host") and rgb is not None]
    assert {"prog", "cmyk", "png"} <= set(names)
    for tf in (T.ResizeCenterCrop(), T.RandomResizedCropFlip(seed=1)):
        (enc, rows), targets = tf.collate_encoded([(fx[n][0], i) for i, n in enumerate(names)])
        packed, _ = jpeg.decode(enc, "cuda", check=True)
        got = tf(packed, draws=rows).cpu().numpy()
        assert targets.tolist() == list(range(len(names)))
        for k, n in enumerate(names):
            assert np.array_equal(got[k], R.to_tensor_normalize(pil_transform(fx[n][0], rows[k], 224))), (type(tf).__name__, n)


def test_evaluation_mode_needs_its_flag_and_no_planes(lib_built):
    """the evaluation mode of esvit_aug_crops is selected by ESVIT_AUG_EVAL in S, never by a missing planes pointer alone"""
    import ctypes as C

    from esvit_amd import data as D, ops
    from esvit_amd._lib import lib
    packed = D.PackedImages([torch.from_numpy(R.synthetic(40, 50, 1))])
    params = torch.zeros((1, 24), dtype=torch.int32, device="cuda")
    out = torch.empty((1, 3, 32, 32), dtype=torch.float32, device="cuda")
    planes = torch.empty(3 * 32 * 32 + 4, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.esvit_aug_crops(p(packed.data), p(packed.table), p(params), 1, 32, 40, 50, None, p(out), ops._stream()) == -1
    assert lib.esvit_aug_crops(p(packed.data), p(packed.table), p(params), 1, 32 | ops.AUG_EVAL, 65536, 65536, p(planes), p(out),
                               ops._stream()) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("prefetch", [True, False])
def test_loader_prefetch_corrupt_and_truncated(lib_built, prefetch):
    from esvit_amd import transforms as T
    fx = _jpeg_fixtures()
    names = [n for n, (_, kind, rgb) in fx.items() if kind == "gpu" and rgb is not None][:14]
    names.insert(6, "corrupt")  # the GPU flags it; the loader re-decodes it with Pillow before its batch is yielded
    items = [(fx[n][0], i) for i, n in enumerate(names)]
    tf = T.ResizeCenterCrop(64, 56)
    batches = [tf.collate_encoded(items[i:i + 4]) for i in range(0, len(items), 4)]
    got = []
    for samples, idx in T.GpuEvalLoader(batches, tf, prefetch=prefetch):
        got.append((samples.clone(), idx))
    torch.cuda.synchronize()
    assert len(got) == len(batches)
    rgb = {n: fx[n][2] for n in names if fx[n][2] is not None}
    from PIL import Image  # noqa: F401  (the corrupt image's reference decode)
    import io
    rgb["corrupt"] = np.asarray(Image.open(io.BytesIO(fx["corrupt"][0])).convert("RGB"))
    for b, (samples, idx) in enumerate(got):
        for k, i in enumerate(idx.tolist()):
            want = R.to_tensor_normalize(R.resize_center_crop(rgb[names[i]], 64, 56))
            assert np.array_equal(samples[k].cpu().numpy(), want), (b, names[i])
    trunc = [tf.collate_encoded([items[0], (fx["truncated"][0], 99)])]
    with pytest.raises(OSError):
        for _ in T.GpuEvalLoader(trunc, tf, prefetch=prefetch):
            pass


def test_extract_features_and_knn_through_the_loader_equal_the_pillow_path(lib_built, tmp_path):
    """eval_knn.py over a root/<class>/<file> tree: ReturnIndexDataset-style encoded folder -> collate_encoded -> GpuEvalLoader ->
    extract_features, against Pillow decode + Pillow transform in a plain DataLoader; samples torch.equal, top-1 / top-5 identical"""
    import io

    from PIL import Image

    from esvit_amd import eval as E, jpeg, transforms as T
    from tests.test_composition_cpu import build_nano_backbone
    fx = _jpeg_fixtures()
    names = [n for n, (_, kind, rgb) in fx.items() if kind in ("gpu", "host") and rgb is not None]
    for split in ("train", "val"):
        for i, n in enumerate(names):
            d = tmp_path / split / ("c%d" % (i % 3))
            d.mkdir(parents=True, exist_ok=True)
            (d / (n + ".jpg")).write_bytes(fx[n][0])
    tf = T.ResizeCenterCrop(72, 64)

    class PillowFolder(jpeg.EncodedImageFolder):  # the reference's path: Pillow decode, Pillow resize + crop, ToTensor + Normalize
        def __getitem__(self, i):
            data, idx = super().__getitem__(i)
            im = Image.open(io.BytesIO(data)).convert("RGB")
            rh, rw = R.resize_geometry(im.size[1], im.size[0], 72)
            if (rw, rh) != im.size:
                im = im.resize((rw, rh), Image.BICUBIC)
            oy, ox = R.center_offsets(rh, rw, 64)
            return torch.from_numpy(R.to_tensor_normalize(np.asarray(im.crop((ox, oy, ox + 64, oy + 64))))), idx

    model = build_nano_backbone().cuda()
    feats, labels = {"gpu": {}, "pil": {}}, {}
    for split in ("train", "val"):
        ds = jpeg.EncodedImageFolder(str(tmp_path / split), return_index=True)
        labels[split] = torch.tensor(ds.targets)
        gpu = T.GpuEvalLoader(torch.utils.data.DataLoader(ds, batch_size=5, collate_fn=tf.collate_encoded), tf)
        ref = torch.utils.data.DataLoader(PillowFolder(str(tmp_path / split), return_index=True), batch_size=5)
        a = torch.cat([s.cpu() for s, _ in gpu])
        b = torch.cat([s for s, _ in ref])
        assert a.shape == (len(ds), 3, 64, 64) and torch.equal(a, b), split
        for key, loader in (("gpu", gpu), ("pil", ref)):
            feats[key][split] = torch.nn.functional.normalize(E.extract_features(model, loader), dim=1, p=2)
    top = {key: E.knn_classifier(f["train"], labels["train"], f["val"], labels["val"], 5, 0.07, num_classes=3) for key, f in feats.items()}
    assert top["gpu"] == top["pil"], top
