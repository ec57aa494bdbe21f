"""Evaluation input (esvit_amd.transforms), CPU side: the numpy restatement of Resample.c (both filters) and of
torchvision's Resize / CenterCrop / RandomResizedCrop geometry (tests/eval_transform_ref.py) against Pillow live and against the
committed fixtures; the product's header arithmetic compiled for the host against the restatement; the parameter rows the
transforms emit against the restatement; the workers' collate without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import eval_transform_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "eval_transform_pil.npz")

try:
    from PIL import Image
except ImportError:  # pragma: no cover
    Image = None
needs_pil = pytest.mark.skipif(Image is None, reason="Pillow not importable")

EDGE = [(256, 341), (256, 343), (345, 256), (150, 200), (100, 90), (37, 41), (150, 2000), (2000, 150), (2000, 3000), (224, 224), (1, 1),
        (7, 9)]


def gold_inputs():
    g = np.load(GOLD)
    j = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    out = {}
    for k in g.files:
        if k.endswith(".src"):
            name = k[:-4]
            out[name] = j[name + ".rgb"] if str(g[k]) == "jpeg" else R.synthetic(*(int(v) for v in g[name + ".hws"]))
    return g, out


# ---------------------------------------------------------------------------------------------------------------------
# restatement == Pillow
# ---------------------------------------------------------------------------------------------------------------------
@needs_pil
@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_restatement_resize_matches_pillow_live(filt):
    pf = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[filt]
    for seed, (h, w) in enumerate(EDGE):
        img = R.synthetic(h, w, seed)
        for resize in (256, 32):
            rh, rw = R.resize_geometry(h, w, resize)
            want = np.asarray(Image.fromarray(img).resize((rw, rh), pf))
            assert (R.resize_window(img, rh, rw, filt) == want).all(), (h, w, resize, filt)
            oy, ox = R.center_offsets(rh, rw, min(224, resize - 8))
            c = min(224, resize - 8)  # a window of the full resize is the same pixels of Pillow's full resize
            assert (R.resize_window(img, rh, rw, filt, oy, ox, c, c) == want[oy:oy + c, ox:ox + c]).all(), (h, w, resize, filt)
        top, left, bh, bw = R.rrc_get_params(np.random.default_rng(seed).random(23), h, w)
        want = np.asarray(Image.fromarray(img).crop((left, top, left + bw, top + bh)).resize((24, 24), pf).transpose(Image.FLIP_LEFT_RIGHT))
        assert (R.resized_crop_flip(img, top, left, bh, bw, 24, True, filt) == want).all(), (h, w, filt)


def test_restatement_matches_pillow_fixtures():
    g, imgs = gold_inputs()
    assert len(imgs) > 40
    for name, img in imgs.items():
        assert (R.resize_center_crop(img, 32, 24, "bicubic") == g[name + ".cc_small"]).all(), name
        assert (R.resize_center_crop(img, 32, 24, "bilinear") == g[name + ".cc_small_bl"]).all(), name
        top, left, h, w, flip = (int(v) for v in g[name + ".rrc_box"])
        assert (R.resized_crop_flip(img, top, left, h, w, 24, flip) == g[name + ".rrc_small"]).all(), name
        assert R.sha256(R.resize_center_crop(img, 256, 224, "bicubic")) == g[name + ".cc224.sha"].tobytes().hex(), name
        assert R.sha256(R.resized_crop_flip(img, top, left, h, w, 224, flip)) == g[name + ".rrc224.sha"].tobytes().hex(), name


def test_center_offsets_round_half_to_even():
    assert R.center_offsets(256, 341, 224) == (16, 58)   # 58.5 -> 58
    assert R.center_offsets(256, 343, 224) == (16, 60)   # 59.5 -> 60
    assert R.resize_geometry(375, 500, 256) == (256, 341) and R.resize_geometry(500, 375, 256) == (341, 256)
    assert R.resize_geometry(256, 999, 256) == (256, 999) and R.resize_geometry(150, 2000, 256) == (256, 3413)


# ---------------------------------------------------------------------------------------------------------------------
# the product's header, compiled for the host, == restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_math(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("evalmath") / "eval_math_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "esvit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "eval_math_host.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("filt,code", [("bicubic", 0), ("bilinear", 1)])
def test_header_coefficients_both_filters(host_math, filt, code):
    for (n_in, n_out) in [(500, 341), (375, 256), (90, 256), (2000, 256), (3000, 384), (150, 3413), (41, 224), (224, 224), (256, 256),
                          (1, 32), (7, 24), (333, 224), (1100, 96)]:
        bounds, kk = R.coeffs(n_in, n_out, filt)
        kmax = host_math.eval_t_ksize(code, n_in, n_out)
        assert kmax == kk.shape[1], (n_in, n_out)
        for lo, n in [(0, n_out), (n_out // 3, min(n_out - n_out // 3, 17))]:  # the whole axis, and a window of it
            b = np.zeros((n, 2), np.int32)
            k = np.zeros((n, kmax), np.int32)
            host_math.eval_t_coeffs(code, n_in, n_out, lo, n, kmax, _ptr(b), _ptr(k))
            assert (b == bounds[lo:lo + n]).all() and (k == kk[lo:lo + n]).all(), (n_in, n_out, lo)
        if n_in == n_out:  # identity taps: one tap of weight 1 at the position itself
            w = kk[np.arange(n_out)[:, None], np.arange(kk.shape[1])[None, :]]
            first = bounds[:, 0]
            assert ((w * (np.arange(kk.shape[1])[None, :] != (np.arange(n_out) - first)[:, None])) == 0).all()
            assert (w[np.arange(n_out), np.arange(n_out) - first] == 1 << R.PRECISION_BITS).all()


# ---------------------------------------------------------------------------------------------------------------------
# the transforms' rows == restatement of torchvision's geometry
# ---------------------------------------------------------------------------------------------------------------------
def test_center_crop_rows_match_restatement_over_sizes(lib_built):
    from esvit_amd import transforms as T
    H, W = np.meshgrid(np.arange(1, 700, 7), np.arange(1, 700, 11), indexing="ij")
    H, W = np.concatenate([H.ravel(), [256, 256, 2000, 150, 3000]]), np.concatenate([W.ravel(), [341, 343, 150, 2000, 2000]])
    for resize, crop in [(256, 224), (32, 24), (256, 256)]:
        rows = T.resize_center_crop_rows(H, W, resize, crop)
        assert rows.dtype == np.int32 and rows.shape == (len(H), 16)
        for i in range(len(H)):
            rh, rw = R.resize_geometry(int(H[i]), int(W[i]), resize)
            oy, ox = R.center_offsets(rh, rw, crop)
            assert rows[i].tolist() == [i, 0, 0, H[i], W[i], 0, rh, rw, oy, ox, 0, 0, 0, 0, 0, 0], (H[i], W[i], resize)
    assert (T.resize_center_crop_rows([300], [400], interpolation="bilinear")[:, 10] == 1).all()
    with pytest.raises(ValueError):
        T.ResizeCenterCrop(224, 256)


def test_random_resized_crop_rows_match_restatement(lib_built):
    from esvit_amd import transforms as T
    rng = np.random.default_rng(5)
    n = 1500
    u = rng.random((n, T.RRC_DRAWS))
    H, W = rng.integers(1, 900, n), rng.integers(1, 900, n)
    H[:100], W[:100] = 20, rng.integers(300, 900, 100)  # no attempt fits: the central-crop fallback
    for scale, ratio in [((0.08, 1.0), (3 / 4, 4 / 3)), ((0.5, 0.9), (0.5, 2.0))]:
        rows = T.random_resized_crop_rows(u, H, W, 224, scale, ratio)
        for i in range(n):
            top, left, h, w = R.rrc_get_params(u[i], int(H[i]), int(W[i]), scale, ratio)
            assert rows[i].tolist() == [i, top, left, h, w, int(u[i, 22] < 0.5), 224, 224, 0, 0, 1, 0, 0, 0, 0, 0], (i, scale)
        T.check_rows(rows, H, W, 224)
    bad = rows.copy()
    bad[3, 1] = H[3]
    with pytest.raises(ValueError):
        T.check_rows(bad, H, W, 224)


def test_collate_encoded_runs_in_a_worker_without_device(lib_built):
    """the eval transforms' collate_encoded: headers parsed and rows made in a DataLoader worker process (no GPU on this machine)"""
    import torch
    from esvit_amd import jpeg
    from esvit_amd import transforms as T
    j = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    names = ["m420_q75", "m444_q95_opt", "mgray_q85", "s17x33_444_q35"] + (["prog"] if Image is not None else [])
    names = [n for n in names if n + ".file" in j.files]
    items = [(j[n + ".file"].tobytes(), 10 + i) for i, n in enumerate(names)]
    for tf in (T.ResizeCenterCrop(), T.RandomResizedCropFlip(seed=0)):
        loader = torch.utils.data.DataLoader(items, batch_size=len(items), collate_fn=tf.collate_encoded, num_workers=1)
        (enc, rows), targets = next(iter(loader))
        assert isinstance(enc, jpeg.Batch) and targets.tolist() == list(range(10, 10 + len(items)))
        assert rows.shape == (len(items), 16) and (rows[:, 0] == np.arange(len(items))).all()
        if isinstance(tf, T.ResizeCenterCrop):
            assert (rows[:, 3] == enc.H).all() and (rows[:, 4] == enc.W).all()
        T.check_rows(rows, enc.H, enc.W, 224)
    (images, rows), targets = T.ResizeCenterCrop(32, 24).collate([(np.zeros((40, 50, 3), np.uint8), 3)])
    assert rows[0].tolist()[:10] == [0, 0, 0, 40, 50, 0, 32, 40, 4, 8] and targets.tolist() == [3]


def test_random_resized_crop_draws_differ_across_workers_and_epochs(lib_built):
    """in DataLoader workers the draws come from each worker's torch seed: two workers, and two epochs, do not repeat each other's
    boxes (a generator copied into the workers would give every worker, and every epoch, the same draws)"""
    import torch
    from esvit_amd import transforms as T
    tf = T.RandomResizedCropFlip(seed=0)
    items = [(np.zeros((300, 400, 3), np.uint8), i) for i in range(16)]
    torch.manual_seed(0)
    loader = torch.utils.data.DataLoader(items, batch_size=4, collate_fn=tf.collate, num_workers=2)
    epochs = [[rows[:, 1:6].copy() for (_, rows), _ in loader] for _ in range(2)]
    for batches in epochs:
        assert len(batches) == 4
        for a in range(4):
            for b in range(a + 1, 4):
                assert not np.array_equal(batches[a], batches[b]), (a, b)   # batches 0 / 2 come from worker 0, 1 / 3 from worker 1
    for a in range(4):
        assert not np.array_equal(epochs[0][a], epochs[1][a]), a
    main = tf.rows(np.full(4, 300), np.full(4, 400))                        # the calling process keeps its seeded generator
    assert np.array_equal(main, T.RandomResizedCropFlip(seed=0).rows(np.full(4, 300), np.full(4, 400)))
