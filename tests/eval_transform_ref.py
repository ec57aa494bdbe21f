"""Numpy restatement of the evaluation transforms (eval_knn.py:48-53, eval_linear.py:50-61) as torchvision's PIL back end runs
them, for the tests of esvit_amd.transforms: Resample.c (precompute_coeffs + normalize_coeffs_8bpc, horizontal pass to uint8, then
vertical) with its bicubic and bilinear filters, and torchvision's Resize / CenterCrop / RandomResizedCrop geometry.  Independent of
the product: plain Python / numpy, no HIP library, no Pillow (the tests check it against Pillow live)."""
import hashlib
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {"bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0)}


def coeffs(in_size, out_size, filt):
    """bounds [out, 2] (first tap, taps) and fixed-point taps [out, ksize] of one axis resized in_size -> out_size"""
    fn, sup = FILTERS[filt]
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = sup * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass0(img, out_size, filt, lo=0, hi=None):
    """resample axis 0 of a uint8 [n, m, 3] array to out_size, output positions [lo, hi) only; uint8 result as Resample.c"""
    bounds, kk = coeffs(img.shape[0], out_size, filt)
    hi = out_size if hi is None else hi
    bounds, kk = bounds[lo:hi], kk[lo:hi]
    idx = np.minimum(bounds[:, :1] + np.arange(kk.shape[1])[None, :], img.shape[0] - 1)  # taps past `count` have weight 0
    k = np.where(np.arange(kk.shape[1])[None, :] < bounds[:, 1:], kk, 0)
    acc = np.full((hi - lo,) + img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    src = img.astype(np.int64)
    for t in range(kk.shape[1]):
        acc += src[idx[:, t]] * k[:, t].reshape((-1,) + (1,) * (img.ndim - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_window(img, rh, rw, filt, off_y=0, off_x=0, S_h=None, S_w=None):
    """``img.resize((rw, rh), filt)`` restricted to the window [off_y, off_y + S_h) x [off_x, off_x + S_w): a pass that would not
    change its axis (size kept) is skipped, as Resample.c skips it; taps are per output position, so the window equals the same
    pixels of the full resize"""
    H, W = img.shape[:2]
    S_h = rh if S_h is None else S_h
    S_w = rw if S_w is None else S_w
    x = img
    if rw != W:
        x = _pass0(np.ascontiguousarray(x.transpose(1, 0, 2)), rw, filt, off_x, off_x + S_w).transpose(1, 0, 2)
    else:
        x = x[:, off_x:off_x + S_w]
    if rh != H:
        x = _pass0(np.ascontiguousarray(x), rh, filt, off_y, off_y + S_h)
    else:
        x = x[off_y:off_y + S_h]
    return np.ascontiguousarray(x)


def resize_geometry(H, W, resize):
    """torchvision F.resize (PIL, int size): (rh, rw)"""
    short, long = (W, H) if W <= H else (H, W)
    if short == resize:
        return H, W
    new_long = int(resize * long / short)
    return (new_long, resize) if W <= H else (resize, new_long)


def center_offsets(rh, rw, crop):
    """torchvision F.center_crop: int(round((size - crop) / 2.0))"""
    return int(round((rh - crop) / 2.0)), int(round((rw - crop) / 2.0))


def resize_center_crop(img, resize, crop, filt="bicubic"):
    """Resize(resize) -> CenterCrop(crop) as uint8 HWC"""
    rh, rw = resize_geometry(img.shape[0], img.shape[1], resize)
    oy, ox = center_offsets(rh, rw, crop)
    return resize_window(img, rh, rw, filt, oy, ox, crop, crop)


def rrc_get_params(u, H, W, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCrop.get_params with its uniforms taken from u[0:20] (attempts: area, log-aspect), u[20] (i), u[21] (j)"""
    area = H * W
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for a in range(10):
        target_area = area * (scale[0] + (scale[1] - scale[0]) * u[2 * a])
        aspect_ratio = math.exp(log_ratio[0] + (log_ratio[1] - log_ratio[0]) * u[2 * a + 1])
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            return int(math.floor(u[20] * (H - h + 1))), int(math.floor(u[21] * (W - w + 1))), h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w, h = W, int(round(W / min(ratio)))
    elif in_ratio > max(ratio):
        h, w = H, int(round(H * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def resized_crop_flip(img, top, left, h, w, size, flip, filt="bilinear"):
    """F.resized_crop (crop, then resize) -> hflip, uint8 HWC"""
    x = resize_window(np.ascontiguousarray(img[top:top + h, left:left + w]), size, size, filt)
    return np.ascontiguousarray(x[:, ::-1]) if flip else x


def to_tensor_normalize(img):
    x = img.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    return (x - np.asarray(MEAN, np.float32)[:, None, None]) / np.asarray(STD, np.float32)[:, None, None]


def synthetic(h, w, seed):
    """deterministic uint8 content (integer arithmetic only): gradients, edges and a hashed texture"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    r = (x * 255 // max(w - 1, 1) + seed * 17) % 256
    g = (y * 255 // max(h - 1, 1) + np.where(((x // 13 + y // 11) % 2) == 1, 60, 0)) % 256
    b = ((x * 2654435761 + y * 40503 + seed * 97) >> 7) % 256
    return np.ascontiguousarray(np.stack([r, g, b], -1).astype(np.uint8))


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
