"""Evaluation input on the GPU: the transforms eval_knn.py and eval_linear.py run through torchvision in CPU
DataLoader workers, applied to a whole batch of decoded images resident in HBM, bit-exact with Pillow's arithmetic:

* :class:`ResizeCenterCrop` -- ``Resize(256, interpolation=3) -> CenterCrop(224) -> ToTensor -> Normalize`` (eval_knn.py:48-53,
  eval_linear.py:56-61: the validation transform);
* :class:`RandomResizedCropFlip` -- ``RandomResizedCrop(224) -> RandomHorizontalFlip -> ToTensor -> Normalize``
  (eval_linear.py:50-55: the probe's training transform; bilinear, torchvision's default).

Each makes one int32 row per image from the image sizes only (numpy, so a DataLoader worker makes them from the JPEG headers) and
the evaluation mode of ``esvit_aug_crops`` (csrc/augment.hip) renders the batch in one launch.  :class:`GpuEvalLoader` turns a DataLoader of
``collate_encoded`` batches into the ``(samples, index_or_label)`` iterator ``eval.extract_features``, ``eval.train_linear_epoch``
and ``eval.validate_network`` consume.  torchvision is not used.
"""
import numpy as np
import torch

from . import data as D
from . import ops

FILTERS = {"bicubic": ops.FILTER_BICUBIC, "bilinear": ops.FILTER_BILINEAR}
RRC_DRAWS = D.U_FLIP + 1  # uniforms per image of RandomResizedCropFlip: the 20 attempts, i, j (data.py's columns) and the flip


def _filter(interpolation):
    if interpolation not in FILTERS:
        raise ValueError("interpolation must be one of %s, got %r" % (sorted(FILTERS), interpolation))
    return FILTERS[interpolation]


def resize_center_crop_rows(H, W, resize=256, crop=224, interpolation="bicubic"):
    """evaluation-mode rows (esvit_aug_crops) of ``Resize(resize) -> CenterCrop(crop)`` for images of H x W pixels (torchvision's PIL rules: the
    shorter side goes to ``resize``, the longer to ``int(resize * long / short)``, nothing is resized when the shorter side already
    is ``resize``; the window starts at ``int(round((size - crop) / 2.0))``, Python's round: half to even)"""
    if crop > resize:
        raise ValueError("ResizeCenterCrop: crop %d > resize %d (torchvision would pad; not supported)" % (crop, resize))
    H, W = np.asarray(H, np.int64), np.asarray(W, np.int64)
    short, long = np.minimum(H, W), np.maximum(H, W)
    new_long = (resize * long / short).astype(np.int64)  # int(size * long / short): a float64 quotient, truncated
    rh, rw = np.where(W <= H, new_long, resize), np.where(W <= H, resize, new_long)
    same = short == resize
    rh, rw = np.where(same, H, rh), np.where(same, W, rw)
    rows = np.zeros((len(H), ops.RESIZE_PARAM_INTS), np.int32)
    rows[:, 0] = np.arange(len(H))
    rows[:, 3], rows[:, 4], rows[:, 6], rows[:, 7] = H, W, rh, rw
    rows[:, 8] = np.rint((rh - crop) / 2.0)
    rows[:, 9] = np.rint((rw - crop) / 2.0)
    rows[:, 10] = _filter(interpolation)
    return rows


def random_resized_crop_rows(u, H, W, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation="bilinear"):
    """evaluation-mode rows (esvit_aug_crops) of ``RandomResizedCrop(size, scale, ratio) -> RandomHorizontalFlip`` from uniforms ``u``
    [n, RRC_DRAWS] in [0, 1): the box and flip logic of :func:`data.sample_params`"""
    u = np.asarray(u, np.float64)
    H, W = np.asarray(H, np.int64), np.asarray(W, np.int64)
    rows = np.zeros((len(H), ops.RESIZE_PARAM_INTS), np.int32)
    rows[:, 0] = np.arange(len(H))
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = D.random_resized_crop_boxes(u, H, W, scale, ratio)
    rows[:, 5] = u[:, D.U_FLIP] < D.P_FLIP
    rows[:, 6], rows[:, 7] = size, size
    rows[:, 10] = _filter(interpolation)
    return rows


def check_rows(rows, H, W, S):
    """refuse rows that would read outside their image or write outside the S x S window (the kernel trusts them)"""
    r = rows.astype(np.int64)
    src = r[:, 0]
    ok = (src >= 0) & (src < len(H))
    Hs, Ws = np.asarray(H, np.int64)[np.where(ok, src, 0)], np.asarray(W, np.int64)[np.where(ok, src, 0)]
    ok &= (r[:, 1] >= 0) & (r[:, 2] >= 0) & (r[:, 3] > 0) & (r[:, 4] > 0) & (r[:, 1] + r[:, 3] <= Hs) & (r[:, 2] + r[:, 4] <= Ws)
    ok &= (r[:, 8] >= 0) & (r[:, 9] >= 0) & (r[:, 8] + S <= r[:, 6]) & (r[:, 9] + S <= r[:, 7]) & np.isin(r[:, 10], list(FILTERS.values()))
    if not ok.all():
        raise ValueError("eval transform: row %d %s is outside its image or window" % (int(np.argmin(ok)), rows[np.argmin(ok)].tolist()))


def render(packed, rows, S):
    """rows through esvit_aug_crops' evaluation mode on the current stream -> fp32 [n, 3, S, S] on the images' device"""
    check_rows(rows, packed.H, packed.W, S)
    dev = packed.data.device
    if dev.type != "cuda":
        raise RuntimeError("esvit_amd.transforms: the eval transforms run on the GPU only")
    r = rows.astype(np.int64)
    ky, kx = int(np.argmax(r[:, 3] / r[:, 6])), int(np.argmax(r[:, 4] / r[:, 7]))  # the largest per-axis scale sizes the LDS
    params = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).pin_memory().to(dev, non_blocking=True)
    return ops.resize_crops(packed.data, packed.table, params, S, (r[ky, 3], r[ky, 6]), (r[kx, 4], r[kx, 7]))


class _EvalTransform:
    """called on a BATCH (a :class:`data.PackedImages` or a list of uint8 HWC tensors / arrays / PIL images) it returns fp32 CUDA
    ``[B, 3, S, S]``; called on ONE image, ``[3, S, S]`` (torchvision's per-sample contract).  ``draws``: rows made earlier
    (by :meth:`collate` / :meth:`collate_encoded` in a DataLoader worker)."""

    def __init__(self, size, device):
        self.size, self.device = int(size), device

    def rows(self, H, W):
        raise NotImplementedError

    def __call__(self, images, draws=None):
        if not isinstance(images, (list, tuple, D.PackedImages)):
            return self.__call__([images], draws=draws)[0]
        packed = images if isinstance(images, D.PackedImages) else D.PackedImages(images, self.device)
        return render(packed, self.rows(packed.H, packed.W) if draws is None else draws, self.size)

    def collate(self, batch):
        """``collate_fn`` for a dataset of ``(uint8 HWC image, label or index)`` -> ``((images, rows), targets)``; the rows are made
        here, in the worker, from the image sizes"""
        images = [torch.as_tensor(np.asarray(x)) for x, _ in batch]
        rows = self.rows([im.shape[0] for im in images], [im.shape[1] for im in images])
        return (images, rows), torch.as_tensor([y for _, y in batch])

    def collate_encoded(self, batch):
        """``collate_fn`` for a dataset of ``(encoded bytes, label or index)`` (``jpeg.EncodedImageFolder``): parses the headers,
        decodes the host-fallback inputs with Pillow and makes the rows from the header sizes -- Python / numpy only, no device
        -> ``((jpeg.Batch, rows), targets)``"""
        from . import jpeg
        enc = jpeg.prepare([x for x, _ in batch])
        return (enc, self.rows(enc.H, enc.W)), torch.as_tensor([y for _, y in batch])


class ResizeCenterCrop(_EvalTransform):
    """``Resize(resize, interpolation) -> CenterCrop(crop) -> ToTensor -> Normalize(ImageNet)`` (eval_knn.py:48-53,
    eval_linear.py:56-61; interpolation=3 there is bicubic).  ``crop > resize`` (torchvision pads) is refused."""

    def __init__(self, resize=256, crop=224, interpolation="bicubic", device="cuda"):
        if crop > resize:
            raise ValueError("ResizeCenterCrop: crop %d > resize %d (torchvision would pad; not supported)" % (crop, resize))
        super().__init__(crop, device)
        self.resize, self.interpolation = int(resize), interpolation
        _filter(interpolation)

    def rows(self, H, W):
        return resize_center_crop_rows(H, W, self.resize, self.size, self.interpolation)


class RandomResizedCropFlip(_EvalTransform):
    """``RandomResizedCrop(size, scale, ratio, interpolation) -> RandomHorizontalFlip -> ToTensor -> Normalize(ImageNet)``
    (eval_linear.py:50-55; torchvision's default interpolation, bilinear).  The algorithm and probabilities are torchvision's, the
    draws come from numpy generators: the same crops as torchvision for the same draws, but not torch's random stream (its
    parity is unpinned, as for DataAugmentationDINO).  In the calling process the draws come from a generator seeded
    with ``seed``.  Inside a DataLoader worker, where that generator would be the same copy in every worker and again at every
    epoch, they come from a generator seeded with the worker's torch seed (and ``seed``): new per worker and per epoch, as torch's
    own stream is for torchvision's transforms."""

    def __init__(self, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation="bilinear", seed=None, device="cuda"):
        super().__init__(size, device)
        self.scale, self.ratio, self.interpolation = tuple(scale), tuple(ratio), interpolation
        _filter(interpolation)
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self._worker = None  # (torch seed of this DataLoader worker, its generator)

    def generator(self):
        """the generator the draws of the current process come from"""
        info = torch.utils.data.get_worker_info()
        if info is None:
            return self.rng
        if self._worker is None or self._worker[0] != info.seed:
            self._worker = (info.seed, np.random.default_rng([info.seed] if self.seed is None else [info.seed, self.seed]))
        return self._worker[1]

    def rows(self, H, W, uniforms=None):
        u = self.generator().random((len(H), RRC_DRAWS)) if uniforms is None else uniforms
        return random_resized_crop_rows(u, H, W, self.size, self.scale, self.ratio, self.interpolation)


class GpuEvalLoader(D.GpuAugmentedLoader):
    """wraps a DataLoader whose collate is an eval transform's ``collate_encoded`` (or ``collate``) into the iterator
    ``eval.extract_features`` / ``train_linear_epoch`` / ``validate_network`` consume: ``(samples fp32 [B, 3, S, S], index or
    label)``.  The machinery is :class:`data.GpuAugmentedLoader`'s: with ``prefetch`` batch n + 1 is uploaded, decoded and
    transformed on a side stream while batch n is consumed; an image the GPU decoder flags corrupt is re-decoded by Pillow and its
    batch rendered again; a truncated file raises Pillow's ``OSError``."""

    def __init__(self, loader, transform, prefetch=True):
        super().__init__(loader, transform, prefetch)

    @property
    def dataset(self):  # extract_features sizes its feature matrix by len(data_loader.dataset)
        return self.loader.dataset
