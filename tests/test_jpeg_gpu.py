"""The JPEG decoder on the MI355X (esvit_amd/jpeg.py + csrc/jpeg.hip) against Pillow's decodes recorded in tests/golden/jpeg_pil.npz
(tools/gen_jpeg_golden.py): bit for bit, in both entropy-decode modes, in mixed batches, repeated and on a side stream, with
malformed inputs, and end to end through the crop producer and the loader."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from esvit_amd import jpeg  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_pil.npz")

try:
    import PIL  # noqa: F401
    HAVE_PIL = True
except ImportError:
    HAVE_PIL = False


def fixtures():
    z = np.load(GOLD)
    out = {}
    for k in z.files:
        if k.endswith(".file"):
            name = k[:-5]
            out[name] = dict(file=z[k].tobytes(), kind=str(z[name + ".kind"]), rgb=z[name + ".rgb"] if name + ".rgb" in z.files else None,
                             sha=z[name + ".sha"].tobytes().hex() if name + ".sha" in z.files else None)
    return out


FIX = fixtures()
GPU_NAMES = [n for n, f in FIX.items() if f["kind"] == "gpu"]
HOST_NAMES = [n for n, f in FIX.items() if f["kind"] == "host"]


def expect_equal(name, got):
    f = FIX[name]
    got = got.cpu().numpy()
    if f["rgb"] is not None:
        assert got.shape == f["rgb"].shape, (name, got.shape, f["rgb"].shape)
        bad = np.argwhere(got != f["rgb"])
        assert len(bad) == 0, "%s: %d bytes differ from Pillow, first at %s" % (name, len(bad), bad[:3].tolist())
    else:
        assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == f["sha"], name


@pytest.mark.parametrize("mode", [jpeg.MODE_PARALLEL, jpeg.MODE_SERIAL])
def test_every_fixture_is_bit_exact(mode):
    files = [FIX[n]["file"] for n in GPU_NAMES]
    packed, status = jpeg.decode(files, "cuda", mode=mode)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all(), dict(zip(GPU_NAMES, status.cpu().tolist()))
    for k, n in enumerate(GPU_NAMES):
        expect_equal(n, jpeg.pixels(packed, k))


def test_each_fixture_alone_both_modes_agree():
    for n in GPU_NAMES:
        a, _ = jpeg.decode([FIX[n]["file"]], "cuda", mode=jpeg.MODE_PARALLEL)
        b, _ = jpeg.decode([FIX[n]["file"]], "cuda", mode=jpeg.MODE_SERIAL)
        assert torch.equal(a.data, b.data), n
        expect_equal(n, jpeg.pixels(a, 0))


@pytest.mark.parametrize("max_passes", [1, 2, 3])
def test_segments_that_do_not_converge_take_the_serial_kernel(max_passes):
    """a bound of 1 sync pass leaves every segment unconverged (all go to jpeg_serial); with 2 the one-lane restart segments converge
    and the multi-lane scans of the larger images do not, so one call mixes jpeg_write and jpeg_serial; 3 is in between"""
    files = [FIX[n]["file"] for n in GPU_NAMES]
    packed, status = jpeg.decode(files, "cuda", max_passes=max_passes)
    assert (status.cpu().numpy() == 0).all()
    for k, n in enumerate(GPU_NAMES):
        expect_equal(n, jpeg.pixels(packed, k))


def _mixed(n=128):
    names = GPU_NAMES + (HOST_NAMES if HAVE_PIL else [])
    names = [x for x in names if x != "big_2000x1500"]
    rng = np.random.default_rng(5)
    return [names[i] for i in rng.permutation(np.arange(n) % len(names))]


def test_mixed_batch_of_128_equals_per_image_results():
    names = _mixed()
    packed, status = jpeg.decode([FIX[n]["file"] for n in names], "cuda")
    st = status.cpu().numpy()
    offs = 0
    table = packed.table.cpu().numpy()
    for k, n in enumerate(names):
        one, st1 = jpeg.decode([FIX[n]["file"]], "cuda")
        want = jpeg.pixels(one, 0)
        assert table[k].tolist() == [offs, want.shape[0], want.shape[1]], (n, table[k])
        assert torch.equal(jpeg.pixels(packed, k), want), n
        assert st[k] == int(st1.cpu()[0]) and st[k] == (jpeg.ST_HOST if FIX[n]["kind"] == "host" else 0), (n, st[k])
        expect_equal(n, want)
        offs += want.numel()
    assert packed.data.numel() == offs + 4


def test_repeated_decodes_are_identical_also_on_a_side_stream():
    names = _mixed(64)
    batch = jpeg.prepare([FIX[n]["file"] for n in names])
    ref, _ = jpeg.decode(batch, "cuda")
    ref = ref.data.clone()
    side = torch.cuda.Stream()
    for it in range(3):
        got, _ = jpeg.decode(batch, "cuda", mode=it % 2)
        assert torch.equal(got.data, ref)
        with torch.cuda.stream(side):
            got2, _ = jpeg.decode(batch, "cuda")
        side.synchronize()
        assert torch.equal(got2.data, ref)


def test_malformed_entries_set_status_and_leave_the_rest_exact():
    names = ["m420_q75", "truncated", "corrupt", "s17x33_gray_q35_opt", "m422_rst_blocks1"]
    files = [FIX[n]["file"] for n in names]
    packed, status = jpeg.decode(files, "cuda")
    st = status.cpu().numpy()
    assert st[1] & jpeg.ST_HOST_FAILED and st[1] & jpeg.ST_TRUNCATED, st
    assert st[2] == jpeg.ST_CORRUPT, st
    for k in (0, 3, 4):
        assert st[k] == 0
        expect_equal(names[k], jpeg.pixels(packed, k))
    serial, st1 = jpeg.decode(files, "cuda", mode=jpeg.MODE_SERIAL)  # the serial kernel flags the same images
    assert st1.cpu().tolist() == st.tolist()
    for k in (0, 3, 4):
        expect_equal(names[k], jpeg.pixels(serial, k))
    with pytest.raises(OSError):
        jpeg.decode(files, "cuda", check=True)
    if HAVE_PIL:  # the corrupt image alone: check=True re-decodes it with Pillow (which warns, not raises)
        packed, status = jpeg.decode([FIX["m420_q75"]["file"], FIX["corrupt"]["file"]], "cuda", check=True)
        assert status.cpu().tolist() == [0, jpeg.ST_CORRUPT]
        expect_equal("m420_q75", jpeg.pixels(packed, 0))
        expect_equal("corrupt", jpeg.pixels(packed, 1))


def test_crops_from_gpu_decoded_images_equal_crops_from_pillow_pixels():
    from esvit_amd import data as D
    names = [n for n in GPU_NAMES if FIX[n]["rgb"] is not None and FIX[n]["rgb"].shape[0] >= 8][:12]
    packed, _ = jpeg.decode([FIX[n]["file"] for n in names], "cuda")
    ref = D.PackedImages([torch.from_numpy(FIX[n]["rgb"].copy()) for n in names])
    aug = D.DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), (8,), (96,), seed=3)
    draws = aug.draw(ref)
    a = aug(packed, draws=draws)
    b = aug(ref, draws=draws)
    torch.cuda.synchronize()
    assert len(a) == 10
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("prefetch", [True, False])
def test_loader_over_encoded_bytes_equals_loader_over_decoded_arrays(prefetch):
    from esvit_amd import data as D
    names = [n for n in GPU_NAMES if FIX[n]["rgb"] is not None and FIX[n]["rgb"].shape[0] >= 8]
    if HAVE_PIL:  # a corrupt image in the third batch: the loader re-decodes it with Pillow before that batch is yielded
        names.insert(9, "corrupt")
    items = [(FIX[n]["file"], i % 5) for i, n in enumerate(names)]
    decoded = [(FIX[n]["rgb"], i % 5) for i, n in enumerate(names)]
    bs = 4
    enc_aug = D.DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), (8,), (96,), seed=11)
    dec_aug = D.DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), (8,), (96,), seed=11)
    enc_batches = [enc_aug.collate_encoded(items[i:i + bs]) for i in range(0, len(items), bs)]
    dec_batches = [dec_aug.collate(decoded[i:i + bs]) for i in range(0, len(items), bs)]
    la = D.GpuAugmentedLoader(enc_batches, enc_aug, prefetch=prefetch)
    lb = D.GpuAugmentedLoader(dec_batches, dec_aug, prefetch=prefetch)
    n = 0
    for (ca, ya), (cb, yb) in zip(la, lb):
        assert torch.equal(ya, yb)
        for x, y in zip(ca, cb):
            assert torch.equal(x, y)
        n += 1
    assert n == len(enc_batches)
