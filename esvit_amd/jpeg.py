"""JPEG decoding on the GPU into the crop producer's input: ``decode(list_of_bytes, device)`` returns the
:class:`data.PackedImages` ``esvit_aug_crops`` reads plus one int32 status per image, and every pixel equals
``np.asarray(PIL.Image.open(io.BytesIO(b)).convert("RGB"))``.

Two halves:

* the WORKER half (:func:`parse`, :func:`prepare`) is pure Python / numpy: it calls nothing in the HIP library and initialises no
  device (the DataLoader forks its workers; importing the package maps libesvit_hip.so, as it does for the existing ``collate``).
  It walks the markers, builds canonical Huffman lookup tables (T.81 Annex C), removes the byte stuffing, splits the scan at its
  restart markers and gives every input a verdict -- GPU, or the host fallback, where Pillow decodes it;
* the DEVICE half (:func:`decode`) uploads a prepared batch in one copy and makes one ``esvit_jpeg_decode`` call on the current
  stream (csrc/jpeg.hip: entropy decode, islow IDCT, fancy upsampling, YCbCr -> RGB), then drops the host-decoded images into
  their slots of the same packed buffer.

The GPU takes baseline Huffman streams (SOF0, SOF1 with 8-bit samples) with one scan holding every component: grayscale, or YCbCr
with 4:4:4, 4:2:2 or 4:2:0 sampling, any Huffman / quantisation tables (8- or 16-bit), restart intervals and any image size.
Everything else -- progressive, arithmetic, lossless, 12-bit, CMYK / YCCK, RGB (Adobe transform 0, component ids 'R','G','B'),
other samplings, multi-scan, malformed marker structure, non-JPEG files -- is decoded by Pillow, so it equals Pillow by
construction.
"""
import hashlib
import io
import os
from collections import namedtuple

import numpy as np

# ---- limits and layouts shared with include/esvit_hip.h ------------------------------------------------------------------------
IMG_INTS, SEG_INTS, HUFF_INTS, COMP_INTS = 64, 8, 832, 12
LANE_BITS = 4096            # entropy-coded bits per lane of the parallel decode (mode 0)
SEG_ALIGN, SEG_PAD = 4, 8   # every segment starts 4-byte aligned and is followed by >= 8 zero bytes (reads past its end see zeros)
MODE_PARALLEL, MODE_SERIAL = 0, 1

# per-image status bits (``decode(...)[1]``)
ST_CORRUPT = 1      # the GPU found corrupt entropy data (bad code, segment too short, ...): Pillow's decode differs -> re-decode on host
ST_TRUNCATED = 2    # the scan runs past the end of the file (the parser's verdict)
ST_HOST = 4         # decoded by Pillow on the host (a fallback input)
ST_HOST_FAILED = 8  # Pillow raised on it: the slot holds zeros

# zig-zag position -> natural position (T.81 Figure A.6)
NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                    47, 55, 62, 63], np.int64)

Component = namedtuple("Component", "id h v tq td ta")


class Record:
    """what the parser knows of one input.  ``gpu`` is True when the GPU decodes it; otherwise ``reason`` says why not.
    GPU records carry: H, W, comps (frame order), hmax, vmax, mcux, mcuy, quant {tq: int32[64] natural order},
    huff {(class, id): int32[HUFF_INTS] lookup record}, restart (MCUs per interval, 0 = none), segments (list of uint8 arrays:
    the un-stuffed entropy data of every restart interval)."""
    gpu = False
    reason = ""
    truncated = False
    H = W = 0

    def __repr__(self):
        return "Record(gpu=%s, %dx%d, %s)" % (self.gpu, self.H, self.W, self.reason or "ok")


class _Fallback(Exception):
    pass


def huffman_record(counts, symbols, is_dc):
    """canonical decoding tables of one DHT table (T.81 Annex C / F.2.2.3) as the int32 record the kernels read:
    [0, 512) lookup of the next 9 bits -> (length << 8 | symbol), 0 for longer codes; [512, 530) maxcode[l] (-1: no code of
    length l); [530, 548) valoff[l] = index of the first symbol of length l minus the first code of length l; [548, 804) symbols.
    Raises _Fallback on a table libjpeg rejects (too many symbols, an all-ones code, a DC category above 15)."""
    counts = [int(c) for c in counts]
    symbols = [int(s) for s in symbols]
    if sum(counts) > 256 or len(symbols) != sum(counts):
        raise _Fallback("bad Huffman table")
    if is_dc and any(s > 15 for s in symbols):
        raise _Fallback("DC Huffman symbol above 15")
    rec = np.zeros(HUFF_INTS, np.int32)
    maxcode = np.full(18, -1, np.int64)
    valoff = np.zeros(18, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        n = counts[length - 1]
        if n:
            valoff[length] = k - code
            for i in range(n):
                if length <= 9:
                    lo = code << (9 - length)
                    rec[lo:lo + (1 << (9 - length))] = (length << 8) | symbols[k]
                code += 1
                k += 1
            maxcode[length] = code - 1
        if code >= (1 << length):  # jdhuff.c: codes must fit and none may be all ones
            raise _Fallback("bad Huffman table")
        code <<= 1
    maxcode[17] = 0x7FFFFFFF  # the sentinel that ends the slow search
    rec[512:530] = maxcode
    rec[530:548] = valoff
    rec[548:548 + len(symbols)] = symbols
    return rec


def _u16(b, i):
    return (b[i] << 8) | b[i + 1]


def _segments(data, start):
    """split the entropy-coded data starting at ``start`` at its restart markers and remove the stuffing; returns (list of uint8
    segment arrays, RST numbers seen in order, index of the marker that ends the scan or -1 if the file ends first)"""
    buf = np.frombuffer(data, np.uint8)
    body = buf[start:]
    ff = np.flatnonzero(body[:-1] == 0xFF)
    nxt = body[ff + 1]
    is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    ends = ff[(nxt != 0) & (nxt != 0xFF) & ~is_rst]
    end = int(ends[0]) if len(ends) else -1
    n = end if end >= 0 else len(body)
    keep = ff < n
    ff, nxt, is_rst = ff[keep], nxt[keep], is_rst[keep]
    drop = np.zeros(n, bool)
    drop[ff[nxt == 0] + 1] = True      # FF 00: a stuffed FF data byte
    drop[ff[nxt == 0xFF]] = True       # FF FF: fill bytes
    rst = ff[is_rst]
    drop[rst] = True
    drop[rst + 1] = True
    bounds = np.concatenate([[0], rst + 2, [n]])
    segs = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        seg = body[a:b][~drop[a:b]]
        segs.append(seg)
    return segs, (body[rst + 1] - 0xD0).tolist(), (start + end if end >= 0 else -1)


def parse(data):
    """walk the markers of one file -> :class:`Record` (never raises on malformed input: it answers with a fallback verdict)"""
    rec = Record()
    try:
        _parse(bytes(data), rec)
        rec.gpu = True
    except _Fallback as e:
        rec.gpu = False
        rec.reason = str(e)
    except (IndexError, ValueError) as e:  # a header cut short
        rec.gpu = False
        rec.reason = "malformed header (%s)" % type(e).__name__
    return rec


def _parse(b, rec):
    if len(b) < 4 or b[0] != 0xFF or b[1] != 0xD8:
        raise _Fallback("not a JPEG file")
    i = 2
    qt, ht = {}, {}
    jfif = adobe = False
    transform = None
    frame = None
    restart = 0
    while True:
        if i + 4 > len(b):
            rec.truncated = True
            raise _Fallback("truncated before the scan")
        if b[i] != 0xFF:
            raise _Fallback("garbage between markers")
        m = b[i + 1]
        if m == 0xFF:  # fill byte before a marker
            i += 1
            continue
        if m in (0xD8, 0xD9) or 0xD0 <= m <= 0xD7 or m == 0x01:
            raise _Fallback("unexpected marker 0x%02X" % m)
        L = _u16(b, i + 2)
        if L < 2:
            raise _Fallback("bad marker length")
        seg = b[i + 4:i + 2 + L]
        if i + 2 + L > len(b):
            rec.truncated = True
            raise _Fallback("truncated header")
        if m == 0xE0 and L - 2 >= 14 and seg[:5] == b"JFIF\0":  # jdmarker.c examine_app0
            jfif = True
        elif m == 0xEE and L - 2 >= 12 and seg[:5] == b"Adobe":  # examine_app14
            adobe, transform = True, seg[11]
        elif m == 0xDB:
            j = 0
            while j < len(seg):
                pq, tq = seg[j] >> 4, seg[j] & 15
                if tq > 3 or pq > 1:
                    raise _Fallback("bad DQT")
                n = 64 * (pq + 1)
                raw = np.frombuffer(seg[j + 1:j + 1 + n], ">u2" if pq else np.uint8).astype(np.int32)
                if len(raw) != 64:
                    raise _Fallback("bad DQT")
                q = np.zeros(64, np.int32)
                q[NATURAL] = raw
                qt[tq] = q
                j += 1 + n
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                tc, th = seg[j] >> 4, seg[j] & 15
                if tc > 1 or th > 3:
                    raise _Fallback("bad DHT")
                counts = list(seg[j + 1:j + 17])
                n = sum(counts)
                if len(counts) != 16 or j + 17 + n > len(seg):
                    raise _Fallback("bad DHT")
                ht[(tc, th)] = (counts, list(seg[j + 17:j + 17 + n]))
                j += 17 + n
        elif m == 0xDD:
            restart = _u16(seg, 0)
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if m not in (0xC0, 0xC1):
                raise _Fallback({0xC2: "progressive", 0xC3: "lossless", 0xC6: "progressive", 0xC7: "lossless"}.get(
                    m, "arithmetic" if m >= 0xC9 else "hierarchical"))
            if frame is not None:
                raise _Fallback("two frames")
            if seg[0] != 8:
                raise _Fallback("%d-bit samples" % seg[0])
            rec.H, rec.W = _u16(seg, 1), _u16(seg, 3)
            nc = seg[5]
            frame = [Component(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k], 0, 0) for k in range(nc)]
            if len(seg) < 6 + 3 * nc:
                raise _Fallback("bad SOF")
        elif m == 0xCC:
            raise _Fallback("arithmetic")
        elif m == 0xDA:
            break
        elif m == 0xDC:
            raise _Fallback("DNL marker")
        i += 2 + L
    # ---- the frame: what libjpeg would make of it (jdapimin.c default_decompress_parms) ----
    if frame is None:
        raise _Fallback("scan before frame")
    nc = len(frame)
    if rec.H == 0 or rec.W == 0:
        raise _Fallback("empty image")
    if any(not (1 <= c.h <= 4 and 1 <= c.v <= 4) for c in frame):
        raise _Fallback("bad sampling factors")
    if nc == 3:
        if jfif:
            space = "YCbCr"
        elif adobe:
            space = "RGB" if transform == 0 else "YCbCr"
        elif (frame[0].id, frame[1].id, frame[2].id) == (82, 71, 66):
            space = "RGB"
        else:
            space = "YCbCr"
        if space != "YCbCr":
            raise _Fallback("RGB colour space")
        if (frame[1].h, frame[1].v, frame[2].h, frame[2].v) != (1, 1, 1, 1) or (frame[0].h, frame[0].v) not in ((1, 1), (2, 1), (2, 2)):
            raise _Fallback("sampling %dx%d,%dx%d,%dx%d" % tuple(x for c in frame for x in (c.h, c.v)))
    elif nc != 1:
        raise _Fallback("%d components" % nc)
    # ---- the scan header ----
    sos = b[i + 4:i + 2 + L]
    ns = sos[0]
    if ns != nc:
        raise _Fallback("multi-scan")
    comps = []
    for k in range(ns):
        cid, tt = sos[1 + 2 * k], sos[2 + 2 * k]
        if cid != frame[k].id:
            raise _Fallback("scan component order")
        comps.append(frame[k]._replace(td=tt >> 4, ta=tt & 15))
    ss, se, ahl = sos[1 + 2 * ns], sos[2 + 2 * ns], sos[3 + 2 * ns]
    if (ss, se, ahl) != (0, 63, 0):
        raise _Fallback("not a sequential scan")
    quant, huff = {}, {}
    for c in comps:
        if c.tq not in qt:
            raise _Fallback("missing quantisation table")
        quant[c.tq] = qt[c.tq]
        for key in ((0, c.td), (1, c.ta)):
            if key not in ht:
                raise _Fallback("missing Huffman table")
            if key not in huff:
                huff[key] = huffman_record(*ht[key], is_dc=key[0] == 0)
    if nc == 1:
        comps = [comps[0]._replace(h=1, v=1)]  # a single-component scan is not interleaved: one block per MCU whatever the factors
    hmax, vmax = max(c.h for c in comps), max(c.v for c in comps)
    rec.comps, rec.hmax, rec.vmax = comps, hmax, vmax
    rec.mcux, rec.mcuy = -(-rec.W // (8 * hmax)), -(-rec.H // (8 * vmax))
    rec.quant, rec.huff, rec.restart = quant, huff, restart
    # ---- the entropy-coded data ----
    segs, rst, end = _segments(b, i + 2 + L)
    if end < 0:
        rec.truncated = True
        raise _Fallback("truncated scan")
    if b[end:end + 2] != b"\xff\xd9":
        raise _Fallback("multi-scan" if b[end + 1] in (0xDA, 0xC4, 0xDB, 0xDD) else "marker 0x%02X after the scan" % b[end + 1])
    nmcu = rec.mcux * rec.mcuy
    want = -(-nmcu // restart) if restart else 1
    if len(segs) != want or any(r != k % 8 for k, r in enumerate(rst)):
        raise _Fallback("restart markers out of sequence")
    rec.segments = segs


def blocks_per_mcu(rec):
    return sum(c.h * c.v for c in rec.comps)


class Batch:
    """a prepared batch (the worker's output; numpy only): ``host`` uint8 -- the bytes :func:`decode` uploads in one copy --
    with the int32 / int64 views at the offsets below; ``fallback`` {index: uint8 HWC array} of Pillow-decoded images;
    ``status`` int32 [B] host-side status bits; ``files`` the encoded inputs (for a host re-decode of a corrupt image)."""

    def __init__(self, files, records, fallback, status, errors):
        self.files, self.records, self.fallback, self.status, self.errors = files, records, fallback, status, errors
        B = len(records)
        self.H = np.asarray([r.H for r in records], np.int64)
        self.W = np.asarray([r.W for r in records], np.int64)
        sizes = self.H * self.W * 3
        self.offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.out_bytes = int(sizes.sum()) + 4
        # dedupe tables across the batch (most files carry the standard ones)
        qkeys, hkeys = {}, {}
        qlist, hlist = [], []

        def tid(keys, lst, arr):
            k = arr.tobytes()
            if k not in keys:
                keys[k] = len(lst)
                lst.append(arr)
            return keys[k]
        img = np.zeros((B, IMG_INTS), np.int32)
        segrows, lane_seg, chunks = [], [], []
        at, block_base, plane_base, nlanes = 0, 0, 0, 0
        for n, r in enumerate(records):
            img[n, 0], img[n, 1] = r.H, r.W
            img[n, 15] = status[n]
            if not r.gpu:
                continue
            bpm = blocks_per_mcu(r)
            img[n, 2:9] = (len(r.comps), r.hmax, r.vmax, r.mcux, r.mcuy, bpm, r.restart)
            img[n, 9], img[n, 10] = len(segrows), len(r.segments)
            img[n, 11] = block_base
            img[n, 12] = plane_base
            boff = poff = 0
            for c, comp in enumerate(r.comps):
                bw, bh = r.mcux * comp.h, r.mcuy * comp.v
                cw, ch = -(-r.W * comp.h // r.hmax), -(-r.H * comp.v // r.vmax)  # jdinput.c downsampled_width / height
                img[n, 16 + COMP_INTS * c:27 + COMP_INTS * c] = (comp.h, comp.v, tid(qkeys, qlist, r.quant[comp.tq]),
                                                                 tid(hkeys, hlist, r.huff[(0, comp.td)]), tid(hkeys, hlist, r.huff[(1, comp.ta)]),
                                                                 bw, bh, boff, poff, cw, ch)
                boff += bw * bh
                poff += bw * bh * 64
            img[n, 13] = boff
            img[n, 14] = poff
            block_base += boff
            plane_base += (poff + 255) // 256 * 256
            if block_base >= (1 << 31) or plane_base >= (1 << 31):  # the records hold them as int32
                raise ValueError("jpeg: the batch needs more than 2^31 coefficient blocks or plane bytes (image %d): split it" % n)
            nmcu = r.mcux * r.mcuy
            per = r.restart if r.restart else nmcu
            for s, seg in enumerate(r.segments):
                nbits = 8 * len(seg)
                nl = max(1, -(-nbits // LANE_BITS))
                first = s * per
                segrows.append((n, nbits, at, first, min(per, nmcu - first), nlanes, nl, 0))
                lane_seg.append(np.full(nl, len(segrows) - 1, np.int32))
                nlanes += nl
                chunks.append(seg)
                pad = (-len(seg)) % SEG_ALIGN + SEG_PAD
                chunks.append(np.zeros(pad, np.uint8))
                at += len(seg) + pad
        if at >= (1 << 28):
            raise ValueError("jpeg: more than 256 MiB of entropy-coded data in one batch")
        self.n_images, self.n_segments, self.n_lanes, self.n_blocks, self.plane_bytes = B, len(segrows), nlanes, block_base, plane_base
        seg = np.asarray(segrows, np.int32).reshape(-1, SEG_INTS)
        lanes = np.concatenate(lane_seg) if lane_seg else np.zeros(0, np.int32)
        huff = np.stack(hlist) if hlist else np.zeros((0, HUFF_INTS), np.int32)
        quant = np.stack(qlist) if qlist else np.zeros((0, 64), np.int32)
        table = np.stack([self.offsets, self.H, self.W], axis=1).astype(np.int64)
        scan = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
        # the host-decoded images travel in the same upload, copied into their slots on the device
        self.fallback_at, fb = {}, []
        at = 0
        for k, px in sorted(fallback.items()):
            self.fallback_at[k] = (at, px.size)
            fb.append(np.ascontiguousarray(px).reshape(-1))
            at += px.size
        fb = np.concatenate(fb) if fb else np.zeros(0, np.uint8)
        parts = [("table", table), ("images", img), ("segments", seg), ("lane_seg", lanes), ("huff", huff), ("quant", quant), ("scan", scan),
                 ("fallback", fb)]
        self.layout = {}
        total = 0
        for name, a in parts:
            self.layout[name] = (total, a.nbytes, a.dtype, a.shape)
            total += (a.nbytes + 255) // 256 * 256
        host = np.zeros(max(total, 256), np.uint8)
        for name, a in parts:
            o, nb, _, _ = self.layout[name]
            host[o:o + nb] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.host = host
        self.scan_bytes = int(scan.nbytes)

    def __len__(self):
        return len(self.records)


def _pil_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def prepare(files):
    """the worker half: parse every file, decode the fallbacks with Pillow, lay the batch out -> :class:`Batch` (numpy only)"""
    files = [bytes(f) for f in files]
    records, fallback, errors = [], {}, {}
    status = np.zeros(len(files), np.int32)
    for n, f in enumerate(files):
        r = parse(f)
        if not r.gpu:
            status[n] |= ST_HOST | (ST_TRUNCATED if r.truncated else 0)
            try:
                px = _pil_decode(f)
                r.H, r.W = px.shape[0], px.shape[1]
                fallback[n] = px
            except ImportError:
                if not r.truncated:
                    raise RuntimeError("jpeg: input %d needs the host fallback (%s) and Pillow is not installed" % (n, r.reason))
                status[n] |= ST_HOST_FAILED
                errors[n] = "image file is truncated"
            except Exception as e:  # what Pillow raises for this file (OSError for a truncated one)
                status[n] |= ST_HOST_FAILED
                errors[n] = str(e) or type(e).__name__
            if status[n] & ST_HOST_FAILED:
                r.H, r.W = max(r.H, 1), max(r.W, 1)
        records.append(r)
    return Batch(files, records, fallback, status, errors)


# ---- the device half ------------------------------------------------------------------------------------------------------------
def _lib():
    from . import ops  # noqa: F401  (loads the library; imported lazily: the worker half must not)
    from ._lib import lib
    return lib


def workspace_bytes(batch):
    from . import ops
    return ops.query(ops.Q_JPEG_WORKSPACE, batch.n_blocks, batch.plane_bytes, batch.n_lanes | (batch.n_segments << 32))


_STAGE = {}


def _staging(nbytes):
    """pinned upload buffers, two per process, alternated (the copy issued two calls ago has finished before one is reused)"""
    import torch
    bufs = _STAGE.setdefault("bufs", [])
    if not bufs or bufs[0][0].numel() < nbytes:
        bufs[:] = [(torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(2)]
    _STAGE["turn"] = 1 - _STAGE.get("turn", 0)
    return bufs[_STAGE["turn"]]


def decode(files, device="cuda", mode=MODE_PARALLEL, check=False, max_passes=0):
    """decode a batch of encoded images (a list of bytes, or a :func:`prepare`'d :class:`Batch`) on ``device`` ->
    (:class:`data.PackedImages`, int32 status tensor [B] on the device).  All GPU work is enqueued on the current stream.
    ``check``: synchronise, and raise the ``OSError`` Pillow raises for a file it cannot decode (truncated); an image the GPU
    flags as corrupt is re-decoded by Pillow into its slot (Pillow decodes corrupt entropy data with a warning, not an error).
    ``max_passes``: the bound of the parallel decode's sync passes (0: the library's default); a segment that has not converged
    within it is decoded serially -- the result is the same, only the time differs."""
    import ctypes as C

    import torch

    from . import data as D
    from . import ops
    from ._lib import JpegDesc, check as lib_check
    batch = files if isinstance(files, Batch) else prepare(files)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("esvit_amd.jpeg: the decoder runs on the GPU only")
    lib = _lib()
    n = batch.host.nbytes
    stage, ready = _staging(n)
    ready.synchronize()
    stage[:n].numpy()[:] = batch.host
    dbuf = torch.empty(n, dtype=torch.uint8, device=dev)
    dbuf.copy_(stage[:n], non_blocking=True)
    ready.record()

    def view(name, dtype):
        o, nb, _, shape = batch.layout[name]
        return dbuf[o:o + nb].view(dtype).view(shape)
    table = view("table", torch.int64)
    out = torch.empty(batch.out_bytes, dtype=torch.uint8, device=dev)
    out[-4:].zero_()  # the pad bytes the crop producer may read
    status = torch.empty(len(batch), dtype=torch.int32, device=dev)
    ws_bytes = workspace_bytes(batch)
    ws = ops.workspace((ws_bytes + 3) // 4, dev, slot="jpeg_ws")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    desc = JpegDesc(n_images=len(batch), n_segments=batch.n_segments, n_lanes=batch.n_lanes, n_blocks=batch.n_blocks,
                    plane_bytes=batch.plane_bytes, images=p(view("images", torch.int32)), segments=p(view("segments", torch.int32)),
                    lane_seg=p(view("lane_seg", torch.int32)), huff=p(view("huff", torch.int32)), quant=p(view("quant", torch.int32)),
                    scan=p(view("scan", torch.uint8)), table=p(table), out=p(out), status=p(status), mode=int(mode), max_passes=int(max_passes))
    lib_check(lib.esvit_jpeg_decode(C.byref(desc), p(ws), C.c_size_t(ws.numel() * 4), ops._stream()), "jpeg_decode")
    fb = view("fallback", torch.uint8)
    for k, (a, size) in batch.fallback_at.items():
        o = int(batch.offsets[k])
        out[o:o + size].copy_(fb[a:a + size])
    for k in batch.errors:
        o = int(batch.offsets[k])
        out[o:o + int(batch.H[k] * batch.W[k] * 3)].zero_()
    packed = D.PackedImages.from_device(out, table, batch.H, batch.W)
    if check:
        st = status.cpu().numpy()
        for k in np.flatnonzero(st & ST_HOST_FAILED):
            raise OSError(batch.errors.get(int(k), "image file is truncated") + " (image %d of the batch)" % k)
        repair(packed, status, batch, st)
    return packed, status


def repair(packed, status, batch, st=None):
    """re-decode with Pillow every image the GPU flagged corrupt (``status`` read back, or ``st`` given) into its slot: Pillow
    decodes corrupt entropy data with a warning and the GPU's pixels would differ from its.  Returns the indices repaired."""
    import torch
    st = status.cpu().numpy() if st is None else st
    bad = np.flatnonzero((st & ST_CORRUPT) != 0)
    for k in bad:
        px = _pil_decode(batch.files[k])
        o = int(batch.offsets[k])
        packed.data[o:o + px.size].copy_(torch.from_numpy(np.array(px, copy=True).reshape(-1)))
    return bad


def pixels(packed, k):
    """image k of a :class:`data.PackedImages` as a uint8 [H, W, 3] tensor view"""
    o, H, W = int(packed.offsets[k]), int(packed.H[k]), int(packed.W[k])
    return packed.data[o:o + H * W * 3].view(H, W, 3)


class EncodedImageFolder:
    """``root/<class>/<file>`` -> ``(file bytes, class index)`` with torchvision ``ImageFolder``'s ordering: classes are the
    sorted sub-directory names, samples the sorted walk of each class directory (following links) filtered by its image
    extensions.  The bytes feed :meth:`data.DataAugmentationDINO.collate_encoded` or an eval transform's ``collate_encoded``.
    ``return_index=True``: ``(file bytes, sample index)`` instead, as the reference's ReturnIndexDataset (eval_knn.py:235-238)
    yields for ``extract_features``."""

    EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")

    def __init__(self, root, return_index=False):
        self.root = root
        self.return_index = return_index
        self.classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            d = os.path.join(root, c)
            for base, _, names in sorted(os.walk(d, followlinks=True)):
                for name in sorted(names):
                    if name.lower().endswith(self.EXTENSIONS):
                        self.samples.append((os.path.join(base, name), self.class_to_idx[c]))
        self.targets = [t for _, t in self.samples]

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        path, target = self.samples[i]
        with open(path, "rb") as f:
            return f.read(), (i if self.return_index else target)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
