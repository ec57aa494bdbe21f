"""CPU restatement of the JPEG decoder (esvit_amd/csrc/jpeg.hip + jpeg_math.h) in numpy, independent of the kernels' code: a
serial Huffman decoder over the parser's segments (T.81 F.2.2), the islow IDCT vectorised over blocks, libjpeg's fancy upsampling
and its YCbCr -> RGB tables.  Pillow is the judge of this module (tests/test_jpeg_cpu.py), and this module is the judge of
jpeg_math.h compiled for the host."""
import numpy as np

from esvit_amd import jpeg

F = dict(F0_298=2446, F0_390=3196, F0_541=4433, F0_765=6270, F0_899=7373, F1_175=9633, F1_501=12299, F1_847=15137, F1_961=16069,
         F2_053=16819, F2_562=20995, F3_072=25172)


class CorruptData(Exception):
    pass


def _tables(rec):
    """{(length, code): symbol} from a kernel lookup record: the codes of length l run from k - valoff[l] to maxcode[l], k being
    the index of the first symbol of that length"""
    maxcode, valoff, syms = rec[512:530].astype(np.int64), rec[530:548].astype(np.int64), rec[548:804]
    codes, k = {}, 0
    for length in range(1, 17):
        if maxcode[length] < 0:
            continue
        for c in range(int(k - valoff[length]), int(maxcode[length]) + 1):
            codes[(length, c)] = int(syms[k])
            k += 1
    return codes


class _Bits:
    def __init__(self, seg):
        self.bits = np.unpackbits(np.asarray(seg, np.uint8)).astype(np.int64)
        self.pos = 0
        self.n = len(self.bits)

    def get(self, n):
        if self.pos + n > self.n:
            raise CorruptData("segment ends inside a symbol")
        v = 0
        for b in self.bits[self.pos:self.pos + n]:
            v = (v << 1) | int(b)
        self.pos += n
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            if self.pos >= self.n:
                raise CorruptData("segment ends inside a code")
            code = (code << 1) | int(self.bits[self.pos])
            self.pos += 1
            s = table.get((length, code))
            if s is not None:
                return s
        raise CorruptData("bad Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def coefficients(r):
    """int16 coefficient blocks [bh, bw, 64] (natural order) of every component of a GPU record, decoded serially"""
    comps = r.comps
    tabs = {key: _tables(t) for key, t in r.huff.items()}
    grids = [np.zeros((r.mcuy * c.v, r.mcux * c.h, 64), np.int16) for c in comps]
    nmcu = r.mcux * r.mcuy
    per = r.restart if r.restart else nmcu
    layout = [(ci, dy, dx) for ci, c in enumerate(comps) for dy in range(c.v) for dx in range(c.h)]
    for s, seg in enumerate(r.segments):
        bits = _Bits(seg)
        pred = [0] * len(comps)
        for mcu in range(s * per, min((s + 1) * per, nmcu)):
            my, mx = divmod(mcu, r.mcux)
            for ci, dy, dx in layout:
                c = comps[ci]
                blk = np.zeros(64, np.int64)
                t = bits.symbol(tabs[(0, c.td)])
                diff = _extend(bits.get(t), t) if t else 0
                pred[ci] += diff
                blk[0] = pred[ci]
                k = 1
                while k < 64:
                    rs = bits.symbol(tabs[(1, c.ta)])
                    rr, ss = rs >> 4, rs & 15
                    if ss:
                        k += rr
                        blk[jpeg.NATURAL[min(k, 63)]] = _extend(bits.get(ss), ss)
                        k += 1
                    elif rr == 15:
                        k += 16
                    else:
                        break
                grids[ci][my * c.v + dy, mx * c.h + dx] = blk.astype(np.int16)
    return grids


def idct_limit(v):
    j = np.asarray(v, np.int64) & 1023
    return np.where(j < 128, j + 128, np.where(j < 512, 255, np.where(j < 896, 0, j - 896))).astype(np.uint8)


def _islow_1d(x, shift, out_fn):
    """x: int32 [..., 8] along the last axis -> [..., 8]; numpy int32 arithmetic wraps as the 32-bit C does"""
    i32 = np.int32
    x = x.astype(i32)
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * i32(F["F0_541"])
    tmp2 = z1 + z3 * i32(-F["F1_847"])
    tmp3 = z1 + z2 * i32(F["F0_765"])
    z2, z3 = x[..., 0], x[..., 4]
    t0 = (z2 + z3) * i32(1 << 13)
    t1 = (z2 - z3) * i32(1 << 13)
    tmp10, tmp13, tmp11, tmp12 = t0 + tmp3, t0 - tmp3, t1 + tmp2, t1 - tmp2
    o0, o1, o2, o3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * i32(F["F1_175"])
    o0, o1, o2, o3 = o0 * i32(F["F0_298"]), o1 * i32(F["F2_053"]), o2 * i32(F["F3_072"]), o3 * i32(F["F1_501"])
    z1, z2 = z1 * i32(-F["F0_899"]), z2 * i32(-F["F2_562"])
    z3, z4 = z3 * i32(-F["F1_961"]) + z5, z4 * i32(-F["F0_390"]) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    r = i32(1 << (shift - 1))
    outs = [tmp10 + o3, tmp11 + o2, tmp12 + o1, tmp13 + o0, tmp13 - o0, tmp12 - o1, tmp11 - o2, tmp10 - o3]
    return np.stack([out_fn((v + r) >> shift) for v in outs], axis=-1)


def idct_islow(coef, q):
    """coef int16 [..., 64] natural order, q int [64] -> uint8 [..., 8, 8]"""
    with np.errstate(over="ignore"):
        deq = (coef.astype(np.int32) * np.asarray(q, np.int32)).reshape(coef.shape[:-1] + (8, 8))
        ws = _islow_1d(np.swapaxes(deq, -1, -2), 11, lambda v: v)      # columns: [..., col, row-out]
        ws = np.swapaxes(ws, -1, -2)                                    # [..., row, col]
        return _islow_1d(ws, 18, idct_limit)


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = (np.asarray(a, np.int64) for a in (y, cb, cr))
    x, z = cr - 128, cb - 128
    r = y + ((91881 * x + 32768) >> 16)
    g = y + ((-22554 * z + 32768 - 46802 * x) >> 16)
    b = y + ((116130 * z + 32768) >> 16)
    return np.stack([np.clip(r, 0, 255), np.clip(g, 0, 255), np.clip(b, 0, 255)], axis=-1).astype(np.uint8)


def _far(n_out, n):
    o = np.arange(n_out)
    i = o >> 1
    return np.where(o & 1, np.minimum(i + 1, n - 1), np.maximum(i - 1, 0))


def upsample(plane, cw, ch, rh, rv, W, H):
    """libjpeg's upsampling of a downsampled plane (valid region cw x ch) to W x H (rh, rv in {1, 2}; not 4:4:0)"""
    p = plane[:ch, :cw].astype(np.int64)
    if rh == 1:
        return p[:H, :W]
    o = np.arange(W)
    if cw <= 2:  # jdsample.c: plain replication for rows of two samples or fewer
        rows = np.arange(H) >> (rv - 1)
        return p[rows][:, o >> 1]
    xn, xf = o >> 1, _far(W, cw)
    if rv == 1:
        return (3 * p[:H][:, xn] + p[:H][:, xf] + 1 + (o & 1)) >> 2
    yo = np.arange(H)
    s = 3 * p[yo >> 1] + p[_far(H, ch)]
    return (3 * s[:, xn] + s[:, xf] + 8 - (o & 1)) >> 4


def decode_record(r):
    """uint8 [H, W, 3] of a GPU record, restated"""
    grids = coefficients(r)
    planes = []
    for c, g in zip(r.comps, grids):
        px = idct_islow(g, r.quant[c.tq])  # [bh, bw, 8, 8]
        bh, bw = g.shape[:2]
        planes.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    Y = planes[0][:r.H, :r.W]
    if len(r.comps) == 1:
        return np.repeat(Y[:, :, None], 3, axis=2)
    chroma = []
    for c, p in zip(r.comps[1:], planes[1:]):
        cw, ch = -(-r.W * c.h // r.hmax), -(-r.H * c.v // r.vmax)
        chroma.append(upsample(p, cw, ch, r.hmax // c.h, r.vmax // c.v, r.W, r.H))
    return ycc_to_rgb(Y, chroma[0], chroma[1])


def decode(data):
    """the restatement's decode of one file (GPU-path inputs only); raises CorruptData where the GPU would set its status"""
    r = jpeg.parse(data)
    if not r.gpu:
        raise ValueError("not a GPU-path input: %s" % r.reason)
    return decode_record(r)
