"""The JPEG decoder without a GPU: the numpy restatement (tests/jpeg_ref.py) against Pillow's decodes (fixtures and live), the
parser's records and fallback verdicts (one per colour-space / format rule), jpeg_math.h compiled with g++ against the restatement,
the worker-side collate, and the C ABI's new export and workspace question."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from tests import jpeg_ref as R
from esvit_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz")


def _fixtures():
    z = np.load(GOLD)
    return {k[:-5]: (z[k].tobytes(), str(z[k[:-5] + ".kind"]), z[k[:-5] + ".rgb"] if k[:-5] + ".rgb" in z.files else None,
                     z[k[:-5] + ".sha"].tobytes().hex() if k[:-5] + ".sha" in z.files else None) for k in z.files if k.endswith(".file")}


FIX = _fixtures()


@pytest.mark.parametrize("name", sorted(n for n, f in FIX.items() if f[1] == "gpu" and n != "big_2000x1500"))
def test_restatement_decodes_every_fixture_bit_exactly(name):
    data, _, rgb, sha = FIX[name]
    got = R.decode(data)
    if rgb is not None:
        assert np.array_equal(got, rgb)
    else:
        assert jpeg.sha256(got) == sha


def test_fixture_verdicts():
    for name, (data, kind, _, _) in FIX.items():
        r = jpeg.parse(data)
        assert r.gpu == (kind in ("gpu", "corrupt")), (name, r)
        if kind == "truncated":
            assert r.truncated
    with pytest.raises(R.CorruptData):
        R.decode(FIX["corrupt"][0])


def _img(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x * 7 + y * 3) % 256], -1) + rng.integers(-50, 50, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def test_restatement_matches_live_pillow_on_random_small_cases():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for case in range(300):
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        a = _img(rng, h, w)
        kw = dict(quality=int(rng.integers(1, 101)), optimize=bool(rng.integers(0, 2)))
        gray = rng.random() < 0.2
        if not gray:
            kw["subsampling"] = int(rng.integers(0, 3))
        if rng.random() < 0.3:
            kw["restart_marker_blocks"] = int(rng.integers(1, 6))
        b = io.BytesIO()
        Image.fromarray(a[:, :, 0] if gray else a).save(b, "JPEG", **kw)
        want = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))
        assert np.array_equal(R.decode(b.getvalue()), want), (case, h, w, kw, gray)


# ---- parser: records and one test per fallback rule ---------------------------------------------------------------------------
def _jfif(sub=2, **kw):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(_img(np.random.default_rng(1), 24, 40)).save(b, "JPEG", subsampling=sub, **kw)
    return b.getvalue()


def _markers(d):
    i, out = 2, []
    while d[i + 1] != 0xDA:
        L = (d[i + 2] << 8) | d[i + 3]
        out.append((d[i + 1], i, L))
        i += 2 + L
    out.append((0xDA, i, (d[i + 2] << 8) | d[i + 3]))
    return out


def _sof(d):
    return next(i for m, i, _ in _markers(d) if m in (0xC0, 0xC1))


def _without_app0(d):
    m = next((i, L) for mk, i, L in _markers(d) if mk == 0xE0)
    return d[:m[0]] + d[m[0] + 2 + m[1]:]


def _with_adobe(d, transform):
    app14 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])
    return d[:2] + app14 + d[2:]


def _patch(d, at, value):
    return d[:at] + bytes([value]) + d[at + 1:]


def test_record_of_a_baseline_file():
    d = _jfif(sub=2, restart_marker_blocks=2)
    r = jpeg.parse(d)
    assert r.gpu and (r.H, r.W) == (24, 40) and (r.hmax, r.vmax) == (2, 2) and (r.mcux, r.mcuy) == (3, 2)
    assert [(c.h, c.v) for c in r.comps] == [(2, 2), (1, 1), (1, 1)]
    assert r.restart == 2 and len(r.segments) == 3
    assert all(s.dtype == np.uint8 for s in r.segments)
    q = r.quant[r.comps[0].tq]
    assert q.shape == (64,) and q.dtype == np.int32
    assert jpeg.parse(_jfif(sub=0)).comps[0][1:3] == (1, 1)
    assert [(c.h, c.v) for c in jpeg.parse(_jfif(sub=1)).comps] == [(2, 1), (1, 1), (1, 1)]


def test_huffman_record_of_the_standard_dc_luminance_table():
    counts = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]  # T.81 Table K.3
    rec = jpeg.huffman_record(counts, list(range(12)), is_dc=True)
    assert rec[0b00 << 7] == (2 << 8) | 0 and rec[0b010 << 6] == (3 << 8) | 1 and rec[0b110 << 6] == (3 << 8) | 5
    assert rec[0b1110 << 5] == (4 << 8) | 6 and rec[0b111111110] == (9 << 8) | 11 and rec[511] == 0
    assert rec[512 + 9] == 0b111111110 and rec[512 + 10] == -1 and rec[512 + 17] == 0x7FFFFFFF
    with pytest.raises(jpeg._Fallback):  # an all-ones code of length 1
        jpeg.huffman_record([2] + [0] * 15, [0, 1], is_dc=True)
    with pytest.raises(jpeg._Fallback):  # libjpeg rejects DC categories above 15
        jpeg.huffman_record([1] + [0] * 15, [16], is_dc=True)


def test_sixteen_bit_quantisation_tables_take_the_gpu():
    d = _jfif(qtables=[list(range(250, 314)), list(range(300, 364))])
    assert d[_sof(d) + 1] == 0xC1
    r = jpeg.parse(d)
    assert r.gpu and r.quant[0].max() == 313 and r.quant[0][0] == 250


def test_fallback_progressive():
    assert jpeg.parse(_jfif(progressive=True)).reason == "progressive"


def test_fallback_arithmetic():
    d = _jfif()
    assert jpeg.parse(_patch(d, _sof(d) + 1, 0xC9)).reason == "arithmetic"


def test_fallback_12_bit():
    d = _jfif()
    assert jpeg.parse(_patch(d, _sof(d) + 4, 12)).reason == "12-bit samples"


def test_fallback_cmyk():
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(_img(np.random.default_rng(2), 16, 16)).convert("CMYK").save(b, "JPEG")
    assert jpeg.parse(b.getvalue()).reason == "4 components"


def test_colour_space_rules():
    d = _jfif()
    s = _sof(d)
    rgb_ids = _patch(_patch(_patch(d, s + 10, 82), s + 13, 71), s + 16, 66)
    sos = next(i for m, i, _ in _markers(rgb_ids) if m == 0xDA)
    rgb_ids = _patch(_patch(_patch(rgb_ids, sos + 5, 82), sos + 7, 71), sos + 9, 66)
    assert jpeg.parse(rgb_ids).gpu  # JFIF says YCbCr whatever the ids
    assert jpeg.parse(_without_app0(rgb_ids)).reason == "RGB colour space"  # no JFIF, no Adobe: ids 'R','G','B' mean RGB
    assert jpeg.parse(_without_app0(d)).gpu  # ids 1, 2, 3: YCbCr
    assert jpeg.parse(_with_adobe(_without_app0(d), 0)).reason == "RGB colour space"  # Adobe transform 0: RGB
    assert jpeg.parse(_with_adobe(_without_app0(d), 1)).gpu  # transform 1: YCbCr
    assert jpeg.parse(_with_adobe(_without_app0(rgb_ids), 1)).gpu  # Adobe decides before the ids


def test_fallback_sampling_factors():
    d = _jfif(sub=0)
    s = _sof(d)
    assert jpeg.parse(_patch(d, s + 11, 0x12)).reason.startswith("sampling")  # 4:4:0
    assert jpeg.parse(_patch(d, s + 11, 0x41)).reason.startswith("sampling")  # 4:1:1
    assert jpeg.parse(_patch(d, s + 11, 0x22)).gpu  # 4:2:0 header


def test_fallback_multi_scan_and_non_jpeg():
    d = _jfif()
    sos = next(i for m, i, _ in _markers(d) if m == 0xDA)
    second = d[sos:-2]
    assert jpeg.parse(d[:-2] + second + b"\xff\xd9").reason == "multi-scan"
    assert jpeg.parse(b"\x89PNG\r\n\x1a\n" + bytes(40)).reason == "not a JPEG file"
    assert jpeg.parse(FIX["png"][0]).reason == "not a JPEG file"


def test_truncated_and_restart_sequence():
    d = _jfif(restart_marker_blocks=1)
    r = jpeg.parse(d[:len(d) * 2 // 3])
    assert not r.gpu and r.truncated
    i = d.index(b"\xff\xd1")
    assert jpeg.parse(d[:i + 1] + b"\xd3" + d[i + 2:]).reason == "restart markers out of sequence"


def test_prepare_does_not_touch_the_gpu():
    import sys
    b = jpeg.prepare([FIX["m420_q75"][0], FIX["s7x9_420_q100"][0]])
    assert b.n_segments == 2 and b.n_lanes >= 2
    assert b.host.dtype == np.uint8 and b.out_bytes == int((b.H * b.W * 3).sum()) + 4
    # in a fresh process (a forked DataLoader worker's view): the worker half initialises no device
    code = ("import sys, torch; sys.path.insert(0, %r); from esvit_amd import jpeg; import numpy as np; "
            "z = np.load(%r); jpeg.prepare([z['m420_q75.file'].tobytes()]); assert not torch.cuda.is_initialized()" % (ROOT, GOLD))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


# ---- jpeg_math.h on the host --------------------------------------------------------------------------------------------------
SHIM = r'''
#define JPG_HD inline
#include "jpeg_math.h"
extern "C" {
void idct(const int16_t* coef, const int32_t* q, uint8_t* out, int n) { for (int i = 0; i < n; ++i) jpg::idct_islow(coef + 64 * i, q + 64 * i, out + 64 * i, 8); }
void ycc(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint8_t* rgb, long n) { for (long i = 0; i < n; ++i) jpg::ycc_to_rgb(y[i], cb[i], cr[i], rgb + 3 * i); }
void up(const uint8_t* p, int pitch, int cw, int ch, int rh, int rv, int W, int H, int32_t* out) {
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) out[y * W + x] = jpg::chroma(p, pitch, cw, ch, rh, rv, x, y); }
}
'''


@pytest.fixture(scope="module")
def host_math(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_math")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "esvit_amd", "csrc"), str(src), "-o", str(so)],
                   check=True)
    return C.CDLL(str(so))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_header_idct_equals_restatement(host_math):
    rng = np.random.default_rng(0)
    n = 4000
    coef = np.zeros((n, 64), np.int16)
    q = rng.integers(1, 256, (n, 64)).astype(np.int32)
    # random sparse blocks, full random blocks, and extreme ones (|dequantised| up to 2^15: the range limit wraps)
    coef[:1000] = rng.integers(-60, 61, (1000, 64)) * (rng.random((1000, 64)) < 0.2)
    coef[1000:2000] = rng.integers(-200, 201, (1000, 64))
    coef[2000:3000, 0] = rng.integers(-2048, 2048, 1000)
    coef[3000:] = rng.choice([-1024, -1023, -512, 511, 512, 1023], (1000, 64))
    q[3000:] = rng.integers(1, 32, (1000, 64))
    out = np.zeros((n, 64), np.uint8)
    host_math.idct(_p(coef), _p(q), _p(out), C.c_int(n))
    want = np.stack([R.idct_islow(coef[i], q[i]).reshape(64) for i in range(n)])
    assert np.array_equal(out, want)
    assert (want == 0).any() and (want == 255).any()


def test_header_colour_conversion_on_all_triples(host_math):
    v = np.arange(1 << 24, dtype=np.int64)
    y, cb, cr = (v >> 16).astype(np.uint8), ((v >> 8) & 255).astype(np.uint8), (v & 255).astype(np.uint8)
    out = np.zeros((1 << 24, 3), np.uint8)
    host_math.ycc(_p(y), _p(cb), _p(cr), _p(out), C.c_long(1 << 24))
    assert np.array_equal(out, R.ycc_to_rgb(y, cb, cr))


def test_header_upsampling_rows_at_edges(host_math):
    rng = np.random.default_rng(1)
    for cw, ch, rh, rv in [(1, 1, 2, 2), (2, 3, 2, 2), (3, 1, 2, 2), (3, 3, 2, 1), (5, 4, 2, 2), (9, 7, 2, 1), (4, 4, 1, 1), (17, 9, 2, 2)]:
        pitch = cw + 7
        plane = rng.integers(0, 256, (ch + 1, pitch), dtype=np.uint8)
        for W in (2 * cw - 1, 2 * cw) if rh == 2 else (cw,):
            H = 2 * ch - 1 if rv == 2 else ch
            out = np.zeros((H, W), np.int32)
            host_math.up(_p(plane), pitch, cw, ch, rh, rv, W, H, _p(out))
            assert np.array_equal(out, R.upsample(plane, cw, ch, rh, rv, W, H)), (cw, ch, rh, rv, W)


# ---- worker collate, the C ABI ------------------------------------------------------------------------------------------------
def test_collate_encoded_makes_the_draws_of_collate(lib_built):
    from esvit_amd import data as D
    names = ["m420_q75", "s17x33_444_q100", "mgray_q85", "sof1_qt16"]
    enc = [(FIX[n][0], i) for i, n in enumerate(names)]
    dec = [(R.decode(FIX[n][0]), i) for i, n in enumerate(names)]
    a = D.DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), (8,), (96,), seed=5)
    b = D.DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), (8,), (96,), seed=5)
    (batch, da), ya = a.collate_encoded(enc)
    (_, db), yb = b.collate(dec)
    assert isinstance(batch, jpeg.Batch) and ya.tolist() == yb.tolist()
    assert da.keys() == db.keys()
    for S in da:
        assert np.array_equal(da[S][0], db[S][0]) and da[S][1:] == db[S][1:]


def test_jpeg_export_and_workspace_question(lib_built):
    from esvit_amd import ops
    from esvit_amd._lib import JpegDesc, lib
    ws = ops.query(ops.Q_JPEG_WORKSPACE, 1000, 70000, 50 | (3 << 32))
    assert ws >= 1000 * 128 + 70000 + 2 * 50 * 48 + 50 * 16 + 3 * 4
    assert ops.query(ops.Q_JPEG_WORKSPACE, 2000, 70000, 50 | (3 << 32)) == ws + 1000 * 128
    b = jpeg.prepare([FIX["m420_q75"][0]])
    assert jpeg.workspace_bytes(b) >= b.n_blocks * 128 + b.plane_bytes
    bad = JpegDesc(n_images=1, mode=7)
    assert lib.esvit_jpeg_decode(C.byref(bad), None, 0, None) == -1  # argument checks need no device
    assert b"esvit_jpeg_decode" in lib.esvit_last_error()
