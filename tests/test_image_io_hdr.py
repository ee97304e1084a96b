"""The HDR readers of the CLI's image I/O (host/image_io.cpp: imreadHDR), host only, in a stand-alone program built with
ASan + UBSan like tests/test_image_io16.py builds its own.  Radiance pictures are crafted by a small RGBE writer here (flat
and run-length scanlines, runs and literals mixed, exponent 0) and PFM files with struct; every decoded float must be
bit-equal to this file's own decode (mantissa m, exponent e: m 2^(e - 136), e = 0 gives 0; PFM: the file's floats, rows
bottom to top).  Damaged files -- truncated at every header line and inside a run, a run past the scanline's end, a wrong
resolution line, dimensions whose product overflows -- must each be refused (an empty image) or decoded, with no sanitizer
finding either way: the program's exit status is 0 only when neither sanitizer reported."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "nonlocal-image-edit_amd", "host", "image_io.cpp")
SRC_JPEG = os.path.join(ROOT, "nonlocal-image-edit_amd", "host", "jpeg.cpp")
MAIN = r"""
#include <cstdio>
#include "nle/image_io.hpp"
int main(int argc, char** argv) {
    if (argc < 3) return 6;
    const nle::Image im = nle::imreadHDR(argv[1]);
    if (im.empty()) { std::puts("EMPTY"); return 0; }
    if (im.channels() != 3 || im.depth() != nle::NLE_32F) return 4;
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 5;
    const int hdr[2] = {im.rows, im.cols};
    std::fwrite(hdr, sizeof(int), 2, f);
    std::fwrite(im.ptr<float>(), 4, im.total() * 3, f);
    std::fclose(f);
    return 0;
}
"""

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("imgiohdr")
    (d / "main.cpp").write_text(MAIN)
    exe = d / "imgiohdr"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "include"), str(d / "main.cpp"), SRC, SRC_JPEG, "-o", str(exe)], check=True)
    return str(exe)


def read(tool, tmp_path, data, name="f.hdr"):
    """the (H, W, 3) float32 BGR image imreadHDR makes of these bytes, or None for an empty one; any sanitizer finding fails"""
    src, dump = tmp_path / name, tmp_path / "dump"
    src.write_bytes(data)
    r = subprocess.run([tool, str(src), str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
    if "EMPTY" in r.stdout:
        return None
    b = open(dump, "rb").read()
    rows, cols = struct.unpack("ii", b[:8])
    return np.frombuffer(b[8:], dtype=np.float32).reshape(rows, cols, 3)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ Radiance
def decode_rgbe(rgbe):
    """this file's own decode of (H, W, 4) uint8 R, G, B, E: float32 BGR"""
    e = rgbe[..., 3].astype(np.int32)
    m = rgbe[..., 2::-1].astype(np.float32)
    v = np.ldexp(m, (e - 136)[..., None]).astype(np.float32)
    return np.where((e == 0)[..., None], np.float32(0), v)


def rle_component(row):
    """one component's bytes of a scanline in runs (>= 3 equal bytes, at most 127) and literals (at most 128)"""
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        j = i
        while j < n and j - i < 127 and row[j] == row[i]:
            j += 1
        if j - i >= 3:
            out += bytes([128 + (j - i), row[i]])
            i = j
            continue
        k = i
        while k < n and k - i < 128 and not (k + 2 < n and row[k] == row[k + 1] == row[k + 2]):
            k += 1
        out += bytes([k - i]) + bytes(row[i:k])
        i = k
    return bytes(out)


def header(h, w, magic=b"#?RADIANCE", lines=(b"FORMAT=32-bit_rle_rgbe",), res=None):
    return magic + b"\n" + b"".join(ln + b"\n" for ln in lines) + b"\n" + (res if res is not None else b"-Y %d +X %d" % (h, w)) + b"\n"


def radiance(rgbe, rle, **kw):
    h, w, _ = rgbe.shape
    body = bytearray()
    for r in range(h):
        if rle:
            body += bytes([2, 2, w >> 8, w & 255]) + b"".join(rle_component(rgbe[r, :, k].tolist()) for k in range(4))
        else:
            body += rgbe[r].tobytes()
    return header(h, w, **kw) + bytes(body)


def picture(h, w, seed):
    """random mantissas and exponents with constant stretches (runs), exponent 0 and both ends of the exponent range"""
    rng = np.random.default_rng(seed)
    rgbe = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    rgbe[..., 3] = rng.integers(100, 160, (h, w), dtype=np.uint8)
    for r in range(h):                                   # stretches of equal bytes, per component, of mixed lengths
        x = 0
        while x < w:
            n = int(rng.integers(1, 40))
            if rng.random() < 0.5:
                rgbe[r, x:x + n, int(rng.integers(0, 4))] = rng.integers(0, 256)
            x += n
    flat = rgbe.reshape(-1, 4)
    for i, e in enumerate((0, 1, 255, 0, 136)):          # e = 0 (with non-zero mantissas), the smallest and the largest exponent
        flat[(i * 7) % len(flat), 3] = e
    rgbe[:, 0, 0] = 77                                   # a flat scanline must not begin like a run-length one (2, 2, w)
    return rgbe


@pytest.mark.parametrize("w", [1, 7, 8, 127, 128, 300, 32768, 40000])
def test_flat_scanlines_decode_bit_for_bit(tool, tmp_path, w):
    rgbe = picture(3 if w < 1000 else 1, w, w)
    got = read(tool, tmp_path, radiance(rgbe, rle=False))
    assert got is not None and same_bits(got, decode_rgbe(rgbe))


@pytest.mark.parametrize("w", [8, 127, 128, 129, 300, 32767])
def test_run_length_scanlines_decode_bit_for_bit(tool, tmp_path, w):
    rgbe = picture(3 if w < 1000 else 1, w, 1000 + w)
    data = radiance(rgbe, rle=True)
    body = data[len(header(rgbe.shape[0], w)):]
    assert body[:4] == bytes([2, 2, w >> 8, w & 255]) and any(b > 130 for b in body[4:])     # the run-length form, with runs
    got = read(tool, tmp_path, data)
    assert got is not None and same_bits(got, decode_rgbe(rgbe))


def test_mixed_scanlines_the_other_magic_and_ignored_variables(tool, tmp_path):
    """a flat and a run-length scanline in one file, `#?RGBE`, EXPOSURE and unknown variables ignored; e = 0 decodes to 0
    whatever the mantissas are"""
    rgbe = picture(4, 64, 5)
    rgbe[1, 3] = (200, 100, 50, 0)
    h, w, _ = rgbe.shape
    body = b""
    for r in range(h):
        if r % 2:
            body += rgbe[r].tobytes()
        else:
            body += bytes([2, 2, 0, w]) + b"".join(rle_component(rgbe[r, :, k].tolist()) for k in range(4))
    head = header(h, w, magic=b"#?RGBE", lines=(b"# a comment", b"EXPOSURE=4.0", b"FORMAT=32-bit_rle_rgbe", b"SOFTWARE=x"))
    got = read(tool, tmp_path, head + body)
    want = decode_rgbe(rgbe)
    assert got is not None and same_bits(got, want) and np.all(got[1, 3] == 0)


def test_damaged_radiance_files_are_refused(tool, tmp_path):
    rgbe = picture(2, 64, 9)
    rgbe[0, 10:60, 1] = 33                                     # a long run in G of the first scanline
    good = radiance(rgbe, rle=True)
    head = header(2, 64)
    assert read(tool, tmp_path, good) is not None
    bad = {}
    pos = 0
    for i in range(head.count(b"\n")):                         # truncated at the end of every header line, and inside it
        pos = head.index(b"\n", pos) + 1
        bad[f"header-line-{i}"] = good[:pos]
        bad[f"header-line-{i}-inside"] = good[:pos - 2]
    body = good[len(head):]
    mark = bytes([2, 2, 0, 64])
    bad["inside-a-run"] = head + mark + bytes([128 + 60])                    # the run's value byte is missing
    bad["inside-a-literal"] = good[:len(head) + 6]
    bad["after-the-first-scanline-marker"] = good[:len(head) + 4]
    bad["second-scanline-missing"] = head + mark + b"".join(rle_component([5] * 64) for _ in range(4))
    bad["run-overruns"] = head + mark + bytes([128 + 60, 7, 128 + 10, 7]) + bytes(4000)      # 70 > 64
    bad["run-overruns-by-one"] = head + mark + bytes([128 + 64, 7]) * 3 + bytes([128 + 63, 7, 128 + 2, 7]) + bytes(4000)
    bad["literal-overruns"] = head + bytes([2, 2, 0, 64]) + bytes([60]) + bytes(60) + bytes([100]) + bytes(4000)
    bad["zero-count"] = head + bytes([2, 2, 0, 64, 0]) + bytes(4000)
    flat = rgbe.tobytes()
    for name, res in [("plus-y", b"+Y 2 +X 64"), ("minus-x", b"-Y 2 -X 64"), ("x-first", b"+X 64 -Y 2"), ("no-width", b"-Y 2 +X"),
                      ("zero", b"-Y 0 +X 64"), ("trailing", b"-Y 2 +X 64 "), ("too-tall", b"-Y 70000 +X 64"),
                      ("too-wide", b"-Y 2 +X 65536"), ("negative", b"-Y -2 +X 64"), ("empty", b""), ("words", b"-Y two +X 64"),
                      ("overflow-32", b"-Y 4294967298 +X 64"), ("overflow-64", b"-Y 18446744073709551618 +X 64"),
                      ("overflow-long", b"-Y 2 +X " + b"9" * 400)]:
        bad["resolution-" + name] = header(2, 64, res=res) + flat
    bad["product-overflows"] = header(65535, 65535) + flat     # 2^32 pixels promised, 128 given
    bad["product-overflows-rle"] = header(65535, 32767) + good[len(head):]
    bad["no-format"] = header(2, 64, lines=()) + flat
    bad["other-format"] = header(2, 64, lines=(b"FORMAT=32-bit_rle_xyze",)) + flat
    bad["other-magic"] = header(2, 64, magic=b"#?RADIANCE2") + flat
    bad["no-blank-line"] = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n-Y 2 +X 64\n" + flat
    bad["flat-one-byte-short"] = head + flat[:-1]
    bad["just-the-magic"] = b"#?"
    for name, data in bad.items():
        assert read(tool, tmp_path, data) is None, name
    # whatever else a cut leaves: refused or decoded, never a finding
    for cut in range(len(head), len(good), 7):
        read(tool, tmp_path, good[:cut])


# ------------------------------------------------------------------------------------------------ PFM
def pfm(img, little, grey=False, scale=1.0, head=None):
    """a PFM of an (H, W, 3) RGB or (H, W) grey float32 array: rows bottom to top"""
    h, w = img.shape[:2]
    hdr = head if head is not None else b"%s\n%d %d\n%s\n" % (b"Pf" if grey else b"PF", w, h, repr(-scale if little else scale).encode())
    return hdr + img[::-1].astype("<f4" if little else ">f4").tobytes()


@pytest.mark.parametrize("little", [True, False], ids=["little", "big"])
@pytest.mark.parametrize("grey", [False, True], ids=["PF", "Pf"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 2), (37, 53)])
def test_pfm_decodes_bit_for_bit(tool, tmp_path, little, grey, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    img = np.exp2(rng.uniform(-20, 20, shape if grey else shape + (3,))).astype(np.float32)
    img.reshape(-1)[:: 5] *= -1
    img.reshape(-1)[0] = np.float32("nan") if grey else np.float32("inf")          # every bit pattern passes through
    got = read(tool, tmp_path, pfm(img, little, grey, scale=2.5), "f.pfm")
    want = np.repeat(img[..., None], 3, axis=2) if grey else img[..., ::-1]
    assert got is not None and same_bits(got, want)


def test_pfm_rows_run_bottom_to_top(tool, tmp_path):
    """a ramp whose value names its row and column: the file's first row is the image's last"""
    h, w = 5, 4
    y, x = np.mgrid[0:h, 0:w]
    ramp = (100 * y + x).astype(np.float32)
    data = b"Pf\n4 5\n-1.0\n" + b"".join(struct.pack("<4f", *ramp[r]) for r in range(h - 1, -1, -1))
    got = read(tool, tmp_path, data, "f.pfm")
    assert got is not None and np.array_equal(got[..., 0], ramp) and got[0, 0, 0] == 0 and got[4, 3, 2] == 403


def test_damaged_pfm_files_are_refused(tool, tmp_path):
    img = np.arange(3 * 5 * 3, dtype=np.float32).reshape(3, 5, 3)
    good = pfm(img, True)
    assert read(tool, tmp_path, good, "f.pfm") is not None
    data = img.tobytes()
    bad = {"one-byte-short": good[:-1], "header-only": good[:len(good) - len(data)], "half": good[:len(good) // 2],
           "just-the-magic": b"PF", "magic-and-newline": b"PF\n", "no-height": b"PF\n5\n", "no-scale": b"PF\n5 3\n",
           "scale-at-the-end": b"PF\n5 3\n-1.0", "zero-scale": pfm(img, True, head=b"PF\n5 3\n0.0\n"),
           "nan-scale": pfm(img, True, head=b"PF\n5 3\nnan\n"), "word-scale": pfm(img, True, head=b"PF\n5 3\nlittle\n"),
           "zero-width": pfm(img, True, head=b"PF\n0 3\n-1.0\n"), "negative": pfm(img, True, head=b"PF\n-5 3\n-1.0\n"),
           "too-wide": pfm(img, True, head=b"PF\n65536 1\n-1.0\n"), "product-overflows": pfm(img, True, head=b"PF\n65535 65535\n-1.0\n"),
           "overflow-64": pfm(img, True, head=b"PF\n18446744073709551621 3\n-1.0\n"),
           "long-token": pfm(img, True, head=b"PF\n" + b"5" * 500 + b" 3\n-1.0\n"), "glued-magic": pfm(img, True, head=b"PF5 3\n-1.0\n"),
           "other-magic": pfm(img, True, head=b"PG\n5 3\n-1.0\n")}
    for name, d in bad.items():
        assert read(tool, tmp_path, d, "f.pfm") is None, name
    for cut in range(0, len(good), 5):
        read(tool, tmp_path, good[:cut] if cut else b"P", "f.pfm")


def test_other_files_are_not_hdr(tool, tmp_path):
    from conftest import GOLDEN
    assert read(tool, tmp_path, open(os.path.join(GOLDEN, "flower-50.bmp"), "rb").read(), "f.bmp") is None
    src = tmp_path / "missing.hdr"
    r = subprocess.run([tool, str(src), str(tmp_path / "dump")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "EMPTY" in r.stdout
