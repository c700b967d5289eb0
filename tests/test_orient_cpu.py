"""Orientation, host side (no GPU): jb_oriented_size and the rectangle mapper against numpy's T_o exhaustively on 7 x 5,
jb_exif_orientation on hand-built byte strings (and against Pillow where it imports), the plan's refusals through
jb_orient_check, the setters' null statuses, and the two stand-alone sanitizer programs of tools/fuzz."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import orient_ref as ot
from conftest import ROOT


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    return jb


# ---- sizes and rectangles ----------------------------------------------------------------------------------------------
def test_oriented_size(jb):
    for o in range(1, 9):
        assert jb.oriented_size(7, 5, o) == ot.size(7, 5, o) == ot.orient(np.zeros((5, 7, 1)), o).shape[1::-1]
    for bad in (0, 9, -1):
        with pytest.raises(jb.JbError) as e:
            jb.oriented_size(7, 5, bad)
        assert e.value.status == -2
    for w, h in ((0, 5), (7, 65536)):
        with pytest.raises(jb.JbError) as e:
            jb.oriented_size(w, h, 6)
        assert e.value.status == -2
    v = ctypes.c_int32()
    assert jb.lib().jb_oriented_size(7, 5, 6, None, ctypes.byref(v)) == -1


@pytest.mark.parametrize("o", range(1, 9))
def test_every_rectangle_maps_back(jb, o):
    """T_o(a)[y:y+h, x:x+w] == T_o(a[the mapped stored rectangle]) for every rectangle of the oriented 7 x 5 frame."""
    W, H = 7, 5
    a = np.arange(W * H).reshape(H, W, 1)
    t = ot.orient(a, o)
    ow, oh = ot.size(W, H, o)
    n = 0
    for x in range(ow):
        for y in range(oh):
            for w in range(1, ow - x + 1):
                for h in range(1, oh - y + 1):
                    sx, sy, sw, sh = jb.orient_map_roi(W, H, o, (x, y, w, h))
                    assert 0 <= sx and 0 <= sy and sx + sw <= W and sy + sh <= H
                    assert np.array_equal(t[y:y + h, x:x + w], ot.orient(a[sy:sy + sh, sx:sx + sw], o)), (o, x, y, w, h)
                    n += 1
    assert n == (W * (W + 1) // 2) * (H * (H + 1) // 2)
    for bad in ((ow, 0, 1, 1), (0, 0, ow + 1, 1), (0, 0, 1, oh + 1), (-1, 0, 1, 1), (0, 0, 0, 1), (2 ** 31 - 1, 0, 2, 1)):
        with pytest.raises(jb.JbError) as e:
            jb.orient_map_roi(W, H, o, bad)
        assert e.value.status == -2


# ---- the Exif parser -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [False, True])
def test_exif_values(jb, big):
    for v in range(10):
        f = ot.tiny_jpeg(ot.exif_app1(v, big))
        assert jb.exif_orientation(f) == (v if 1 <= v <= 8 else 1), (v, big)


def test_exif_everything_else_is_1(jb):
    big = False
    cases = {"no segment": ot.tiny_jpeg(),
             "tag absent": ot.tiny_jpeg(ot.exif_app1(6, with_tag=False)),
             "type LONG": ot.tiny_jpeg(ot.exif_app1(6, typ=4)),
             "count 2": ot.tiny_jpeg(ot.exif_app1(6, count=2)),
             "IFD offset beyond the segment": ot.tiny_jpeg(ot.app1(b"Exif\0\0" + b"II" + b"\x2a\x00" + (4096).to_bytes(4, "little") + b"\0" * 40)),
             "IFD offset at the segment's last byte": ot.tiny_jpeg(ot.app1(b"Exif\0\0" + b"II" + b"\x2a\x00" + (47).to_bytes(4, "little") + b"\0" * 40)),
             "entries beyond the segment": ot.tiny_jpeg(ot.app1(b"Exif\0\0" + b"II" + b"\x2a\x00" + (8).to_bytes(4, "little") + b"\xff\xff" + b"\0" * 11)),
             "not 42": ot.tiny_jpeg(ot.app1(b"Exif\0\0" + b"II" + b"\x2b\x00" + ot.tiff([(0x0112, 3, 1, 6)], big)[4:])),
             "not II or MM": ot.tiny_jpeg(ot.app1(b"Exif\0\0" + b"IM" + ot.tiff([(0x0112, 3, 1, 6)], big)[2:])),
             "Exif behind SOS": ot.tiny_jpeg() + ot.exif_app1(6),
             "segment longer than the file": ot.tiny_jpeg(ot.exif_app1(6))[:30]}
    for name, f in cases.items():
        assert jb.exif_orientation(f) == 1, name
    # an IFD that does not start at 8, and the tag as the only entry
    assert jb.exif_orientation(ot.tiny_jpeg(ot.app1(b"Exif\0\0" + ot.tiff([(0x0112, 3, 1, 8)], ifd_offset=20)))) == 8
    # XMP in front (an APP1 that is not Exif) is walked over, and its own tiff:Orientation is out of scope
    assert jb.exif_orientation(ot.tiny_jpeg(ot.XMP + ot.exif_app1(3))) == 3
    assert jb.exif_orientation(ot.tiny_jpeg(ot.XMP)) == 1
    assert jb.exif_orientation(ot.tiny_jpeg(ot.APP0 + ot.exif_app1(5, True))) == 5
    # the FIRST Exif segment decides
    assert jb.exif_orientation(ot.tiny_jpeg(ot.exif_app1(2) + ot.exif_app1(7))) == 2
    assert jb.exif_orientation(ot.tiny_jpeg(ot.exif_app1(9) + ot.exif_app1(7))) == 1


def test_exif_prefixes_and_statuses(jb):
    f = ot.tiny_jpeg(ot.APP0 + ot.exif_app1(6))
    whole = f.index(b"\xff\xdb")          # the first byte behind the Exif segment
    for n in range(2, len(f) + 1):
        assert jb.exif_orientation(f[:n]) == (6 if n >= whole else 1), n
    for bad in (b"", b"\xff", b"\xff\xd9\xff\xd8", b"\x00" * 16, f[1:]):
        with pytest.raises(jb.JbError) as e:
            jb.exif_orientation(bad)
        assert e.value.status == -8
    o = ctypes.c_int(5)
    buf = np.frombuffer(f, np.uint8)
    assert jb.lib().jb_exif_orientation(None, 10, ctypes.byref(o)) == -1
    assert jb.lib().jb_exif_orientation(buf.ctypes.data_as(ctypes.c_void_p), buf.size, None) == -1


def test_exif_equals_pillow(jb):
    Image = pytest.importorskip("PIL.Image")
    img = Image.fromarray(np.arange(24 * 16 * 3, dtype=np.uint8).reshape(16, 24, 3))
    for v in range(10):
        ex = Image.Exif()
        ex[0x0112] = v
        b = io.BytesIO()
        img.save(b, "JPEG", exif=ex)
        want = Image.open(io.BytesIO(b.getvalue())).getexif().get(0x0112, 1)
        assert jb.exif_orientation(b.getvalue()) == (want if 1 <= want <= 8 else 1), v
    b = io.BytesIO()
    img.save(b, "JPEG")
    assert jb.exif_orientation(b.getvalue()) == 1


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_plan_refusals(jb):
    L = jb.lib()
    d = jb.make_desc(7, 5, 1, 1)
    roi = jb.Roi(5, 0, 2, 5)                      # lies in the stored 7 x 5 frame, not in the oriented 5 x 7 one
    assert L.jb_orient_check(ctypes.byref(d), 1, 1, ctypes.byref(roi)) == 0
    assert L.jb_orient_check(ctypes.byref(d), 6, 1, ctypes.byref(roi)) == -2
    assert L.jb_orient_check(ctypes.byref(d), 6, 1, ctypes.byref(jb.Roi(0, 5, 5, 2))) == 0   # and the other way round
    assert L.jb_orient_check(ctypes.byref(d), 1, 1, ctypes.byref(jb.Roi(0, 5, 5, 2))) == -2
    assert L.jb_orient_check(ctypes.byref(d), 3, 2, None) == -9
    assert L.jb_orient_check(ctypes.byref(d), 1, 2, None) == 0
    assert L.jb_orient_check(ctypes.byref(d), 3, 1, None) == 0
    assert L.jb_orient_check(ctypes.byref(d), 9, 1, None) == -2
    assert L.jb_orient_check(ctypes.byref(d), -1, 1, None) == -2
    assert L.jb_orient_check(ctypes.byref(d), 3, 3, None) == -2   # (the scale's own error comes first)
    assert L.jb_orient_check(None, 3, 1, None) == -1


def test_setters_on_null(jb):
    L = jb.lib()
    assert L.jb_ctx_set_orientation(None, 6) == L.jb_ctx_set_arithmetic(None, 1) == -1
    assert L.jb_ctx_orientation(None) == jb.ORIENT_STORED == 1 and jb.ORIENT_EXIF == 0
    assert L.jb_batch_decoder_set_orientation(None, 6) == L.jb_batch_decoder_set_arithmetic(None, 1) == -1


# ---- the stand-alone sanitizer programs ----------------------------------------------------------------------------------
def _built(target):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tools", "fuzz")
    b = subprocess.run(["make", "-C", d, target], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr):
        pytest.skip("toolchain without sanitizer runtimes")
    assert b.returncode == 0, b.stderr[-2000:]
    return os.path.join(d, target)


def test_exif_parser_under_sanitizers():
    """tools/fuzz/exif_check: every prefix and every single-byte mutation of valid II and MM files, in exactly-sized heap
    blocks, under ASan + UBSan."""
    r = subprocess.run([_built("exif_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split()[0]) > 40000, r.stdout


def test_orient_kernel_body_under_sanitizers():
    """tools/fuzz/orient_kernel_check: the body of jb_orient_kernel on the CPU, every orientation x format x edge size and
    the table variant, exactly-sized buffers, under ASan + UBSan."""
    r = subprocess.run([_built("orient_kernel_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split()[0]) >= 8 * 4 * 5 * 2 + 8, r.stdout
