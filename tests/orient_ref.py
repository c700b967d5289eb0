"""NumPy statement of "orientation" (include/jpegblk.h) for the tests: T_o as the header's table writes it, and a
hand-built Exif APP1 segment to splice behind a JPEG's SOI (pure Python, no Pillow)."""
import struct

import numpy as np

# the header's table, expression for expression (a: [H, W, ...])
T = {1: lambda a: a,
     2: lambda a: a[:, ::-1],
     3: lambda a: a[::-1, ::-1],
     4: lambda a: a[::-1],
     5: lambda a: a.transpose(1, 0, 2),
     6: lambda a: a.transpose(1, 0, 2)[:, ::-1],
     7: lambda a: a[::-1, ::-1].transpose(1, 0, 2),
     8: lambda a: a.transpose(1, 0, 2)[::-1]}


def orient(a, o):
    return np.ascontiguousarray(T[o](np.asarray(a)))


def size(w, h, o):
    return (h, w) if o >= 5 else (w, h)


def tiff(entries, big=False, ifd_offset=8):
    """A TIFF header and one IFD: entries = [(tag, type, count, the four value bytes as an int or bytes)]."""
    e = ">" if big else "<"
    out = (b"MM" if big else b"II") + struct.pack(e + "HI", 42, ifd_offset) + b"\0" * (ifd_offset - 8)
    out += struct.pack(e + "H", len(entries))
    for tag, typ, count, value in entries:
        out += struct.pack(e + "HHI", tag, typ, count)
        if isinstance(value, bytes):
            out += value
        elif typ == 3 and count == 1:
            out += struct.pack(e + "HH", value, 0)     # a SHORT sits in the first two of the four bytes
        else:
            out += struct.pack(e + "I", value)
    return out + struct.pack(e + "I", 0)


def app1(payload):
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def exif_app1(value, big=False, typ=3, count=1, with_tag=True):
    entries = [(0x0100, 4, 1, 640)]
    if with_tag:
        entries.append((0x0112, typ, count, value))
    entries.append((0x0128, 3, 1, 2))
    return app1(b"Exif\0\0" + tiff(entries, big))


def splice(jpeg, segment):
    """The file with `segment` right behind SOI."""
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + segment + jpeg[2:]


def tiny_jpeg(before_sos=b""):
    """SOI, the given segments, a stub DQT, SOS, two data bytes, EOI: enough for a parser that stops at SOS."""
    return b"\xff\xd8" + before_sos + b"\xff\xdb\x00\x04\x00\x01" + b"\xff\xda\x00\x02\x12\x34\xff\xd9"


APP0 = b"\xff\xe0\x00\x10JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
XMP = app1(b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta><rdf:Description tiff:Orientation=\"6\"/></x:xmpmeta>")
