"""The files the host front end's verdicts are pinned on (tests/golden/frontend_verdicts.json, recorded by
tools/record_frontend_verdicts.py with tools/fuzz/frontend_verdicts; compared by tests/test_frontend_verdicts_cpu.py).

seeds() are small valid files: the build's own writer over arithmetic coefficients (no random numbers), two Pillow-made
files of tests/golden/libjpeg_decode_kat.npz for what the writer cannot write (progressive, one component), and the two
small bundled images.  structured() is hand-made surgery on them, one named case per rule of the parser; sweeps() are,
per seed, every prefix up to 8 bytes past its first SOS and every header byte set to 0x00, 0xFF and byte ^ 0x01.

A case is (name, seed name or None, length, ((offset, bytes), ...)): the first `length` bytes of the seed with bytes
replaced, or -- seed None -- the bytes themselves in the patch at offset 0.  case_bytes() gives the byte string."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- seeds ----------------------------------------------------------------------------------------------------------
def _blocks(n):
    """Arithmetic coefficients: DC in -64..64, the first AC positions small and mostly non-zero, the rest zero."""
    b = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(64, dtype=np.int64)[None, :]
    c = np.where(k < 9, (b * 7 + k * 13) % 11 - 5, 0)
    c[:, 0] = (b[:, 0] * 37) % 129 - 64
    c[:, 63] = np.where(b[:, 0] % 3 == 0, 1, 0)  # a ZRL run in every third block
    return c.astype(np.int16)


def _qtabs(n_tables=2):
    q = np.zeros((4, 64), np.uint16)
    for t in range(n_tables):
        q[t] = 1 + (np.arange(64) * (t + 3)) % 97
    return q


def _written(w, h, hs, vs, **kw):
    from jpeg_decoder_amd import synth
    qtab_id = kw.pop("qtab_id", (0, 1, 1))
    return synth.encode_jpeg(_blocks(synth.geometry(w, h, hs, vs)[3]), w, h, hs, vs, _qtabs(max(qtab_id) + 1), qtab_id=qtab_id, **kw)


def segments(f):
    """-> [(marker, offset of its FF, offset of the payload, payload length)] up to and including the first SOS."""
    out, pos = [], 2
    while pos + 4 <= len(f):
        assert f[pos] == 0xff
        m, n = f[pos + 1], (f[pos + 2] << 8) | f[pos + 3]
        out.append((m, pos, pos + 4, n - 2))
        pos += 2 + n
        if m == 0xda:
            break
    return out


def seg(f, marker, nth=0):
    return [s for s in segments(f) if s[0] == marker][nth]


def scan_start(f):
    s = seg(f, 0xda)
    return s[2] + s[3]


def _splice(f, start, end, new=b""):
    return bytes(f[:start]) + bytes(new) + bytes(f[end:])


def _set(f, at, *values):
    return _splice(f, at, at + len(values), bytes(values))


def _segment(marker, payload):
    return bytes([0xff, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def _three_huffman_tables(f):
    """Cr on Huffman tables 2/2: copies of tables 1/1 under id 2 in a DHT of their own in front of the SOS."""
    extra = b""
    for m, at, p, n in segments(f):
        if m != 0xc4:
            continue
        i = p
        while i < p + n:
            total = sum(f[i + 1:i + 17])
            if f[i] & 15 == 1:
                extra += bytes([(f[i] & 0xf0) | 2]) + bytes(f[i + 1:i + 17 + total])
            i += 17 + total
    sos = seg(f, 0xda)
    f = _set(f, sos[2] + 6, 0x22)
    return _splice(f, sos[1], sos[1], _segment(0xc4, extra))


def _one_component(f):
    """The first scan of a file written with one scan per component, under a frame header of that component alone."""
    sof, sos = seg(f, 0xc0), seg(f, 0xda)
    end = f.index(b"\xff\xda", scan_start(f))
    f = _splice(f, end, len(f), b"\xff\xd9")
    return _splice(f, sof[1], sof[2] + sof[3], _segment(0xc0, bytes(f[sof[2]:sof[2] + 5]) + b"\x01" + bytes(f[sof[2] + 6:sof[2] + 9])))


_seeds = None


def seeds():
    """-> {name: bytes}, in a fixed order."""
    global _seeds
    if _seeds is not None:
        return _seeds
    s = {}
    for name, hs, vs in (("444", 1, 1), ("422", 2, 1), ("440", 1, 2), ("420", 2, 2)):
        for w, h in ((16, 16), (17, 9)):
            s[f"w{name}_{w}x{h}"] = _written(w, h, hs, vs)
    s["w444_17x9_ri1"] = _written(17, 9, 1, 1, restart_interval=1)
    s["w444_17x9_ri5"] = _written(17, 9, 1, 1, restart_interval=5)
    s["w420_16x16_dqt16"] = _written(16, 16, 2, 2, dqt16=True)
    s["w420_17x9_3tables"] = _three_huffman_tables(_written(17, 9, 2, 2, qtab_id=(0, 1, 2)))
    s["w420_17x9_scans"] = _written(17, 9, 2, 2, per_component_scans=True)
    s["w444_17x9_scans_ri1"] = _written(17, 9, 1, 1, per_component_scans=True, restart_interval=1)
    s["gray_8x8"] = _one_component(_written(8, 8, 1, 1, per_component_scans=True))
    with np.load(os.path.join(HERE, "golden", "libjpeg_decode_kat.npz")) as z:
        names = {str(z[k]): k.replace("name_", "jpeg_") for k in z.files if k.startswith("name_")}
        s["pillow_gray_33x21"] = z[names["gray_33x21"]].tobytes()
        s["pillow_progressive_45x35"] = z[names["420_45x35_progressive"]].tobytes()
    for name in ("img2", "img4"):
        with open(os.path.join(HERE, "golden", "images", name + ".jpg"), "rb") as fh:
            s[name] = fh.read()
    _seeds = s
    return s


# ---- cases ----------------------------------------------------------------------------------------------------------
def _whole(name, data):
    return (name, None, len(data), ((0, bytes(data)),))


def structured():
    """-> [case]: surgery by hand, every case a rule of the parser or of the scan decoder."""
    S = seeds()
    out = []
    add = lambda name, data: out.append(_whole(name, data))

    # each marker's payload length
    f = S["w444_17x9_ri5"]
    for i, (m, at, p, n) in enumerate(segments(f)):
        for tag, v in (("-1", n + 1), ("+1", n + 3), ("0", 0), ("1", 1), ("ffff", 0xffff)):
            add(f"length:{m:02x}#{i}:{tag}", _set(f, at + 2, v >> 8, v & 255))

    # DQT
    f = S["w420_16x16"]
    _, at, p, n = seg(f, 0xdb)
    add("dqt:pq 2", _set(f, p, 0x20 | f[p]))
    add("dqt:tq 4", _set(f, p, 4))
    add("dqt:one byte short", _splice(_set(f, at + 2, (n + 1) >> 8, (n + 1) & 255), p + n - 1, p + n))
    g = S["w420_16x16_dqt16"]
    _, at, p, n = seg(g, 0xdb)
    add("dqt16:one byte short", _splice(_set(g, at + 2, (n + 1) >> 8, (n + 1) & 255), p + n - 1, p + n))
    add("dqt16:pq 2", _set(g, p, 0x20 | (g[p] & 15)))

    # DHT
    _, at, p, n = seg(f, 0xc4)
    add("dht:class 2", _set(f, p, 0x20 | (f[p] & 15)))
    add("dht:id 4", _set(f, p, (f[p] & 0xf0) | 4))
    add("dht:counts sum to 257", _splice(f, p + 1, p + 17, bytes(14) + bytes([2, 255])))
    assert list(f[p + 1:p + 4]) == [0, 1, 5]
    add("dht:over-subscribed", _set(f, p + 1, 3, 1, 2))  # (three codes of one bit; as many symbols as before)
    add("dht:three more symbols than its bytes", _set(f, p + 1, 3))
    add("dht:17 bytes short", _splice(f, at, p + n, _segment(0xc4, f[p:p + 16])))
    add("dht:symbols short", _splice(f, at, p + n, _segment(0xc4, f[p:p + n - 1])))

    # DRI
    g = S["w444_17x9_ri5"]
    _, at, p, n = seg(g, 0xdd)
    add("dri:length 3", _splice(g, at, p + n, _segment(0xdd, g[p:p + 1])))
    add("dri:length 5", _splice(g, at, p + n, _segment(0xdd, g[p:p + 2] + b"\x00")))
    add("dri:0", _set(g, p, 0, 0))
    add("dri:1 on a file coded with 5", _set(g, p, 0, 1))

    # SOF, on a three-component baseline file, a file of several scans and a one-component file
    for tag in ("w420_16x16", "w420_17x9_scans", "gray_8x8", "pillow_progressive_45x35"):
        f = S[tag]
        m0 = 0xc2 if "progressive" in tag else 0xc0
        _, at, p, n = seg(f, m0)
        nf = f[p + 5]
        add(f"sof:{tag}:precision 12", _set(f, p, 12))
        for v in (0, 1, 2, 3, 4):
            if v != nf:
                add(f"sof:{tag}:nf {v}", _set(f, p + 5, v))
        add(f"sof:{tag}:nf 1, its length", _splice(f, at, p + n, _segment(m0, bytes(f[p:p + 5]) + b"\x01" + bytes(f[p + 6:p + 9]))))
        add(f"sof:{tag}:luma 3x1", _set(f, p + 7, 0x31))
        add(f"sof:{tag}:luma 1x3", _set(f, p + 7, 0x13))
        add(f"sof:{tag}:luma 0x1", _set(f, p + 7, 0x01))
        add(f"sof:{tag}:luma 5x1", _set(f, p + 7, 0x51))
        for c in range(nf):
            add(f"sof:{tag}:tq 4 on component {c}", _set(f, p + 8 + 3 * c, 4))
            if c:
                add(f"sof:{tag}:component {c} 2x1", _set(f, p + 7 + 3 * c, 0x21))
                add(f"sof:{tag}:component {c} 0x1", _set(f, p + 7 + 3 * c, 0x01))
        add(f"sof:{tag}:zero width", _set(f, p + 3, 0, 0))
        add(f"sof:{tag}:zero height", _set(f, p + 1, 0, 0))
        add(f"sof:{tag}:zero width, tq 4", _set(_set(f, p + 3, 0, 0), p + 8, 4))
        add(f"sof:{tag}:zero width, luma 3x1", _set(_set(f, p + 3, 0, 0), p + 7, 0x31))
        add(f"sof:{tag}:payload 5 bytes", _splice(f, at, p + n, _segment(m0, f[p:p + 5])))
        add(f"sof:{tag}:payload one byte short", _splice(f, at, p + n, _segment(m0, f[p:p + n - 1])))
        whole = bytes(f[at:p + n])
        add(f"sof:{tag}:twice", _splice(f, p + n, p + n, whole))
        add(f"sof:{tag}:twice, other sizes", _splice(f, p + n, p + n, _set(whole, 7, 0, 40)))
        add(f"sof:{tag}:twice, 4:4:4 then its own", _splice(f, at, at, _set(_set(whole, 7, 0, 8), 11, 0x11)))
        add(f"sof:{tag}:then SOF2", _splice(f, p + n, p + n, _set(whole, 1, 0xc2)))
        add(f"sof:{tag}:then SOF0", _splice(f, p + n, p + n, _set(whole, 1, 0xc0)))
        for m in (0xc0, 0xc1, 0xc2, 0xc3, 0xc5, 0xc9, 0xcb, 0xcf):
            if m != m0:
                add(f"sof:{tag}:SOF{m - 0xc0}", _set(f, at + 1, m))
        add(f"sof:{tag}:DHP, DAC and JPG markers", _splice(f, at, at, _segment(0xde, b"\x00") + _segment(0xcc, b"\x00\x00") + _segment(0xc8, b"")))
        add(f"sof:{tag}:none", _splice(f, at, p + n))

    # SOS
    for tag in ("w420_16x16", "w420_17x9_scans", "gray_8x8", "pillow_gray_33x21"):
        f = S[tag]
        _, at, p, n = seg(f, 0xda)
        ns = f[p]
        t = p + 1 + 2 * ns
        for v in (0, 1, 2, 3, 4):
            if v != ns:
                add(f"sos:{tag}:ns {v}", _set(f, p, v))
                add(f"sos:{tag}:ns {v}, its length", _splice(f, at, p + n, _segment(0xda, bytes([v]) + bytes((f[p + 1:p + 1 + 2 * ns] * 4)[:2 * v]) + bytes(f[t:t + 3]))))
        add(f"sos:{tag}:component not in the frame", _set(f, p + 1, 9))
        add(f"sos:{tag}:empty payload", _splice(f, at, p + n, _segment(0xda, b"")))
        add(f"sos:{tag}:payload one byte short", _splice(f, at, p + n, _segment(0xda, f[p:p + n - 1])))
        add(f"sos:{tag}:payload one byte long", _splice(f, at, p + n, _segment(0xda, bytes(f[p:p + n]) + b"\x00")))
        if ns == 3:
            add(f"sos:{tag}:components out of frame order", _splice(f, p + 1, p + 5, bytes(f[p + 3:p + 5]) + bytes(f[p + 1:p + 3])))
            add(f"sos:{tag}:last component not in the frame", _set(f, p + 5, 9))
            add(f"sos:{tag}:the first component twice", _set(f, p + 3, f[p + 1]))
        for c in range(ns):
            add(f"sos:{tag}:td 4 on component {c}", _set(f, p + 2 + 2 * c, 0x40 | (f[p + 2 + 2 * c] & 15)))
            add(f"sos:{tag}:ta 4 on component {c}", _set(f, p + 2 + 2 * c, (f[p + 2 + 2 * c] & 0xf0) | 4))
            add(f"sos:{tag}:td 3 (not defined) on component {c}", _set(f, p + 2 + 2 * c, 0x30 | (f[p + 2 + 2 * c] & 15)))
            add(f"sos:{tag}:ta 3 (not defined) on component {c}", _set(f, p + 2 + 2 * c, (f[p + 2 + 2 * c] & 0xf0) | 3))
        add(f"sos:{tag}:ss 1", _set(f, t, 1))
        add(f"sos:{tag}:se 62", _set(f, t + 1, 62))
        add(f"sos:{tag}:ah 1", _set(f, t + 2, 0x10))
        add(f"sos:{tag}:al 1", _set(f, t + 2, 0x01))
        add(f"sos:{tag}:ss 1, td 4", _set(_set(f, t, 1), p + 2, 0x40 | (f[p + 2] & 15)))
        add(f"sos:{tag}:ss 1, no DQT", _set(_set(f, t, 1), seg(f, 0xdb)[1] + 1, 0xfe))

    # a table that is not there, for each component separately
    f = S["w420_17x9_3tables"]
    i = 0
    for m, at, p, n in segments(f):
        if m == 0xdb:
            q = p
            while q < p + n:
                add(f"missing:DQT {f[q] & 15}", _set(f, q, (f[q] & 0xf0) | 3))
                q += 65
        if m == 0xc4:
            q = p
            while q < p + n:
                add(f"missing:DHT {'AC' if f[q] >> 4 else 'DC'} {f[q] & 15}", _set(f, q, (f[q] & 0xf0) | 3))
                q += 17 + sum(f[q + 1:q + 17])
    for tag in ("w420_17x9_scans", "gray_8x8", "pillow_progressive_45x35"):
        f = S[tag]
        for j, (m, at, p, n) in enumerate(segments(f)):
            if m in (0xdb, 0xc4):
                add(f"missing:{tag}:segment {m:02x}#{j} as a comment", _set(f, at + 1, 0xfe))

    # between the segments
    f = S["w420_16x16"]
    first = segments(f)[0]
    sos = seg(f, 0xda)
    add("between:EOI before SOS", _splice(f, sos[1], sos[1], b"\xff\xd9"))
    add("between:EOI after SOI", _splice(f, 2, 2, b"\xff\xd9"))
    g = f
    for m, at, p, n in reversed(segments(f)):
        g = _splice(g, at, at, b"\xff\xff")
    add("between:fill bytes in front of every marker", g)
    add("between:FF01", _splice(f, first[2] + first[3], first[2] + first[3], b"\xff\x01"))
    add("between:a stray RST3", _splice(f, first[2] + first[3], first[2] + first[3], b"\xff\xd3"))
    add("between:a second SOI", _splice(f, first[2] + first[3], first[2] + first[3], b"\xff\xd8"))
    add("between:a byte that is no marker", _splice(f, first[2] + first[3], first[2] + first[3], b"\x00"))
    add("between:ends in FF", _splice(f, sos[1], len(f), b"\xff"))
    add("between:ends in fill bytes", _splice(f, sos[1], len(f), b"\xff\xff\xff"))
    add("between:ends behind a marker", f[:sos[1] + 2])
    add("between:ends inside a length", f[:sos[1] + 3])
    add("between:no SOI", f[2:])
    add("between:SOI alone", f[:2])
    add("between:three bytes", f[:3])
    add("between:empty", b"")
    add("between:an unknown marker with a length", _splice(f, sos[1], sos[1], _segment(0xf3, b"abc")))
    for tag in ("w420_17x9_scans", "pillow_progressive_45x35"):
        f = S[tag]
        second = f.index(b"\xff\xda", scan_start(f))
        sof = seg(f, 0xc2 if "progressive" in tag else 0xc0)
        add(f"between:{tag}:EOI before the second scan", _splice(f, second, second, b"\xff\xd9"))
        add(f"between:{tag}:ends before the second scan", f[:second])
        add(f"between:{tag}:ends in FF before the second scan", f[:second + 1])
        add(f"between:{tag}:ends inside the second SOS", f[:second + 5])
        add(f"between:{tag}:a second frame header before the second scan", _splice(f, second, second, bytes(f[sof[1]:sof[2] + sof[3]])))
        add(f"between:{tag}:DRI 1 before the second scan", _splice(f, second, second, _segment(0xdd, b"\x00\x01")))
        add(f"between:{tag}:a Huffman table dropped before the second scan, bad id", _splice(f, second, second, _segment(0xc4, b"\x05" + bytes(16))))
        add(f"between:{tag}:second scan of the first component again", _set(f, second + 5, f[seg(f, 0xda)[2] + 1]))
        add(f"between:{tag}:no EOI", f[:-2])

    # progressive scans: the four rules
    f = S["pillow_progressive_45x35"]
    _, at, p, n = seg(f, 0xda)
    t = p + 1 + 2 * f[p]
    assert f[p] == 3 and f[t] == 0 and f[t + 1] == 0
    add("progressive:al 14", _set(f, t + 2, 14))
    add("progressive:ah 14", _set(f, t + 2, 0xe0))
    add("progressive:se 64", _set(f, t + 1, 64))
    add("progressive:ss 64", _set(f, t, 64))
    add("progressive:se below ss", _set(f, t, 5, 2))
    add("progressive:a DC scan with se 5", _set(f, t + 1, 5))
    add("progressive:an AC scan of three components", _set(f, t, 1, 5))
    add("progressive:ah 3, al 0", _set(f, t + 2, 0x30))
    add("progressive:ah 1, al 0 (a refinement first)", _set(f, t + 2, 0x10))
    second = f.index(b"\xff\xda", scan_start(f))
    add("progressive:second scan al 14", _set(f, second + 4 + 1 + 2 * f[second + 4] + 2, 14))
    add("progressive:second scan se below ss", _set(f, second + 4 + 1 + 2 * f[second + 4], 9, 3))
    add("progressive:second scan ah 5", _set(f, second + 4 + 1 + 2 * f[second + 4] + 2, 0x50 | (f[second + 4 + 1 + 2 * f[second + 4] + 2] & 15)))

    # the scan's bytes
    for tag in ("w420_16x16", "w444_17x9_ri1", "w444_17x9_ri5", "w420_17x9_scans", "w444_17x9_scans_ri1", "gray_8x8", "pillow_progressive_45x35"):
        f = S[tag]
        b = scan_start(f)
        e = b
        while not (f[e] == 0xff and f[e + 1] not in (0, 0xff) and not 0xd0 <= f[e + 1] <= 0xd7):
            e += 1
        for cut, what in ((b, "0"), (b + 1, "1"), (b + (e - b) // 2, "half")):
            add(f"scan:{tag}:cut after {what} of its bytes", f[:cut])
            add(f"scan:{tag}:{what} of its bytes, then EOI", f[:cut] + b"\xff\xd9")
        add(f"scan:{tag}:no EOI", _splice(f, len(f) - 2, len(f)))
        add(f"scan:{tag}:a byte of FF inside", _set(f, b + (e - b) // 2, 0xff))
        add(f"scan:{tag}:ones inside", _splice(f, b + 2, b + 4, b"\xff\x00\xff\x00"))
        add(f"scan:{tag}:zeros inside", _set(f, b + 2, 0, 0, 0))
        add(f"scan:{tag}:bytes behind the scan", _splice(f, e, e, b"\xff\x00\xaa\x55"))
        r = f.find(b"\xff\xd0", b)
        if r > 0:
            add(f"scan:{tag}:first RST missing", _splice(f, r, r + 2))
            add(f"scan:{tag}:first RST twice", _splice(f, r, r, b"\xff\xd0"))
            add(f"scan:{tag}:first RST numbered 3", _set(f, r + 1, 0xd3))
            add(f"scan:{tag}:an RST at the end", _splice(f, e, e, b"\xff\xd7"))
            add(f"scan:{tag}:no DRI", _set(f, seg(f, 0xdd)[1] + 1, 0xfe))
    f = S["w420_16x16"]
    sos = seg(f, 0xda)
    add("scan:w420_16x16:DRI 1 on a file without RST", _splice(f, sos[1], sos[1], _segment(0xdd, b"\x00\x01")))
    add("scan:w420_16x16:an RST0 inside", _splice(f, scan_start(f) + 4, scan_start(f) + 4, b"\xff\xd0"))

    # the limits of the device decoder (jb_huff_prepare_): table shapes, and frames far larger than their bytes
    import huff_tables
    add("device:more long codes than the tables hold", _written(16, 16, 1, 1, huffman=huff_tables.family("pool25")))
    add("device:long codes that fit", _written(16, 16, 1, 1, huffman=huff_tables.family("pool24")))
    f = S["w444_16x16"]
    p = seg(f, 0xc0)[2]
    add("device:a 32768x32768 frame", _set(f, p + 1, 0x80, 0, 0x80, 0))
    add("device:a 65535x65535 frame", _set(f, p + 1, 0xff, 0xff, 0xff, 0xff))
    f = S["gray_8x8"]
    p = seg(f, 0xc0)[2]
    add("device:a 28672x28672 frame of one component", _set(f, p + 1, 0x70, 0, 0x70, 0))
    add("device:a 32768x32768 frame of one component", _set(f, p + 1, 0x80, 0, 0x80, 0))
    assert len({c[0] for c in out}) == len(out)
    return out


# The byte sweeps of the two bundled images are recorded without the calls that decode the scan (rows of a, c0, c64
# and d): six decodes of a 20 to 30 KB scan for each of 2841 mutants take minutes under the sanitizers, and what a
# header byte does to the scan decoder is in the rows of the seventeen small seeds.
HEADERS_ONLY = ("img2", "img4")
SWEEP_VALUES = (("00", lambda b: 0x00), ("ff", lambda b: 0xff), ("x1", lambda b: b ^ 0x01))


def sweeps():
    """-> {sweep name: [case]}: per seed, every prefix up to 8 bytes past its first SOS segment, and every header byte
    (everything in front of the scan's first byte) set to 0x00, 0xFF and byte ^ 0x01."""
    out = {}
    for name, f in seeds().items():
        b = scan_start(f)
        out[f"prefix:{name}"] = [(f"prefix:{name}:{n}", name, n, ()) for n in range(min(len(f), b + 8) + 1)]
        out[f"bytes:{name}"] = [(f"bytes:{name}:{at}:{tag}", name, len(f), ((at, bytes([fn(f[at])])),))
                                for at in range(b) for tag, fn in SWEEP_VALUES if fn(f[at]) != f[at]]
    return out


def case_bytes(case):
    name, seed, length, patches = case
    f = bytearray(seeds()[seed][:length] if seed is not None else bytes(length))
    for at, data in patches:
        f[at:at + len(data)] = data
    return bytes(f)


def case_line(case):
    """The case as a line of the file tools/fuzz/frontend_verdicts reads."""
    name, seed, length, patches = case
    if seed is None:
        return "B\t%s\t%s" % (name, patches[0][1].hex())
    kind = "H" if name.startswith("bytes:") and seed in HEADERS_ONLY else "C"
    return "\t".join([kind, name, seed, str(length)] + ["%d:%s" % (at, data.hex()) for at, data in patches])


def cases_file(path):
    """Writes every seed and case; -> (names of the structured cases, {sweep: names})."""
    st, sw = structured(), sweeps()
    with open(path, "w") as fh:
        for name, f in seeds().items():
            fh.write("S\t%s\t%s\n" % (name, f.hex()))
        for c in st + [c for cs in sw.values() for c in cs]:
            fh.write(case_line(c) + "\n")
    return [c[0] for c in st], {k: [c[0] for c in v] for k, v in sw.items()}


def entry_files(directory):
    """The good and the corrupt file of the entry points' rows: one the device decoder takes at JPEGBLK_GPU_HUFFMAN=1
    (16 restart intervals or more), and the same with its scan cut in half."""
    good = _written(40, 40, 1, 1, restart_interval=1)
    paths = []
    for name, data in (("good.jpg", good), ("corrupt.jpg", good[:scan_start(good) + (len(good) - scan_start(good)) // 2])):
        paths.append(os.path.join(directory, name))
        with open(paths[-1], "wb") as fh:
            fh.write(data)
    return paths
