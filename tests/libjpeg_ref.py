"""NumPy statement of "decoder arithmetic" JB_ARITH_LIBJPEG (include/jpegblk.h), rule by rule: dequantise and
jidctint.c's islow IDCT, jdsample.c's fancy chroma upsampling, jdcolor.c's fixed-point colour conversion.
decode_blocks(desc, qtabs, coef) -> the full-size image [H, W, 3] uint8 that libjpeg(-turbo) -- Pillow's
Image.open(f).convert("RGB") -- gives for those coefficients (held against Pillow's own bits in test_libjpeg_cpu.py).
Everything is computed in int64, and an input that leaves the contract's domain (an intermediate beyond int32, a pass
input beyond int16) raises OutOfDomain: outside it libjpeg's C code, its SIMD code and a plain clamp disagree, so no
test may compare bits there without knowing."""
import os

import numpy as np


def load_kat():
    """tests/golden/libjpeg_decode_kat.npz (tools/gen_libjpeg_kat.py) -> [(name, jpeg bytes, Pillow's convert("RGB") of them)]"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "libjpeg_decode_kat.npz"))
    return [(str(z[f"name_{k}"]), z[f"jpeg_{k}"].tobytes(), z[f"rgb_{k}"]) for k in range(int(z["n"]))]


class OutOfDomain(ValueError):
    pass


def _i32(x, what):
    if x.size and (x.min() < -2 ** 31 or x.max() > 2 ** 31 - 1):
        raise OutOfDomain(f"{what} leaves int32")
    return x


def _i16(x, what):
    if x.size and (x.min() < -2 ** 15 or x.max() > 2 ** 15 - 1):
        raise OutOfDomain(f"{what} leaves int16")
    return x


def _islow_1d(v, n, what):
    """v [..., 8] int64 along the last axis -> the network's eight outputs, each (x + (1 << (n - 1))) >> n"""
    c = lambda x: _i32(x, what)
    in0, in1, in2, in3, in4, in5, in6, in7 = (v[..., k] for k in range(8))
    z1 = c((in2 + in6) * 4433)
    tmp2 = c(z1 - c(in6 * 15137))
    tmp3 = c(z1 + c(in2 * 6270))
    tmp0 = c((in0 + in4) << 13)
    tmp1 = c((in0 - in4) << 13)
    tmp10, tmp13, tmp11, tmp12 = c(tmp0 + tmp3), c(tmp0 - tmp3), c(tmp1 + tmp2), c(tmp1 - tmp2)
    t0, t1, t2, t3 = in7, in5, in3, in1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = c((z3 + z4) * 9633)
    t0, t1, t2, t3 = c(t0 * 2446), c(t1 * 16819), c(t2 * 25172), c(t3 * 12299)
    z1, z2 = c(z1 * -7373), c(z2 * -20995)
    z3, z4 = c(c(z3 * -16069) + z5), c(c(z4 * -3196) + z5)
    t0, t1, t2, t3 = c(t0 + c(z1 + z3)), c(t1 + c(z2 + z4)), c(t2 + c(z2 + z3)), c(t3 + c(z1 + z4))
    r = 1 << (n - 1)
    outs = [c(tmp10 + t3), c(tmp11 + t2), c(tmp12 + t1), c(tmp13 + t0), c(tmp13 - t0), c(tmp12 - t1), c(tmp11 - t2), c(tmp10 - t3)]
    return np.stack([c(o + r) >> n for o in outs], axis=-1)


def idct_blocks(coef, q):
    """coef [n, 64] (natural order), q [64] -> samples [n, 8, 8] uint8"""
    v = _i32(coef.astype(np.int64) * q.astype(np.int64)[None, :], "coef * q").reshape(-1, 8, 8)
    _i16(v, "the columns pass's input")
    ws = _islow_1d(v.transpose(0, 2, 1), 11, "the columns pass").transpose(0, 2, 1)   # along the columns
    _i16(ws, "the rows pass's input")
    out = _islow_1d(ws, 18, "the rows pass")
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes_of(desc, qtabs, coef):
    """-> (Y [mcus_y * 8 vs, mcus_x * 8 hs], Cb, Cr [mcus_y * 8, mcus_x * 8]) uint8: every coded sample"""
    w, h, hs, vs = int(desc.width), int(desc.height), int(desc.hs), int(desc.vs)
    ids = [int(desc.qtab_id[c]) for c in range(3)]
    ny, nb = hs * vs, hs * vs + 2
    bw, bh = (w + 7) // 8, (h + 7) // 8
    mcus_x, mcus_y = (bw + hs - 1) // hs, (bh + vs - 1) // vs
    coef = np.asarray(coef).reshape(mcus_y, mcus_x, nb, 64)
    qtabs = np.asarray(qtabs).reshape(-1, 64)
    y = idct_blocks(coef[:, :, :ny].reshape(-1, 64), qtabs[ids[0]]).reshape(mcus_y, mcus_x, vs, hs, 8, 8)
    y = y.transpose(0, 2, 4, 1, 3, 5).reshape(mcus_y * vs * 8, mcus_x * hs * 8)
    cs = []
    for c in (1, 2):
        p = idct_blocks(coef[:, :, ny + c - 1].reshape(-1, 64), qtabs[ids[c]]).reshape(mcus_y, mcus_x, 8, 8)
        cs.append(p.transpose(0, 2, 1, 3).reshape(mcus_y * 8, mcus_x * 8))
    return y, cs[0], cs[1]


def upsample(c, w, h, hs, vs):
    """one chroma plane (coded samples) -> [h, w] int64 at the luma grid: jdsample.c's fancy upsampling, with every
    neighbour index clamped to the dw x dh samples the frame has"""
    dw, dh = (w + hs - 1) // hs, (h + vs - 1) // vs
    c = c[:dh, :dw].astype(np.int64)
    plain = hs == 2 and dw <= 2
    ys, xs = np.arange(h), np.arange(w)
    if plain:
        return c[(ys // vs)[:, None], (xs // hs)[None, :]]
    if vs == 2:
        cy = ys // 2
        nyr = np.clip(cy + np.where(ys & 1, 1, -1), 0, dh - 1)
        rows = 3 * c[cy] + c[nyr]                                  # [h, dw]: 4:2:0 keeps the sum unscaled
        if hs == 1:
            return (rows + np.where(ys & 1, 2, 1)[:, None]) >> 2
    else:
        rows = c[ys]
    if hs == 1:
        return rows
    cx = xs // 2
    nxc = np.clip(cx + np.where(xs & 1, 1, -1), 0, dw - 1)
    s = 3 * rows[:, cx] + rows[:, nxc]
    if vs == 2:
        return (s + np.where(xs & 1, 7, 8)[None, :]) >> 4
    return (s + np.where(xs & 1, 2, 1)[None, :]) >> 2


def colour(y, cb, cr):
    """[h, w] int64 samples -> [h, w, 3] uint8"""
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode_blocks(desc, qtabs, coef):
    """desc: anything with width, height, hs, vs, qtab_id; qtabs [4, 64] natural order; coef [n_coded_blocks, 64] in
    decode order -> [H, W, 3] uint8.  Raises OutOfDomain where the contract pins nothing."""
    w, h, hs, vs = int(desc.width), int(desc.height), int(desc.hs), int(desc.vs)
    y, cb, cr = planes_of(desc, qtabs, coef)
    return colour(y[:h, :w].astype(np.int64), upsample(cb, w, h, hs, vs), upsample(cr, w, h, hs, vs))
