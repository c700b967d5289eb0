"""NumPy statement of "draft decode" (include/jpegblk.h), on top of libjpeg_ref: jdmaster.c's block sizes, jidctred.c's
4 x 4, 2 x 2 and 1 x 1 reduced IDCTs, and libjpeg_ref's upsampling and colour on the draft frame.
decode_blocks(desc, qtabs, coef, K) -> the image [ceil(H / K), ceil(W / K), 3] uint8 that libjpeg gives for those
coefficients at scale 1 / K -- Pillow's draft -- held against Pillow's own bits in test_draft_cpu.py.  As in libjpeg_ref
everything is int64 and an input outside the contract's domain raises OutOfDomain."""
import io
import os

import numpy as np

import libjpeg_ref
from libjpeg_ref import OutOfDomain, _i16, _i32, colour, upsample   # noqa: F401  (OutOfDomain: for callers)

DENOMS = (2, 4, 8)


def load_kat():
    """tests/golden/libjpeg_draft_kat.npz (tools/gen_draft_kat.py) -> [(name, jpeg bytes, {K: Pillow's draft decode})]:
    every file of libjpeg_decode_kat.npz (its bytes are taken from there) and the files only this one stores"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "libjpeg_draft_kat.npz"))
    base = {name: jpeg for name, jpeg, _ in libjpeg_ref.load_kat()}
    out = []
    for k in range(int(z["n"])):
        name = str(z[f"name_{k}"])
        jpeg = z[f"jpeg_{k}"].tobytes() if f"jpeg_{k}" in z.files else base[name]
        out.append((name, jpeg, {K: z[f"rgb_{k}_{K}"] for K in DENOMS}))
    return out


def geometry(w, h, hs, vs, K):
    """-> (ow, oh, S, Sc, eh, ev, fancy): jb_draft_geometry_of, restated"""
    S = 8 // K
    Sc = S
    while Sc < 8 and (hs * S) % (2 * Sc) == 0 and (vs * S) % (2 * Sc) == 0:
        Sc *= 2
    return -(-w // K), -(-h // K), S, Sc, hs * S // Sc, vs * S // Sc, int(S > 1)


def _red4_1d(v, n, what):
    """v [..., 8] along the last axis (index 4 is never read) -> the 4-point network's outputs, each D(x, n)"""
    c = lambda x: _i32(x, what)
    in0, in1, in2, in3, _, in5, in6, in7 = (v[..., k] for k in range(8))
    t0 = c(in0 << 14)
    t2 = c(c(in2 * 15137) - c(in6 * 6270))
    t10, t12 = c(t0 + t2), c(t0 - t2)
    a = c(c(c(-in7 * 1730) + c(in5 * 11893)) + c(c(-in3 * 17799) + c(in1 * 8697)))
    b = c(c(c(-in7 * 4176) - c(in5 * 4926)) + c(c(in3 * 7373) + c(in1 * 20995)))
    r = 1 << (n - 1)
    return np.stack([c(o + r) >> n for o in (c(t10 + b), c(t12 + a), c(t12 - a), c(t10 - b))], axis=-1)


def _red2_1d(v, n, what):
    """v [..., 8] (indices 0, 1, 3, 5, 7 are read) -> the 2-point network's outputs"""
    c = lambda x: _i32(x, what)
    in0, in1, in3, in5, in7 = (v[..., k] for k in (0, 1, 3, 5, 7))
    t10 = c(in0 << 15)
    t = c(c(c(-in7 * 5906) + c(in5 * 6967)) + c(c(-in3 * 10426) + c(in1 * 29692)))
    r = 1 << (n - 1)
    return np.stack([c(o + r) >> n for o in (c(t10 + t), c(t10 - t))], axis=-1)


def idct_blocks(coef, q, size):
    """coef [n, 64] (natural order), q [64] -> samples [n, size, size] uint8; size 8 is libjpeg_ref's islow"""
    if size == 8:
        return libjpeg_ref.idct_blocks(coef, q)
    v = _i32(coef.astype(np.int64) * q.astype(np.int64)[None, :], "coef * q").reshape(-1, 8, 8)
    if size == 1:
        out = (v[:, :1, :1] + 4) >> 3
        return np.clip(out + 128, 0, 255).astype(np.uint8)
    net, n1, n2 = (_red4_1d, 12, 19) if size == 4 else (_red2_1d, 13, 20)
    _i16(v, "the columns pass's input")
    ws = net(v.transpose(0, 2, 1), n1, "the columns pass").transpose(0, 2, 1)   # [n, size, 8]: along the columns
    _i16(ws, "the rows pass's input")
    out = net(ws, n2, "the rows pass")
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes_of(desc, qtabs, coef, K):
    """-> (Y [mcus_y * vs * S, mcus_x * hs * S], Cb, Cr [mcus_y * Sc, mcus_x * Sc]) uint8: every sample of the draft"""
    w, h, hs, vs = int(desc.width), int(desc.height), int(desc.hs), int(desc.vs)
    _, _, S, Sc, _, _, _ = geometry(w, h, hs, vs, K)
    ids = [int(desc.qtab_id[c]) for c in range(3)]
    ny, nb = hs * vs, hs * vs + 2
    bw, bh = (w + 7) // 8, (h + 7) // 8
    mcus_x, mcus_y = (bw + hs - 1) // hs, (bh + vs - 1) // vs
    coef = np.asarray(coef).reshape(mcus_y, mcus_x, nb, 64)
    qtabs = np.asarray(qtabs).reshape(-1, 64)
    y = idct_blocks(coef[:, :, :ny].reshape(-1, 64), qtabs[ids[0]], S).reshape(mcus_y, mcus_x, vs, hs, S, S)
    y = y.transpose(0, 2, 4, 1, 3, 5).reshape(mcus_y * vs * S, mcus_x * hs * S)
    cs = []
    for c in (1, 2):
        p = idct_blocks(coef[:, :, ny + c - 1].reshape(-1, 64), qtabs[ids[c]], Sc).reshape(mcus_y, mcus_x, Sc, Sc)
        cs.append(p.transpose(0, 2, 1, 3).reshape(mcus_y * Sc, mcus_x * Sc))
    return y, cs[0], cs[1]


def _chroma(c, ow, oh, eh, ev, fancy):
    if fancy:
        return upsample(c, ow, oh, eh, ev)
    dw, dh = -(-ow // eh), -(-oh // ev)
    return c[:dh, :dw].astype(np.int64)[(np.arange(oh) // ev)[:, None], (np.arange(ow) // eh)[None, :]]


def decode_blocks(desc, qtabs, coef, K):
    """desc: anything with width, height, hs, vs, qtab_id; qtabs [4, 64]; coef [n_coded_blocks, 64]; K in 1, 2, 4, 8
    -> the draft image [oh, ow, 3] uint8 (K = 1: libjpeg_ref.decode_blocks)"""
    if K == 1:
        return libjpeg_ref.decode_blocks(desc, qtabs, coef)
    ow, oh, _, _, eh, ev, fancy = geometry(int(desc.width), int(desc.height), int(desc.hs), int(desc.vs), K)
    y, cb, cr = planes_of(desc, qtabs, coef, K)
    return colour(y[:oh, :ow].astype(np.int64), _chroma(cb, ow, oh, eh, ev, fancy), _chroma(cr, ow, oh, eh, ev, fancy))


def pillow_draft(jpeg, K):
    """Pillow's decode of `jpeg` at libjpeg scale 1 / K, forced the way JpegImageFile.draft sets it -> [oh, ow, 3] uint8"""
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    ow, oh = -(-im.size[0] // K), -(-im.size[1] // K)
    im._size = (ow, oh)
    im.decoderconfig = (K, 0)
    im.tile = [im.tile[0]._replace(extents=(0, 0, ow, oh))]
    return np.asarray(im.convert("RGB"))
