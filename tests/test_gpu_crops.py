"""Per-image rectangles on the GPU (-m gpu): with crops=[r_0, r_1, ...] and resize=(ow, oh) image i of a launch, or file
i of a batch, comes out as format_ref.to_format(resize_ref.area_resize(full_i[slice of r_i], ow, oh), fmt, scale, bias)
bit for bit, where full_i is the oracle's full-size decode (seam) or the reference's golden RGB (batch decoder): never
something the code under test computed.  At the seam the whole sentinel-filled buffer is compared, pads included."""
import ctypes
import os

import numpy as np
import pytest

import format_ref as fr
from conftest import GOLD, load_golden
from resize_ref import area_resize
from seam_harness import LAYOUTS, NO_PARAMS, SENT, Seam, _oracle_full

pytestmark = pytest.mark.gpu

SETS = list(fr.PARAM_SETS.items())


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    return jb


@pytest.fixture(scope="module")
def ctx(jb):
    c = jb.Context(0)
    yield c
    c.close()


def _params(i, fmt):
    return SETS[(i + fmt) % 3][1] if fmt >= 2 else ((1, 1, 1), (0, 0, 0))


class _Through:
    """What Seam.run sees as its context: the launch goes out with crops= (a list), or -- crops = "null" -- straight to
    the C entry point with rois = NULL.  catch: a refusal is kept in .error instead of raised, so that run() still
    returns the buffer the refused call was given."""

    def __init__(self, jb, ctx, crops, catch):
        self.jb, self.ctx, self.crops, self.catch, self.error = jb, ctx, crops, catch, None

    def blocks_to_rgb_device(self, batch, **kw):
        try:
            if self.crops == "null":
                w, h = kw["resize"]
                rc = self.jb.lib().jb_blocks_to_rgb_device_crops(self.ctx._h, ctypes.byref(batch), None, w, h, None, None)
                if rc:
                    raise self.jb.JbError(rc, self.jb.lib().jb_last_error(self.ctx._h).decode())
            else:
                self.ctx.blocks_to_rgb_device(batch, crops=self.crops, **kw)
        except self.jb.JbError as e:
            if not self.catch:
                raise
            self.error = e

    def synchronize(self):
        self.ctx.synchronize()


class CropSeam(Seam):
    """Seam whose run passes crops= (self.crops; None: the launch of the harness as it is).  After a run with
    self.catch set, self.error is the refusal (or None)."""
    crops = None
    catch = False
    error = None

    def run(self, ctx, fmt, out_size, scale_bias=NO_PARAMS, *, scale=1, roi=None, resize=None):
        if self.crops is None:
            return super().run(ctx, fmt, out_size, scale_bias, scale=scale, roi=roi, resize=resize)
        through = _Through(self.jb, ctx, self.crops, self.catch)
        out = super().run(through, fmt, out_size, scale_bias, scale=scale, roi=roi, resize=resize)
        self.error = through.error
        return out


def _cut(full, r):
    x, y, w, h = r
    return full[y:y + h, x:x + w]


def _check(s, ctx, fulls, crops, resize, fmt, scale=(1, 1, 1), bias=(0, 0, 0), tag=None):
    """The launch with `crops` and `resize`: image i's output is the reference of its own rectangle of fulls[i], and
    every other byte of the buffer still holds the sentinel."""
    wants = [fr.to_format(area_resize(_cut(f, r), *resize), fmt, scale, bias) for f, r in zip(fulls, crops)]
    s.crops = list(crops)
    try:
        return s.check(ctx, wants, fmt, (scale, bias), resize=resize, tag=(tag, crops))
    finally:
        s.crops = None


# ---- five images of 600 x 100 (wider than one tile's 512 pixels in every layout), per-image tables --------------------
BW, BH = 600, 100
T = (37, 29)
FIVE = [(0, 0, BW, BH),            # the whole image: the most tiles ...
        (599, 99, 1, 1),           # ... next to the fewest; the last pixel
        (19, 9, 5, 3),             # inside one MCU
        (509, 3, 10, 90),          # across the tile boundary at 512, 4-pixel groups cut on both edges
        (1, 50, 598, 1)]           # a one-row strip
_five = {}


def _batch5(jb, oracle, hs, vs, qid=(0, 1, 2)):
    """-> (CropSeam, the oracle's five full-size images), made once per layout and table assignment and not changed"""
    from jpeg_decoder_amd import synth
    key = (hs, vs, qid)
    if key not in _five:
        coefs, qs, fulls = [], [], []
        for i in range(5):
            q = synth.annex_k_qtabs(40 + 12 * i).copy()          # per-image quantisation tables
            q[2] = np.clip(q[1].astype(int) * 3 // 2 + 1, 1, 255)
            c = synth.synth_blocks(BW, BH, hs, vs, image_index=20 + i, qtabs=q, qtab_id=qid, dense=(i == 4))[0]
            coefs.append(c), qs.append(q)
            fulls.append(_oracle_full(oracle, BW, BH, hs, vs, c, q, qid))
        _five[key] = CropSeam(jb, BW, BH, hs, vs, coefs, qs, qid, pad_row=13, pad_plane=7, pad_img=77), fulls
    return _five[key]


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_five_rectangles_per_layout(jb, ctx, oracle, hs, vs):
    s, fulls = _batch5(jb, oracle, hs, vs)
    for k, fmt in enumerate((0, 1, 2, 3) if (hs, vs) == (2, 2) else (0, 3)):
        _check(s, ctx, fulls, FIVE, T, fmt, *_params(k, fmt), tag=(hs, vs, fmt))
        # and in another order: the fewest tiles first, the most last
        order = [1, 2, 4, 3, 0]
        _check(s, ctx, [fulls[i] for i in range(5)], [FIVE[i] for i in order], T, fmt, *_params(k, fmt), tag=(hs, vs, fmt, "reordered"))
    if (hs, vs) == (2, 2):     # Cb and Cr share a table: the other 4:2:0 instantiation
        s, fulls = _batch5(jb, oracle, hs, vs, (0, 1, 1))
        _check(s, ctx, fulls, FIVE, T, 0, tag=(hs, vs, "one chroma table"))


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_equal_rectangles_are_the_shipped_route(jb, ctx, oracle, hs, vs):
    """All five rectangles equal: byte for byte the buffer of roi= + resize=."""
    s, fulls = _batch5(jb, oracle, hs, vs)
    for k, (r, fmt) in enumerate(((FIVE[3], 0), (FIVE[3], 3), ((37, 18, 224, 64), 2), (FIVE[0], 1))):
        host, _ = _check(s, ctx, fulls, [r] * 5, T, fmt, *_params(k, fmt), tag=(hs, vs))
        old, _ = s.run(ctx, fmt, T, _params(k, fmt), roi=r, resize=T)
        assert np.array_equal(host, old), (hs, vs, r, fmt)


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_seam_random_crop_is_the_slice(jb, ctx, oracle, hs, vs):
    """Five positions of one 224 x 64 rectangle, target 224 x 64: no resampling, the slices themselves."""
    s, fulls = _batch5(jb, oracle, hs, vs, (0, 1, 1))
    crops = [(0, 0, 224, 64), (376, 36, 224, 64), (13, 7, 224, 64), (200, 20, 224, 64), (301, 35, 224, 64)]
    host, idx = _check(s, ctx, fulls, crops, (224, 64), 0, tag=(hs, vs))
    for i, r in enumerate(crops):
        assert np.array_equal(host[idx[i]].reshape(64, 224, 3), _cut(fulls[i], r)), (hs, vs, i)
    _check(s, ctx, fulls, crops, (224, 64), 3, *fr.IMAGENET, tag=(hs, vs))


def test_seam_more_images_than_a_table_holds(jb, ctx, oracle, monkeypatch):
    """70 images (three launch pairs at 32 per table); then on a context whose scratch ends the sub-batches on bytes
    before the count: identical buffers.  (The knob is read when a context is created.)"""
    from jpeg_decoder_amd import synth
    w, h, n = 40, 24, 70
    q = synth.annex_k_qtabs(60)
    coefs = [synth.synth_blocks(w, h, 2, 2, image_index=100 + i, qtabs=q)[0] for i in range(n)]
    fulls = [_oracle_full(oracle, w, h, 2, 2, c, q) for c in coefs]
    rng = np.random.default_rng(70)
    crops = []
    for _ in range(n):
        cw, ch = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        crops.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
    crops[33] = (0, 0, w, h)
    s = CropSeam(jb, w, h, 2, 2, coefs, [q] * n, pad_row=3, pad_plane=5, pad_img=7)
    first = {fmt: _check(s, ctx, fulls, crops, (8, 8), fmt, *_params(1, fmt))[0] for fmt in (0, 3)}
    # 3 * 40 * 24 = 2,880 bytes for the largest intermediate: 4,000 hold one to a few images, and one image alone at 1,000
    for cap in (4000, 1000):
        assert sum(3 * c[2] * c[3] for c in crops[:32]) > cap
        monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", str(cap))
        with jb.Context(0) as small:
            for fmt in (0, 3):
                s.crops = crops
                try:
                    host, _ = s.run(small, fmt, (8, 8), _params(1, fmt), resize=(8, 8))
                finally:
                    s.crops = None
                assert np.array_equal(host, first[fmt]), (cap, fmt)


def test_seam_refusals_write_nothing(jb, ctx, oracle):
    s, fulls = _batch5(jb, oracle, 2, 2)
    s.catch = True
    try:
        bad = list(FIVE)
        bad[3] = (509, 3, BW - 509 + 1, 90)                  # image 3's rectangle one pixel too wide
        for crops, resize, status in ((bad, T, -2), ("null", T, -1), (FIVE, (0, 5), -2), (FIVE[:4], T, -2)):
            s.crops = crops
            host, _ = s.run(ctx, 0, T, resize=resize)
            assert s.error is not None and s.error.status == status, (crops, resize, s.error)
            assert (host == SENT).all(), (crops, resize)
            if crops is bad:
                text = str(s.error)
                assert "image 3" in text and f"{BW} x {BH}" in text and f"{BW - 509 + 1} x 90" in text, text
    finally:
        s.crops, s.catch = None, False
    _check(s, ctx, fulls, FIVE, T, 0)                        # and the context still serves a good call


# ---- the batch decoder -------------------------------------------------------------------------
NAMES = ["img2", "img2", "img2", "img4", "img6", "img"]     # 400x266 4:2:0 (three times), 800x400 4:4:4, 427x640 4:2:0, 679x451 4:2:0
CROPS = [(0, 0, 400, 266), (13, 7, 224, 200), (399, 265, 1, 1), (100, 50, 512, 300), (5, 600, 400, 40), (300, 200, 37, 29)]
OTHER = [(200, 100, 100, 100), (0, 0, 400, 266), (1, 2, 3, 4), (0, 0, 800, 400), (0, 0, 427, 640), (3, 1, 670, 449)]
BT = (32, 32)


def _gold(name):
    return os.path.join(GOLD, "images", name + ".jpg"), load_golden(name)[3]


def _want(rgb, spec, roi=None, t=BT):
    src = rgb if roi is None else _cut(rgb, roi)
    return fr.to_format(area_resize(src, *t), spec.format, list(spec.scale), list(spec.bias))


def _all_good(imgs, st, tm, rgbs, spec, crops):
    assert tm["rc"] == 0 and st == [0] * len(crops), (tm, st)
    for i, r in enumerate(crops):
        assert fr.same_bits(imgs[i], _want(rgbs[i], spec, r)), (i, r)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("huff", ["0", None])
def test_batch_decoder_crops_every_route(jb, monkeypatch, huff, threads):
    import torch
    if huff is None:
        monkeypatch.delenv("JPEGBLK_GPU_HUFFMAN", raising=False)
    else:
        monkeypatch.setenv("JPEGBLK_GPU_HUFFMAN", huff)
    paths, rgbs = zip(*[_gold(n) for n in NAMES])
    paths, n = list(paths), len(NAMES)
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    with jb.BatchDecoder(threads, 0, resize=BT, fmt=spec, arena_bytes=1 << 20) as dec:      # a pinned arena
        _all_good(*dec.run(paths, crops=CROPS), rgbs, spec, CROPS)
    with jb.BatchDecoder(threads, 0, resize=BT, fmt=spec) as dec:
        _all_good(*dec.run(paths, crops=CROPS), rgbs, spec, CROPS)
        assert [tuple(i.shape) for i in dec.run(paths, crops=OTHER)[0]] == [(3, BT[1], BT[0])] * n
        out = torch.full((n, 3, BT[1], BT[0]), 7.0, dtype=torch.float16, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(paths, out, crops=CROPS)
        assert ret is out
        _all_good(out.cpu().numpy(), st, tm, rgbs, spec, CROPS)
        t0 = dec.submit(paths, crops=CROPS)
        t1 = dec.submit(paths, crops=OTHER)                  # two in flight, each with its own rectangles
        for t, crops in ((t0, CROPS), (t1, OTHER)):
            _all_good(*dec.collect(t), rgbs, spec, crops)
        # one rectangle that does not fit its file: -2 and None for that file only
        bad = list(CROPS)
        bad[1] = (13, 7, 388, 200)                           # img2 is 400 wide
        imgs, st, tm = dec.run(paths, crops=bad)
        for i in range(n):
            if i == 1:
                assert st[i] == -2 and imgs[i] is None, st
            else:
                assert st[i] == 0 and fr.same_bits(imgs[i], _want(rgbs[i], spec, bad[i])), (i, st)
        out.fill_(7.0)
        ret, st, tm = dec.run_to_tensor(paths, out, crops=bad)
        assert st[1] == -2 and (out[1] == 7.0).all() and fr.same_bits(out[2].cpu().numpy(), _want(rgbs[2], spec, bad[2]))
        # refusals: crops of the wrong length; a decoder-wide rectangle as well; no target
        for call in (dec.run, dec.submit):
            with pytest.raises(jb.JbError) as e:
                call(paths, crops=CROPS[:5])
            assert e.value.status == -2
        dec.set_roi((0, 0, 100, 100))
        assert dec.run(paths, crops=CROPS)[2]["rc"] == -7
        with pytest.raises(jb.JbError) as e:
            dec.submit(paths, crops=CROPS)
        assert e.value.status == -7
        dec.set_roi(None)
        dec.set_resize(None)
        imgs, st, tm = dec.run(paths, crops=CROPS)
        assert tm["rc"] == -7 and imgs == [None] * n
        with pytest.raises(jb.JbError) as e:
            dec.submit(paths, crops=CROPS)
        assert e.value.status == -7
        dec.set_resize(BT)
        _all_good(*dec.run(paths, crops=CROPS), rgbs, spec, CROPS)     # the decoder is as good as before
        _all_good(*dec.run(paths), rgbs, spec, [None] * n)             # and a plain run is what set_resize gives
