"""The resize family's kernels where their other GPU tests do not take them (-m gpu): saturating content through every
route (both clamps of jb_filter_kernel, and every u8 value at the area, resample and filter stores), the chunked passes
at eight rows per workgroup, frames at the 65535 limit, and a sweep of ratios over the device-computed weights.  The
expected bits come from the oracle's full-size decode and the NumPy restatements (pillow_resize_ref, resize_ref,
format_ref) alone; the whole sentinel-filled buffer is compared.  Where a test is about a property of its inputs -- a
clamp that must bite, a pass that must be chunked, a tap count next to the cap -- it asserts that property first, from
the formulas, so that it cannot turn into one of the already covered cases unnoticed."""
import os
import re

import numpy as np
import pytest

import format_ref as fr
import pillow_resize_ref as pr
from conftest import ROOT
from resize_ref import area_resize
from seam_harness import LAYOUTS, NO_PARAMS, SENT, _oracle_full
from test_gpu_filter import FilterSeam

pytestmark = pytest.mark.gpu

AREA, BILINEAR, BICUBIC = pr.FILTER_AREA, pr.FILTER_BILINEAR, pr.FILTER_BICUBIC
FILTERS = (BILINEAR, BICUBIC)
# format 0 and 1, and 2 and 3 with every parameter set
FMT_CASES = [(0, NO_PARAMS), (1, NO_PARAMS)] + [(fmt, sb) for fmt in (2, 3) for sb in fr.PARAM_SETS.values()]
FMT_0_3 = [(0, NO_PARAMS), (3, fr.F16_TIES), (3, fr.IMAGENET)]


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


def _cut(full, r):
    return full if r is None else full[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]


def _ref(full, rect, target, filt):
    """the expected uint8 image of one rectangle (None: the whole frame) -> target"""
    if target is None:
        return _cut(full, rect)
    return area_resize(_cut(full, rect), *target) if filt == AREA else pr.resize(full, rect, target, filt)


def _launch(s, ctx, want_u8, fmt, sb, *, rect=None, target=None, filt=AREA, crops=None, tag=None):
    """One launch of seam `s`: image i's output is want_u8[i] in format `fmt` with sb = (scale, bias), bit for bit."""
    wants = [fr.to_format(u, fmt, *sb) for u in want_u8]
    s.filter, s.crops = filt, (list(crops) if crops is not None else None)
    try:
        return s.check(ctx, wants, fmt, sb, roi=rect, resize=target, tag=(tag, filt, rect, crops, target))
    finally:
        s.filter, s.crops = 0, None


def _check(s, ctx, fulls, rect, target, filt, cases, crops=None, tag=None):
    """The launch in every (fmt, parameters) of `cases`, against the references of fulls[i] -> the expected uint8 images"""
    rects = crops if crops is not None else [rect] * len(fulls)
    want = [_ref(f, r, target, filt) for f, r in zip(fulls, rects)]
    for fmt, sb in cases:
        _launch(s, ctx, want, fmt, sb, rect=rect, target=target, filt=filt, crops=crops, tag=tag)
    return want


_frames = {}


def _frame(jb, oracle, w, h, hs, vs, n=1, saturating=True):
    """-> (FilterSeam over n images of w x h, the oracle's full-size images), made once and not changed.  saturating:
    uniform coefficients in -700..700 under the quality-50 tables, seeds 5, 6, ...: at least a quarter of the pixels is
    0 and at least a quarter is 255 (asserted); else synth_blocks' mid-grey noise."""
    from jpeg_decoder_amd import synth
    key = (w, h, hs, vs, n, saturating)
    if key not in _frames:
        if saturating:
            q = synth.annex_k_qtabs(50)
            nb = synth.geometry(w, h, hs, vs)[3]
            coefs, qs = [synth.random_blocks(nb, 5 + i, -700, 700) for i in range(n)], [q] * n
        else:
            coefs, qs = zip(*[synth.synth_blocks(w, h, hs, vs, image_index=w + h + 7 * i) for i in range(n)])
        fulls = [_oracle_full(oracle, w, h, hs, vs, c, q) for c, q in zip(coefs, qs)]
        for f in fulls:
            assert f.shape == (h, w, 3)
            assert not saturating or ((f == 0).mean() >= 0.25 and (f == 255).mean() >= 0.25), ((f == 0).mean(), (f == 255).mean())
        _frames[key] = FilterSeam(jb, w, h, hs, vs, list(coefs), list(qs), pad_row=3, pad_plane=5, pad_img=7), fulls
    return _frames[key]


# ---- A. saturating content ---------------------------------------------------------------------------------------------
W, H = 130, 97
WHOLE = (0, 0, W, H)
INNER, STRIP = (32, 24, 65, 48), (3, 2, 60, 40)
# (rectangle, target, does a sum of the VERTICAL pass leave 0..255 under bicubic?).  The first three are the reductions
# and the near-identity the clamps were measured on; a reduction of this content averages so much that no final sum
# overshoots (whole frame -> 29 x 19: 0 of 1,653 outputs, in every layout), so two enlargements are added for the final clamp.
GEOMS = [(None, (29, 19), False), (INNER, (64, 50), True), (STRIP, (23, 17), False), (None, (173, 129), True), (STRIP, (64, 50), True)]
FULL_RANGE = [(INNER, (64, 50)), (None, (173, 129))]      # the expected image holds every value 0..255, under both filters


def _teeth(full, rect, target, filt, final):
    """Under bicubic the restatement without the clamp between the passes (and, `final`, with the low byte stored
    instead of the final clamp) computes another image than the true one: a kernel that lost a clamp fails the launch
    this precedes.  (Bilinear weights are not negative: it never overshoots.)  -> the true image"""
    want = pr.resize(full, rect, target, filt)
    for lost in ([dict(mid_clamp="none")] + ([dict(out_clamp="wrap")] if final else [])) if filt == BICUBIC else []:
        assert not np.array_equal(pr.resize(full, rect, target, filt, **lost), want), (rect, target, lost)
    if filt == BILINEAR:
        assert np.array_equal(pr.resize(full, rect, target, filt, mid_clamp="none", out_clamp="wrap"), want)
    return want


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("hs,vs", [(2, 2), (1, 1)])
def test_saturating_filter_every_format(jb, ctx, oracle, hs, vs, filt):
    """Half the pixels 0 and half 255: bicubic's overshoot reaches the clamp between the passes in every geometry and
    the final one in the enlargements, and the store sees every u8 value under every parameter set."""
    s, fulls = _frame(jb, oracle, W, H, hs, vs)
    finals = 0
    for rect, target, final in GEOMS:
        want = _teeth(fulls[0], rect, target, filt, final)
        finals += final
        if (rect, target) in FULL_RANGE:
            assert np.unique(want).size == 256
        for fmt, sb in FMT_CASES:
            _launch(s, ctx, [want], fmt, sb, rect=rect, target=target, filt=filt, tag=(hs, vs))
    assert finals >= 3


@pytest.mark.parametrize("hs,vs", LAYOUTS)
def test_saturating_bicubic_every_layout(jb, ctx, oracle, hs, vs):
    s, fulls = _frame(jb, oracle, W, H, hs, vs)
    want = _teeth(fulls[0], INNER, (64, 50), BICUBIC, True)
    assert np.unique(want).size == 256
    for fmt, sb in FMT_0_3:
        _launch(s, ctx, [want], fmt, sb, rect=INNER, target=(64, 50), filt=BICUBIC, tag=(hs, vs))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("hs,vs", [(2, 2), (1, 1)])
def test_saturating_filter_crops(jb, ctx, oracle, hs, vs, filt):
    """Three images, the three rectangles, one target: the clamps in the CROPS instantiations."""
    s, fulls = _frame(jb, oracle, W, H, hs, vs, n=3)
    crops = [WHOLE, INNER, STRIP]
    for target in ((64, 50), (23, 17)):
        want = [_teeth(f, r, target, filt, target == (64, 50) and r != WHOLE) for f, r in zip(fulls, crops)]
        if target == (64, 50):
            assert np.unique(want[1]).size == 256
        for fmt, sb in FMT_CASES:
            _launch(s, ctx, want, fmt, sb, target=target, filt=filt, crops=crops, tag=(hs, vs))


# the area kernel: enlarging (every u8 value in the expected image: asserted), reducing, one pixel.  65 x 48 -> 131 x 97 and
# not 130 x 97: at exactly 2 : 1 a row of this content blends so few pairs that the image holds some 80 values only.
AREA_ROUTES = {"resize": (None, None, [(173, 129), (29, 19), (1, 1)]),
               "roi": (INNER, None, [(131, 97), (29, 19), (1, 1)]),
               "crops": (None, [INNER, WHOLE, STRIP], [(131, 97), (29, 19), (1, 1)])}


@pytest.mark.parametrize("route", list(AREA_ROUTES))
@pytest.mark.parametrize("hs,vs", [(2, 2), (1, 1)])
def test_saturating_area_every_route(jb, ctx, oracle, hs, vs, route):
    rect, crops, targets = AREA_ROUTES[route]
    s, fulls = _frame(jb, oracle, W, H, hs, vs, n=3 if crops else 1)
    for k, target in enumerate(targets):
        want = _check(s, ctx, fulls, rect, target, AREA, FMT_0_3, crops=crops, tag=(hs, vs, route))
        if k == 0:     # the float formats' store saw every u, under F16_TIES too
            assert np.unique(want[0]).size == 256


# ---- B. the chunked passes at full workgroup height ------------------------------------------------------------------------
def _consts():
    """kFilterRows, kFilterLdsBytes and the tap cap, read out of the kernel's source: another value there changes the
    plans below and fails their assertions instead of quietly un-chunking the launches"""
    csrc = os.path.join(ROOT, "jpeg_decoder_amd", "csrc")
    hip = open(os.path.join(csrc, "jb_resample.hip")).read()
    rows = re.search(r"constexpr int kFilterRows = (\d+);", hip)
    lds = re.search(r"constexpr int kFilterLdsBytes = (\d+) << (\d+);", hip)
    cap = re.search(r"constexpr int kJbFilterMaxTaps = (\d+);", open(os.path.join(csrc, "jb_filter.h")).read())
    return int(rows[1]), int(lds[1]) << int(lds[2]), int(cap[1])


def _taps(filt, n_in, n_out):
    """the taps of an axis as the cap counts them: floor(2 * sup) + 2"""
    scale = n_in / n_out
    return int(2.0 * ((2.0 if filt == BICUBIC else 1.0) * (1.0 if scale < 1.0 else scale))) + 2


def _plan(filt, frame, rects, target):
    """filter_plan's arithmetic -> (tx_cap, ty_cap, span, t_rows): the maxima over the launch's rectangles"""
    R, lds, cap = _consts()
    tx_cap = ty_cap = span = 1
    for r in rects:
        tx, ty = _taps(filt, r[2], target[0]), _taps(filt, r[3], target[1])
        assert tx <= cap and ty <= cap, (r, tx, ty)
        tx_cap, ty_cap = max(tx_cap, tx), max(ty_cap, ty)
        span = max(span, min(int((R - 1) * (r[3] / target[1])) + ty + 2, pr.window(filt, frame[0], frame[1], r, target)[3]))
    fixed = (tx_cap * 64 + 64 + R * ty_cap + 2 * R) * 4
    return tx_cap, ty_cap, span, min(span, (lds - fixed) // 256)


def _workgroups(filt, frame_h, rect, oh, t_rows):
    """[(output rows, chunks, does a row's footprint straddle a chunk boundary)] of the workgroups of one tile column"""
    R = _consts()[0]
    ky = pr.axis_weights(filt, frame_h, rect[1], rect[1] + rect[3], oh)
    out = []
    for k0 in range(0, oh, R):
        rows = ky[k0:k0 + R]
        lo, hi = rows[0][0], rows[-1][0] + len(rows[-1][1])
        bounds = range(lo + t_rows, hi, t_rows)
        out.append((len(rows), len(bounds) + 1, any(a < b < a + len(k) for b in bounds for a, k in rows)))
    return out


# (frame height, layout, filter, target, ty taps, t_rows, chunks of the plan's span, chunks of the fullest workgroup)
CHUNKED = [(360, (2, 2), BILINEAR, (3, 9), 82, 226, 2, 2),
           (680, (1, 1), BILINEAR, (3, 9), 153, 217, 4, 3),
           (360, (2, 2), BICUBIC, (3, 17), 86, 210, 2, 2),
           (680, (1, 1), BICUBIC, (3, 18), 153, 201, 3, 3)]


@pytest.mark.parametrize("fh,layout,filt,target,ty,t_rows,plan_chunks,wg_chunks", CHUNKED)
def test_chunked_passes_with_eight_rows_per_workgroup(jb, ctx, oracle, fh, layout, filt, target, ty, t_rows, plan_chunks, wg_chunks):
    """24 x 360 and 24 x 680 to 9, 17 and 18 rows: the source rows of a workgroup's eight output rows do not fit LDS, so
    passes 2 and 3 run chunk by chunk with all eight accumulators live, footprints straddle the chunk boundaries, and
    the last workgroup has 1 (9, 17 rows) or 2 (18) rows."""
    R, _, cap = _consts()
    assert R == 8
    plan = _plan(filt, (24, fh), [(0, 0, 24, fh)], target)
    assert plan[1] == ty <= cap and plan[3] == t_rows < plan[2] and -(-plan[2] // t_rows) == plan_chunks, plan
    wgs = _workgroups(filt, fh, (0, 0, 24, fh), target[1], t_rows)
    assert wgs[0][0] == R and wgs[-1][0] == target[1] % R in (1, 2)
    assert max(c for n, c, _ in wgs if n == R) == wg_chunks >= 2 and any(st for n, c, st in wgs if n == R), wgs
    jb.filter_check(jb.make_desc(24, fh, *layout), target, filt)
    s, fulls = _frame(jb, oracle, 24, fh, *layout)
    _check(s, ctx, fulls, None, target, filt, FMT_0_3, tag=(fh, layout))


CHUNKED_CROPS = [(0, 0, 24, 680), (3, 5, 8, 8), (0, 300, 24, 80), (23, 679, 1, 1)]


@pytest.mark.parametrize("filt,target", [(BILINEAR, (3, 9)), (BICUBIC, (3, 18))])
def test_chunked_and_unchunked_images_in_one_crops_launch(jb, ctx, oracle, filt, target):
    """Four rectangles of the 24 x 680 frame in one launch: t_rows and the caps are the maxima over the launch, so the
    whole frame's workgroups are chunked and the 8 x 8 and 1 x 1 rectangles' run with tables and a T far larger than
    their own.  Image by image the bytes of the single-rectangle route.  (Bicubic: to 18 rows -- to 9 the whole frame
    wants 304 taps, which is refused.)"""
    fw, fh = 24, 680
    d = jb.make_desc(fw, fh, 1, 1)
    if filt == BICUBIC:
        with pytest.raises(jb.JbError) as e:
            jb.filter_check(d, (3, 9), BICUBIC, roi=CHUNKED_CROPS[0])
        assert e.value.status == -9 and _taps(BICUBIC, fh, 9) > _consts()[2]
    _, ty_cap, span, t_rows = _plan(filt, (fw, fh), CHUNKED_CROPS, target)
    assert ty_cap == 153 and t_rows < span
    chunks = [max(c for _, c, _ in _workgroups(filt, fh, r, target[1], t_rows)) for r in CHUNKED_CROPS]
    assert chunks[0] >= 2 and chunks[1:] == [1, 1, 1], chunks
    own = [_plan(filt, (fw, fh), [r], target) for r in CHUNKED_CROPS]
    assert all(p[3] == p[2] for p in own[1:]) and own[0][3] < own[0][2]      # alone, only the whole frame is chunked
    s, fulls = _frame(jb, oracle, fw, fh, 1, 1, n=4)
    for fmt, sb in FMT_0_3[:2]:
        want = [_ref(f, r, target, filt) for f, r in zip(fulls, CHUNKED_CROPS)]
        host, idx = _launch(s, ctx, want, fmt, sb, target=target, filt=filt, crops=CHUNKED_CROPS)
        for i, r in enumerate(CHUNKED_CROPS):
            jb.filter_check(d, target, filt, roi=r)
            one, at = _launch(s, ctx, [_ref(f, r, target, filt) for f in fulls], fmt, sb, rect=r, target=target, filt=filt)
            assert np.array_equal(host[idx[i]], one[at[i]]), (i, r, fmt)


@pytest.mark.parametrize("filt,target,lanes_of_last_tile", [(BILINEAR, (64, 2), 64), (BILINEAR, (65, 2), 1), (BICUBIC, (128, 2), 64)])
def test_full_column_table_next_to_the_tap_cap(jb, ctx, oracle, filt, target, lanes_of_last_tile):
    """5056 x 16 -> 64 and 128 columns: 160 taps per column, the cap itself, in all 64 lanes of a tile (the 1 x 1 targets
    reach the cap's neighbourhood with one live lane); -> 65 columns (157 taps) adds a tile with one live lane."""
    fw, fh = 5056, 16
    cap = _consts()[2]
    tx = _taps(filt, fw, target[0])
    assert tx == (cap if target[0] != 65 else 157) and (target[0] - 1) % 64 + 1 == lanes_of_last_tile
    d = jb.make_desc(fw, fh, 2, 2)
    jb.filter_check(d, target, filt)                           # accepted at exactly the cap
    assert jb.filter_window(d, target, filt) == pr.window(filt, fw, fh, (0, 0, fw, fh), target) == (0, 0, fw, fh)
    assert max(len(k) for _, k in pr.axis_weights(filt, fw, 0, fw, target[0])) >= tx - 2
    s, fulls = _frame(jb, oracle, fw, fh, 2, 2)
    _check(s, ctx, fulls, None, target, filt, FMT_0_3[:2])


# ---- C. frames at the size limit ---------------------------------------------------------------------------------------------
LIMIT = 65535


def _limit(jb, oracle, tall, n=1):
    """65535 x 9 4:2:0, or (tall) 9 x 65535 4:4:4, mid-grey noise; -> (seam, fulls, T): T turns a (long, short) pair or
    an (along, across, length, breadth) rectangle into the frame's (x, y[, w, h])"""
    T = (lambda a: a) if not tall else (lambda a: (a[1], a[0]) + ((a[3], a[2]) if len(a) == 4 else ()))
    s, fulls = _frame(jb, oracle, *T((LIMIT, 9)), *((1, 1) if tall else (2, 2)), n=n, saturating=False)
    return s, fulls, T


FAR = (LIMIT - 200, 0, 200, 9)       # the last 200 pixels of the long axis
LAST = (LIMIT - 1, 8, 1, 1)          # the last pixel


@pytest.mark.parametrize("tall", [False, True])
def test_limit_roi(jb, ctx, oracle, tall):
    s, fulls, T = _limit(jb, oracle, tall)
    for rect in (FAR, LAST):
        _check(s, ctx, fulls, T(rect), None, AREA, FMT_0_3[::2], tag=tall)


@pytest.mark.parametrize("tall", [False, True])
def test_limit_area(jb, ctx, oracle, tall):
    """The footprint arithmetic of jb_resample_kernel with 65535 on one side of its products."""
    s, fulls, T = _limit(jb, oracle, tall)
    for rect, target in ((None, (224, 5)), (None, (1, 1)), (FAR, (31, 7)), (LAST, (31, 7))):
        _check(s, ctx, fulls, rect and T(rect), T(target), AREA, FMT_0_3[::2], tag=tall)


@pytest.mark.parametrize("tall", [False, True])
def test_limit_filters(jb, ctx, oracle, tall):
    """The whole long axis to 840 (bilinear) and 1680 (bicubic) outputs: 158 taps each, the last footprints end at
    sample 65535; and the far end alone."""
    s, fulls, T = _limit(jb, oracle, tall)
    d = s.desc
    for filt, long in ((BILINEAR, 840), (BICUBIC, 1680)):
        assert _taps(filt, LIMIT, long) == 158 <= _consts()[2]
        for rect, target in ((None, (long, 5)), (FAR, (64, 9)), (LAST, (5, 3))):
            r, t = rect and T(rect), T(target)
            jb.filter_check(d, t, filt, roi=r)
            assert jb.filter_window(d, t, filt, roi=r) == pr.window(filt, *T((LIMIT, 9)), r or T((0, 0, LIMIT, 9)), t)
            _check(s, ctx, fulls, r, t, filt, FMT_0_3[::2], tag=tall)


@pytest.mark.parametrize("filt", (AREA,) + FILTERS)
@pytest.mark.parametrize("tall", [False, True])
def test_limit_crops(jb, ctx, oracle, tall, filt):
    s, fulls, T = _limit(jb, oracle, tall, n=3)
    crops = [T(r) for r in ((0, 0, 200, 9), FAR, (32000, 2, 300, 5))]
    _check(s, ctx, fulls, None, T((31, 7)), filt, FMT_0_3[::2], crops=crops, tag=tall)


# ---- D. a sweep of ratios over the device-computed weights -------------------------------------------------------------------
SW, SH = 97, 61
SWEEP_OW = (1, 2, 3, 5, 7, 8, 13, 31, 32, 33, 48, 49, 64, 65, 96, 97, 98, 127, 194, 195, 291)
SWEEP_RECTS = (None, (1, 1, 95, 59), (11, 7, 40, 29))


def _sweep_targets():
    return [(ow, (ow * 7) % 83 + 1) for ow in SWEEP_OW]


@pytest.mark.parametrize("filt", FILTERS)
def test_ratio_sweep(jb, ctx, oracle, filt):
    """21 targets x 3 rectangles of one saturating 97 x 61 frame: reductions up to the cap, identities, enlargements up to
    7 x, each with its own weights out of the device's fp64 arithmetic.  What the cap refuses is refused with -9 and
    nothing written -- and only that."""
    s, fulls = _frame(jb, oracle, SW, SH, 1, 1)
    cap = _consts()[2]
    ran = refused = 0
    for target in _sweep_targets():
        for rect in SWEEP_RECTS:
            x, y, w, h = rect or (0, 0, SW, SH)
            if max(_taps(filt, w, target[0]), _taps(filt, h, target[1])) > cap:
                s.catch, s.filter = True, filt
                try:
                    host, _ = s.run(ctx, 0, target, roi=rect, resize=target)
                    assert s.error is not None and s.error.status == -9 and str(cap) in str(s.error), (rect, target, s.error)
                    assert (host == SENT).all()
                finally:
                    s.catch, s.filter = False, 0
                refused += 1
                continue
            _check(s, ctx, fulls, rect, target, filt, FMT_CASES[:1], tag="sweep")
            ran += 1
    # refused: the whole frame's and the 95 x 59 rectangle's 1-column targets under bilinear (196 and 192 taps); under
    # bicubic their 1- and 2-column targets (390, 382, 196, 192) and the 40 x 29 rectangle's 1-column one (162)
    assert ran + refused == 63 and refused == (2 if filt == BILINEAR else 5), (ran, refused)


def test_ratio_sweep_equals_pillow(jb, ctx, oracle):
    Image = pytest.importorskip("PIL.Image")
    s, fulls = _frame(jb, oracle, SW, SH, 1, 1)
    targets = _sweep_targets()
    for filt, resample in ((BILINEAR, Image.BILINEAR), (BICUBIC, Image.BICUBIC)):
        for target, rect in ((targets[4], SWEEP_RECTS[0]), (targets[11], SWEEP_RECTS[1]), (targets[20], SWEEP_RECTS[2])):
            x, y, w, h = rect or (0, 0, SW, SH)
            want = np.asarray(Image.fromarray(fulls[0]).resize(target, resample, box=(x, y, x + w, y + h)))
            _launch(s, ctx, [want], 0, NO_PARAMS, rect=rect, target=target, filt=filt, tag="pillow")
