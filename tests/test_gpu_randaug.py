"""The RandAugment colour operations on the GPU (-m gpu): JB_COLOR_POSTERIZE / _INVERT / _AUTOCONTRAST / _EQUALIZE /
_SHARPNESS through Context.color_device -- jb_color_hist_kernel and jb_color_table_kernel in up to two rounds in front of the
apply, blur and sharpness kernels -- against the numpy restatement tests/randaug_ref.py and Pillow's recorded answers
(tests/golden/randaug_kat.npz).  The shapes are chosen for where the kernels go wrong: views without an interior, one filtered
pixel, one past a 64 x 32 tile both ways, one past the apply kernel's 256 columns; every (lo, hi) pair of the device's fp64
table; counts far above 16 bits; the equalize clip.  At the seam and in the batch decoder the definition is checked:

    out(i, v) = to_format(randaug_ref.apply_chain(u, chain[i][v]), fmt, scale, bias)

with u what THE SAME CALL WITHOUT colors= writes in format 0.  Every comparison is bit-exact, and for color_device the whole
sentinel-filled buffer is compared, pads included."""
import os

import numpy as np
import pytest

import blur_ref as BR
import color_ref as R
import format_ref as fr
import randaug_ref as RA
from conftest import GOLD
from seam_harness import SENT
from test_gpu_color import (FILES, FILE_VIEWS, GROUPS, GROUP_VIEWS, SEAM_VIEWS, TARGET, _params, _seam, _u8_views, _views_call, check_color_device,
                            color_device)
from test_gpu_view_groups import run_groups
from test_gpu_views import BT, _gold

pytestmark = pytest.mark.gpu

B, C, S, H, G, Z, BLUR = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE, BR.BLUR
P, I, A, E, SH = RA.POSTERIZE, RA.INVERT, RA.AUTOCONTRAST, RA.EQUALIZE, RA.SHARPNESS
AREA, BILINEAR, BICUBIC = 0, 1, 2


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


def content(w, h, seed=0):
    """random content in a narrow range per channel (so that autocontrast moves it), the right half few-valued"""
    rng = np.random.default_rng(1000 * w + h + seed)
    u = rng.integers(30 + seed % 5, 180 + 7 * (seed % 9), (h, w, 3), dtype=np.uint8)
    u[:, w // 2:] = rng.choice(np.array([12, 13, 100, 240], np.uint8), (h, w - w // 2, 3))
    return u


def check(jb, ctx, images, chains, fmts=(0, 1, 2, 3), wants=None, **kw):
    wants = wants if wants is not None else [RA.apply_chain(u, c) for u, c in zip(images, chains)]
    for fmt in fmts:
        check_color_device(jb, ctx, images, chains, fmt, wants=wants, **kw)
    return wants


# views without an interior; one filtered pixel; odd; one past a 64 x 32 tile both ways; one past 256 columns; a model's input
SIZES = [(1, 1), (2, 1), (3, 1), (2, 2), (3, 3), (7, 13), (97, 3), (65, 33), (257, 5), (224, 224)]
SIZE_CHAINS = [[(P, 3), (I, 0)], [(A, 0)], [(E, 0)], [(SH, 1.6)], [(SH, 0.3)], [(E, 0), (C, 1.3), (SH, 0.4), (Z, 128)],
               [(B, 0.8), (A, 0), (S, 1.2), (E, 0)], [(H, 30), (SH, 1.9), (P, 5)], []]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_sizes_strides_and_formats(jb, ctx, size):
    w, h = size
    images = [content(w, h, i) for i in range(len(SIZE_CHAINS))]
    wants = check(jb, ctx, images, SIZE_CHAINS, pads=(13, 7, 77), in_pads=(5, 11))
    if w * h >= 91:
        assert sum(not np.array_equal(a, b) for a, b in zip(wants, images)) >= len(SIZE_CHAINS) - 2
    check(jb, ctx, images[3:4], SIZE_CHAINS[3:4], fmts=(0,), wants=wants[3:4])          # one image, tight, its strides unused


def test_pillows_recorded_answers(jb, ctx):
    z = np.load(os.path.join(GOLD, "randaug_kat.npz"))
    chains = [[(int(op), float(v)) for op, v in rows if int(op) != 0] for rows in z["chains"]]
    assert len(chains) >= 24
    check(jb, ctx, [z["image"]] * len(chains), chains, wants=list(z["out"]), pads=(3, 5, 7))


def test_every_autocontrast_pair_on_the_device(jb, ctx):
    """all 32,640 (lo, hi), three a view (one per channel): views of 256 x 1 holding clip(arange(256), lo, hi), so the view
    shows the whole table between lo and hi; the reference is the fp64 definition, evaluated by numpy in float64"""
    pairs = np.array([(lo, hi) for lo in range(256) for hi in range(lo + 1, 256)], np.int64)
    assert pairs.shape == (32640, 2)
    lo, hi = pairs[:, 0], pairs[:, 1]
    scale = 255.0 / (hi - lo).astype(np.float64)
    offset = -lo.astype(np.float64) * scale
    t = np.arange(256, dtype=np.float64)[None, :] * scale[:, None]
    t = t + offset[:, None]
    luts = np.clip(np.trunc(t), 0, 255).astype(np.uint8)                               # [32640, 256]
    for k in (0, 1, 254, 255, 4321, 32639):
        h = [0] * 256
        h[lo[k]] = h[hi[k]] = 1
        assert luts[k].tolist() == RA.autocontrast_lut(h)
    ramp = np.clip(np.arange(256)[None, :], lo[:, None], hi[:, None])                  # [32640, 256]
    views = ramp.reshape(10880, 3, 256).transpose(0, 2, 1)[:, None].astype(np.uint8)   # [10880, 1, 256, 3]
    wants = np.take_along_axis(luts, ramp, 1).reshape(10880, 3, 256).transpose(0, 2, 1)[:, None]
    for first in range(0, 10880, 2720):
        part = slice(first, first + 2720)
        check(jb, ctx, list(views[part]), [[(A, 0)]] * 2720, fmts=(0,), wants=list(wants[part]))


def test_counts_far_above_16_bits(jb, ctx):
    rng = np.random.default_rng(1024)
    two = np.where(rng.random((1024, 1024, 3)) < 0.3, 17, 230).astype(np.uint8)
    rnd = rng.integers(5, 250, (1024, 1024, 3), dtype=np.uint8)
    counts = RA.counts(two)
    assert min(c for c in counts[0] if c) > 1 << 16 and (sum(counts[0]) - counts[0][230]) // 255 > 1000     # step is large
    wants = check(jb, ctx, [two, rnd], [[(E, 0)], [(A, 0), (B, 0.9), (E, 0)]], fmts=(0,))
    assert not np.array_equal(wants[0], two) and not np.array_equal(wants[1], rnd)


def test_the_equalize_clip_case(jb, ctx):
    h = [2] * 150 + [0] * 105 + [3]
    assert RA.equalize_overshoots(h) and max(RA.equalize_lut(h)) == 255
    line = np.repeat(np.arange(256), h).astype(np.uint8)
    u = np.stack([line, line[::-1], np.roll(line, 7)], -1)[None]                      # [1, 303, 3]
    want = check(jb, ctx, [u, u], [[(E, 0)], [(E, 0), (I, 0)]])
    assert want[0].max() == 255 and not np.array_equal(want[0], u)


def _pairs_of_statistics():
    kinds = [(x, y) for x in (C, A, E) for y in (C, A, E) if (x, y) != (C, C)]
    value = {C: 1.3, A: 0, E: 0}
    chains = []
    for i, (x, y) in enumerate(kinds):
        between = [[(B, 0.8)], [(S, 1.4), (P, 5)], [(H, 40)], []][i % 4]
        base = [(B, 1.1)] * (i % 2) + [(x, value[x])] + between + [(y, value[y])]
        chains += [base + [(I, 0)], base + [(Z, 100), (BLUR, (0.7, 2.0, 5.0)[i % 3]), (P, 6)], base + [(S, 0.7), (SH, (1.8, 0.2)[i % 2]), (Z, 128)]]
    return kinds, chains


def test_two_statistics_operations_in_every_order(jb, ctx):
    kinds, chains = _pairs_of_statistics()
    assert len(kinds) == 8 and len(chains) == 24
    jb.color_check(chains)
    images = [content(67, 39, i) for i in range(len(chains))]                          # two tiles each way, ragged
    check(jb, ctx, images, chains, fmts=(0, 3), pads=(1, 2, 3))


def _mixed_chains():
    shapes = [lambda i: [(B, 0.6 + 0.03 * i), (H, (7 * i) % 256)],                                         # none of the new kernels
              lambda i: [(E, 0)],
              lambda i: [(P, 1 + i % 7), (A, 0), (C, 0.5 + 0.05 * i)],
              lambda i: [(SH, 0.1 * i)],
              lambda i: [(C, 0.7 + 0.02 * i), (G, 0), (BLUR, (0.3, 1.1, 4.2)[i % 3]), (Z, 128)],           # DINO's longest shape
              lambda i: [(S, 0.5 + 0.04 * i), (E, 0), (I, 0), (A, 0), (SH, 1.0 + 0.05 * i), (P, 6)],
              lambda i: [],
              lambda i: [(C, 1.2), (SH, 1.5)],
              lambda i: [(I, 0), (P, 4)]]
    chains = [shapes[i % len(shapes)](i) for i in range(33)]
    chains[32] = [(A, 0), (E, 0)]                  # the second launch: one view, two rounds of histograms, no mean
    return chains


def test_33_views_in_one_call_of_mixed_kinds(jb, ctx):
    """two launches (32 + 1); views with no, one and two statistics operations and with each neighbourhood kernel side by side:
    every kernel returns early on the others' views, and the second launch has no contrast at all"""
    chains = _mixed_chains()
    n_stats = {sum(op in (C, A, E) for op, _ in c) for c in chains}
    assert n_stats == {0, 1, 2} and {op for c in chains for op, _ in c} >= {P, I, A, E, SH, BLUR, C}
    images = [content(67, 39, i) for i in range(33)]
    check(jb, ctx, images, chains, fmts=(0, 3), pads=(1, 2, 3))


def test_identical_from_run_to_run(jb, ctx):
    u = content(224, 224, 5)
    chain = [(B, 1.1), (E, 0), (C, 1.3), (SH, 1.5), (Z, 128)]
    a, idx, _ = color_device(jb, ctx, [u, u], [chain, [(A, 0), (E, 0)]], 3, fr.IMAGENET)
    b, _, _ = color_device(jb, ctx, [u, u], [chain, [(A, 0), (E, 0)]], 3, fr.IMAGENET)
    assert np.array_equal(a, b) and not (a[idx[0]] == SENT).all()


def test_refusals_launch_and_write_nothing(jb, ctx):
    u = np.zeros((5, 6, 3), np.uint8)
    nan = float("nan")
    for bad, status in (([(P, 9)], -2), ([(P, 1.5)], -2), ([(I, 1)], -2), ([(A, nan)], -2), ([(E, 2)], -2), ([(SH, -1.0)], -2), ([(SH, nan)], -2),
                        ([(A, 0), (E, 0), (C, 1.0)], -9), ([(SH, 1.0), (SH, 1.0)], -9), ([(BLUR, 1.0), (SH, 1.0)], -9), ([(SH, 1.0), (E, 0)], -9),
                        ([(SH, 1.0), (A, 0), (H, 300)], -2)):
        host, _, err = color_device(jb, ctx, [u, u], [[(E, 0), (SH, 1.0)], bad], 3, fr.IMAGENET, catch=True)
        assert err is not None and err.status == status and "colour chain 1" in str(err), (bad, err)
        assert (host == SENT).all()


# ---- the seam ---------------------------------------------------------------------------------------------------------------
SEAM_CHAINS = [[[(B, 1.3), (E, 0), (S, 1.2), (C, 0.7), (SH, 1.6)], [(A, 0)], [(G, 0), (P, 3), (SH, 0.2), (Z, 128)]],
               [[(H, 240), (A, 0), (I, 0), (E, 0)], [(SH, 1.9), (S, 1.8)], None]]
GROUP_CHAINS = [SEAM_CHAINS[0][:2] + SEAM_CHAINS[1], [[(C, 0.3), (E, 0), (BLUR, 0.9)], [(Z, 10), (P, 2)]] + SEAM_CHAINS[0]]


@pytest.mark.parametrize("filt", [AREA, BICUBIC], ids=["area", "bicubic"])
@pytest.mark.parametrize("size", list(SEAM_VIEWS), ids=lambda s: "%dx%d" % s)
def test_seam_views_with_the_new_operations(jb, ctx, size, filt):
    s, views = _seam(jb, size), SEAM_VIEWS[size]
    n_out = s.n * len(views[0])
    plain, pidx = s.run_outputs(ctx, 0, TARGET, n_out, _views_call(views, TARGET, filt, None))
    us = [plain[pidx[n]].reshape(TARGET[1], TARGET[0], 3) for n in range(n_out)]
    refs = [RA.apply_chain(u, chain) for u, chain in zip(us, [chain for row in SEAM_CHAINS for chain in row])]
    assert sum(not np.array_equal(r, u) for r, u in zip(refs, us)) >= 4
    for fmt in (0, 1, 2, 3):
        sb = _params(fmt)
        host, idx = s.run_outputs(ctx, fmt, TARGET, n_out, _views_call(views, TARGET, filt, SEAM_CHAINS), sb)
        want = np.full(host.size, SENT, np.uint8)
        for n, ref in enumerate(refs):
            want[idx[n]] = fr.bits(fr.to_format(ref, fmt, *sb)).view(np.uint8).reshape(idx[n].shape)
        bad = np.flatnonzero(host != want)
        assert bad.size == 0, (fmt, filt, bad.size, int((~np.isin(bad, idx.ravel())).sum()), "bytes differ / of them outside the outputs")


def test_seam_view_groups_with_the_new_operations(jb, ctx):
    s = _seam(jb, (679, 451))
    plain, play = run_groups(s, ctx, 0, GROUP_VIEWS, GROUPS)
    for fmt in (0, 3):
        sb = _params(fmt)
        hosts, lay = run_groups(s, ctx, fmt, GROUP_VIEWS, GROUPS, sb,
                                call=lambda c_, b, spec, outs: c_.blocks_to_rgb_device(b, fmt=spec, views=GROUP_VIEWS, view_groups=GROUPS,
                                                                                       view_outputs=outs, colors=GROUP_CHAINS))
        wants = [np.full(h.size, SENT, np.uint8) for h in hosts]
        first = 0
        for g, grp in enumerate(GROUPS):
            k, (w, h) = grp[0], grp[1]
            for i in range(s.n):
                for v in range(k):
                    u = plain[play.buf_of[g]][play.idx[g][i, v]].reshape(h, w, 3)
                    ref = fr.to_format(RA.apply_chain(u, GROUP_CHAINS[i][first + v]), fmt, *sb)
                    wants[lay.buf_of[g]][lay.idx[g][i, v]] = fr.bits(ref).view(np.uint8).reshape(lay.idx[g][i, v].shape)
            first += k
        for host, want in zip(hosts, wants):
            assert np.array_equal(host, want), (fmt, int((host != want).sum()))


# ---- the batch decoder ------------------------------------------------------------------------------------------------------
def test_batch_decoder_with_rand_augment(jb):
    import torch
    from jpeg_decoder_amd.color import rand_augment_color, trivial_augment_wide_color
    paths = [_gold(n)[0] for n in FILES]
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    rng = np.random.default_rng(9)
    chains = [[rand_augment_color(rng, 3, 9 + 2 * i), trivial_augment_wide_color(rng)] for i in range(len(FILES))]
    chains[0][0] = [(E, 0), (C, 1.27), (SH, 1.27)]                        # (whatever the draws: every new kernel runs)
    chains[3][1] = [(P, 4), (A, 0)]
    us = _u8_views(jb, paths, FILE_VIEWS, resize=BT)
    want = np.stack([np.stack([fr.to_format(RA.apply_chain(u, c), spec.format, list(spec.scale), list(spec.bias)) for u, c in zip(ku, kc)])
                     for ku, kc in zip(us, chains)])
    with jb.BatchDecoder(4, 0, resize=BT, fmt=spec) as dec:
        out = torch.full((len(paths), 2, 3, BT[1], BT[0]), 7.0, dtype=torch.float16, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(paths, out, views=FILE_VIEWS, colors=chains)
        assert ret is out and tm["rc"] == 0 and st == [0] * len(paths)
        assert fr.same_bits(out.cpu().numpy(), want)
        # a chain with a statistics operation behind its sharpness refuses the whole call: the tensor keeps its bytes
        broken = [list(r) for r in chains]
        broken[6][1] = [(SH, 1.0), (E, 0)]
        out.fill_(7.0)
        ret, st, tm = dec.run_to_tensor(paths, out, views=FILE_VIEWS, colors=broken)
        assert tm["rc"] == -9 and bool((out == 7.0).all())
