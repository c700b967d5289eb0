"""JB_COLOR_BLUR on the GPU (-m gpu): jb_color_blur_kernel -- a 64 x 32 tile with a halo of 3 (r + 1) samples, six passes in
LDS -- against jb_color_host (the same csrc/jb_color_core.h on the CPU, itself pinned to Pillow by tests/test_blur_cpu.py),
against the numpy restatement tests/blur_ref.py where the view's border is the point, and against Pillow's recorded answers
(tests/golden/blur_kat.npz).  The shapes are chosen for where a tile kernel goes wrong: views smaller than one halo, narrower
than a halo and taller than a tile, three ragged tiles each way; box radii 0, 1 and 7, through both instantiations of the
kernel (the halo for r <= 1 and the one for r <= 7).  At the seam and in the batch decoder the definition is checked:

    out(i, v) = to_format(color_host(u, chain[i][v]), fmt, scale, bias)

with u what THE SAME CALL WITHOUT colors= writes in format 0.  Every comparison is bit-exact, and for color_device the whole
sentinel-filled buffer is compared, pads included."""
import os

import numpy as np
import pytest

import blur_ref as BR
import color_ref as R
import format_ref as fr
from conftest import GOLD
from seam_harness import SENT
from test_gpu_color import (FILES, FILE_VIEWS, SEAM_VIEWS, _params, _seam, _u8_views, _views_call, check_color_device, color_device)
from test_gpu_view_groups import run_groups
from test_gpu_views import BT, _gold

pytestmark = pytest.mark.gpu

B, C, S, H, G, Z, BLUR = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE, BR.BLUR
AREA, BILINEAR, BICUBIC = 0, 1, 2
R0, R1, R7 = 0.5, 2.0, 8.0                       # Gaussian radii whose box radius is 0, 1 and 7
TILE = (64, 32)                                   # jb_color_blur_kernel's


@pytest.fixture(scope="module")
def jb():
    import jpeg_decoder_amd as jb
    assert jb.lib().jb_device_count() >= 1, jb.lib().jb_last_error(None)
    assert [jb.blur_params(x)[0] for x in (R0, R1, R7)] == [0, 1, 7]
    return jb


@pytest.fixture(scope="module")
def ctx(jb):
    c = jb.Context(0)
    yield c
    c.close()


def content(w, h, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    u = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    u[:, w // 2:] = np.where(rng.random((h, w - w // 2, 3)) < 0.5, 0, 255)
    return u


def check(jb, ctx, images, chains, fmts=(0, 1, 2, 3), wants=None, **kw):
    wants = wants if wants is not None else [jb.color_host(u, c) for u, c in zip(images, chains)]
    for fmt in fmts:
        check_color_device(jb, ctx, images, chains, fmt, wants=wants, **kw)
    return wants


# smaller than one halo; narrower than a halo and taller than a tile; the KAT's size; three tiles each way, ragged in both
SIZES = [(1, 1), (2, 3), (5, 4), (3, 97), (61, 47), (2 * TILE[0] + 11, 2 * TILE[1] + 7)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_blur_alone_sizes_strides_and_formats(jb, ctx, size):
    w, h = size
    images = [content(w, h, i) for i in range(2)]
    # the kernel with the small halo (every r <= 1), then the one with the large halo (an r = 7 in the launch) on r = 7 and 1
    for radii in ((R0, R1), (R7, R1)):
        chains = [[(BLUR, x)] for x in radii]
        wants = check(jb, ctx, images, chains, pads=(13, 7, 77), in_pads=(5, 11))
        assert all(np.array_equal(w_, BR.gaussian_blur(u, x)) for w_, u, x in zip(wants, images, radii))
    check(jb, ctx, images[:1], [[(BLUR, R1)]], fmts=(0,))                  # one image, tight, its strides unused


def test_blur_alone_224(jb, ctx):
    u = content(224, 224)
    check(jb, ctx, [u, u, u], [[(BLUR, R0)], [(BLUR, R1)], [(BLUR, 0.0)]], fmts=(3,), pads=(3, 5, 7))
    check(jb, ctx, [u], [[(BLUR, R7)]], fmts=(3,))
    assert np.array_equal(jb.color_host(u, [(BLUR, 0.0)]), u)


def test_border_band(jb, ctx):
    """a steep ramp from left to right and from top to bottom: the outermost 24 rows and columns are where a halo replicated
    ONCE, in front of six unclamped passes, differs from Pillow's clamp in every pass"""
    w, h = 150, 101
    y, x = np.mgrid[0:h, 0:w]
    u = np.stack([np.clip(9 * x + 3 * y, 0, 255), np.clip(255 - 7 * x + 11 * (h - 1 - y), 0, 255) & 255, (13 * x + 17 * y) & 255], -1).astype(np.uint8)
    for radius in (R0, 1.0, R1, 3.7, R7):
        want = BR.gaussian_blur(u, radius)
        # what a pre-replicated halo would give differs from it in the band: the check can see the mistake
        pad = np.pad(u, ((24, 24), (24, 24), (0, 0)), mode="edge")
        assert not np.array_equal(BR.gaussian_blur(pad, radius)[24:-24, 24:-24], want)
        host, idx, _ = color_device(jb, ctx, [u], [[(BLUR, radius)]], 0)
        got = host[idx[0]].reshape(h, w, 3)
        band = np.ones((h, w), bool)
        band[24:-24, 24:-24] = False
        assert np.array_equal(got[band], want[band]), radius
        assert np.array_equal(got, want), radius


def test_blur_gives_pillows_recorded_answers(jb, ctx):
    z = np.load(os.path.join(GOLD, "blur_kat.npz"))
    chains = [[(int(op), float(v)) for op, v in rows if int(op) != 0] for rows in z["chains"]]
    wants = list(z["out"])
    assert len(chains) >= 16
    check(jb, ctx, [z["image"]] * len(chains), chains, wants=wants, pads=(3, 5, 7))
    # the chains with r <= 1 on their own: the kernel with the small halo
    small = [i for i, c in enumerate(chains) if all(op != BLUR or jb.blur_params(v)[0] <= 1 for op, v in c)]
    assert 10 <= len(small) < len(chains)
    check(jb, ctx, [z["image"]] * len(small), [chains[i] for i in small], wants=[wants[i] for i in small], pads=(3, 5, 7))


def _mixed_chains():
    chains = []
    for i in range(33):
        radius = (0.3, 1.1, 2.0, 1.7, 4.2, 8.0, 0.0)[i % 7]
        chains.append([[(B, 0.6 + 0.03 * i), (H, (7 * i) % 256)],                                   # no blur
                       [(BLUR, radius)],                                                           # blur only
                       [(S, 0.5 + 0.04 * i), (H, (11 * i) % 256), (BLUR, radius)],                 # prefix + blur
                       [(C, 0.5 + 0.05 * i), (G, 0), (BLUR, radius), (Z, 128)],                    # DINO's longest shape
                       []][i % 5])
    chains[32] = [(C, 1.3), (BLUR, 1.0), (Z, 100)]          # the second launch: one view, the small halo
    return chains


def test_33_views_in_one_call_with_and_without_a_blur(jb, ctx):
    """two launches (32 + 1); views with and without a blur side by side -- each kernel returns early on the other's -- with a
    radius per view and the contrast's reduction pass in front of some"""
    chains = _mixed_chains()
    kinds = [(BLUR in [op for op, _ in c], C in [op for op, _ in c]) for c in chains]
    assert set(kinds) == {(False, False), (True, False), (True, True)}
    assert {jb.blur_params(v)[0] for c in chains for op, v in c if op == BLUR} >= {0, 1, 3, 7}
    images = [content(67, 39, i) for i in range(33)]          # two tiles each way, ragged
    check(jb, ctx, images, chains, fmts=(0, 3), pads=(1, 2, 3))


def test_blur_is_identical_from_run_to_run(jb, ctx):
    u = content(224, 224, 5)
    chain = [(B, 1.1), (C, 1.3), (BLUR, 1.5), (Z, 128)]
    a, idx, _ = color_device(jb, ctx, [u], [chain], 3, fr.IMAGENET)
    b, _, _ = color_device(jb, ctx, [u], [chain], 3, fr.IMAGENET)
    assert np.array_equal(a, b) and not (a[idx[0]] == SENT).all()


def test_blur_refusals_launch_and_write_nothing(jb, ctx):
    u = np.zeros((5, 6, 3), np.uint8)
    nan, inf = float("nan"), float("inf")
    for bad, status in (([(BLUR, -1.0)], -2), ([(BLUR, nan)], -2), ([(BLUR, inf)], -2), ([(BLUR, 9.0)], -9),
                        ([(BLUR, 1.0), (BLUR, 1.0)], -9), ([(BLUR, 1.0), (C, 1.0)], -9), ([(BLUR, 1.0), (C, 1.0), (H, 300)], -2)):
        host, _, err = color_device(jb, ctx, [u, u], [[(BLUR, 1.0)], bad], 3, fr.IMAGENET, catch=True)
        assert err is not None and err.status == status and "colour chain 1" in str(err), (bad, err)
        assert (host == SENT).all()


# ---- the seam ---------------------------------------------------------------------------------------------------------------
SIZE = (679, 451)
BLUR_CHAINS = [[[(B, 1.3), (C, 0.7), (S, 1.2), (H, 20), (BLUR, 1.3)], [(BLUR, 0.4)], [(G, 0), (BLUR, 1.9), (Z, 128)]],
               [[(H, 240), (S, 0.4)], [(BLUR, 2.0), (S, 1.8)], None]]
GROUPS = [(2, (224, 224)), (3, (96, 96), BICUBIC)]
GROUP_VIEWS = [SEAM_VIEWS[SIZE][0][:2] + SEAM_VIEWS[SIZE][1], SEAM_VIEWS[SIZE][1][:2] + SEAM_VIEWS[SIZE][0]]
GROUP_CHAINS = [BLUR_CHAINS[0][:2] + BLUR_CHAINS[1], [[(C, 0.3), (BLUR, 0.9)], [(Z, 10), (BLUR, 3.0)]] + BLUR_CHAINS[0]]


def _check_views(jb, s, c, target, filt):
    views = SEAM_VIEWS[SIZE]
    n_out = s.n * len(views[0])
    plain, pidx = s.run_outputs(c, 0, target, n_out, _views_call(views, target, filt, None))
    us = [plain[pidx[n]].reshape(target[1], target[0], 3) for n in range(n_out)]
    refs = [jb.color_host(u, chain) for u, chain in zip(us, [chain for row in BLUR_CHAINS for chain in row])]
    assert sum(not np.array_equal(r, u) for r, u in zip(refs, us)) >= 4
    for fmt in (0, 3):
        sb = _params(fmt)
        host, idx = s.run_outputs(c, fmt, target, n_out, _views_call(views, target, filt, BLUR_CHAINS), sb)
        want = np.full(host.size, SENT, np.uint8)
        for n, ref in enumerate(refs):
            want[idx[n]] = fr.bits(fr.to_format(ref, fmt, *sb)).view(np.uint8).reshape(idx[n].shape)
        bad = np.flatnonzero(host != want)
        assert bad.size == 0, (fmt, filt, bad.size, int((~np.isin(bad, idx.ravel())).sum()), "bytes differ / of them outside the outputs")


def _check_groups(jb, s, c):
    plain, play = run_groups(s, c, 0, GROUP_VIEWS, GROUPS)
    for fmt in (0, 3):
        sb = _params(fmt)
        hosts, lay = run_groups(s, c, fmt, GROUP_VIEWS, GROUPS, sb,
                                call=lambda c_, b, spec, outs: c_.blocks_to_rgb_device(b, fmt=spec, views=GROUP_VIEWS, view_groups=GROUPS,
                                                                                       view_outputs=outs, colors=GROUP_CHAINS))
        wants = [np.full(h.size, SENT, np.uint8) for h in hosts]
        first = 0
        for g, grp in enumerate(GROUPS):
            k, (w, h) = grp[0], grp[1]
            for i in range(s.n):
                for v in range(k):
                    u = plain[play.buf_of[g]][play.idx[g][i, v]].reshape(h, w, 3)
                    ref = fr.to_format(jb.color_host(u, GROUP_CHAINS[i][first + v]), fmt, *sb)
                    wants[lay.buf_of[g]][lay.idx[g][i, v]] = fr.bits(ref).view(np.uint8).reshape(lay.idx[g][i, v].shape)
            first += k
        for host, want in zip(hosts, wants):
            assert np.array_equal(host, want), (fmt, int((host != want).sum()))


@pytest.mark.parametrize("arith", ["reference", "libjpeg"])
def test_seam_views_and_view_groups_with_a_blur(jb, arith):
    s = _seam(jb, SIZE)
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG if arith == "libjpeg" else jb.ARITH_REFERENCE) as c:
        _check_views(jb, s, c, (224, 224), AREA)
        _check_views(jb, s, c, (96, 96), BICUBIC)
        _check_groups(jb, s, c)


# ---- the batch decoder ------------------------------------------------------------------------------------------------------
def test_batch_decoder_with_dino_augment(jb):
    import torch
    from jpeg_decoder_amd.color import dino_augment
    paths = [_gold(n)[0] for n in FILES]
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    rng = np.random.default_rng(21)
    chains = [[dino_augment(rng, v) for v in range(2)] for _ in FILES]
    assert all(BLUR in [op for op, _ in row[0]] for row in chains)           # the first global view is always blurred
    assert any(C in [op for op, _ in row[0]] for row in chains)
    us = _u8_views(jb, paths, FILE_VIEWS, resize=BT)
    want = np.stack([np.stack([fr.to_format(jb.color_host(u, c), spec.format, list(spec.scale), list(spec.bias)) for u, c in zip(ku, kc)])
                     for ku, kc in zip(us, chains)])
    with jb.BatchDecoder(4, 0, resize=BT, fmt=spec) as dec:
        out = torch.full((len(paths), 2, 3, BT[1], BT[0]), 7.0, dtype=torch.float16, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(paths, out, views=FILE_VIEWS, colors=chains)
        assert ret is out and tm["rc"] == 0 and st == [0] * len(paths)
        assert fr.same_bits(out.cpu().numpy(), want)
        # a chain with a contrast behind its blur refuses the whole call: the tensor keeps its bytes
        broken = [list(r) for r in chains]
        broken[6][1] = [(BLUR, 1.0), (C, 1.0)]
        out.fill_(7.0)
        ret, st, tm = dec.run_to_tensor(paths, out, views=FILE_VIEWS, colors=broken)
        assert tm["rc"] == -9 and bool((out == 7.0).all())
