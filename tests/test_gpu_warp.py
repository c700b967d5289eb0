"""The geometric operations of the colour chains on the GPU (-m gpu): JB_COLOR_SHEAR_X / _SHEAR_Y / _TRANSLATE_X /
_TRANSLATE_Y / _ROTATE through Context.color_device -- jb_color_warp_table_kernel, then the WARP instantiations of the mean,
histogram, apply, blur and sharpness kernels, whose every pixel load is jbc_gather -- against jb_color_host (the same
csrc/jb_color_core.h on the CPU; tests/test_warp_cpu.py holds it to the numpy restatement and to Pillow) and against Pillow's
recorded answers (tests/golden/warp_kat.npz).  The sizes cross the apply kernel's 256 columns and 4 rows and the 64 x 32 tiles of
the blur and sharpness kernels.  At the seam and in the batch decoder the definition is checked:

    out(i, v) = to_format(warp_ref.apply_chain(u, chain[i][v]), fmt, scale, bias)

with u what THE SAME CALL WITHOUT colors= writes in format 0.  Every comparison is bit-exact, and for color_device the whole
sentinel-filled buffer is compared, pads included."""
import os

import numpy as np
import pytest

import blur_ref as BR
import color_ref as R
import format_ref as fr
import randaug_ref as RA
import warp_ref as WR
from conftest import GOLD
from seam_harness import SENT
from test_gpu_color import (FILES, FILE_VIEWS, GROUPS, GROUP_VIEWS, SEAM_VIEWS, TARGET, _params, _seam, _u8_views, _views_call, check_color_device,
                            color_device)
from test_gpu_view_groups import run_groups
from test_gpu_views import BT, _gold

pytestmark = pytest.mark.gpu

B, C, S, H, G, Z, BLUR = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE, BR.BLUR
P, I, A, E, SH = RA.POSTERIZE, RA.INVERT, RA.AUTOCONTRAST, RA.EQUALIZE, RA.SHARPNESS
SX, SY, TX, TY, ROT = WR.SHEAR_X, WR.SHEAR_Y, WR.TRANSLATE_X, WR.TRANSLATE_Y, WR.ROTATE
AREA, BICUBIC = 0, 2


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
    """random content without black (a filled pixel is told from a copied one), a narrow range in the left half (so that
    autocontrast moves it)"""
    rng = np.random.default_rng(1000 * w + h + seed)
    u = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
    u[:, :w // 2] = rng.integers(40 + seed % 5, 170, (h, w // 2, 3), dtype=np.uint8)
    return u


def check(jb, ctx, images, chains, fmts=(0, 1, 2, 3), wants=None, **kw):
    """the device against the host statement (or `wants`)"""
    wants = wants if wants is not None else [jb.color_host(u, c) for u, c in zip(images, chains)]
    for fmt in fmts:
        check_color_device(jb, ctx, images, chains, fmt, wants=wants, **kw)
    return wants


# one pixel; no interior; Pillow's image; one past a 64 x 32 tile both ways; one past 256 columns; more than 256 rows of two pixels
SIZES = [(1, 1), (3, 2), (61, 47), (65, 33), (257, 5), (2, 300)]
SIZE_CHAINS = [[(SX, 0.27)], [(SY, -0.3)], [(TX, 1)], [(TY, -1)], [(ROT, 30)], [(ROT, -91)], [(TX, 1000)], [(ROT, 360)],
               [(B, 1.2), (SY, 0.99), (I, 0)],                                             # between pointwise operations
               [(SX, -0.27), (ROT, 44.999)], [(ROT, 135), (I, 0), (TX, -1)],               # two warps
               [(ROT, 30), (C, 1.3)], [(C, 1.3), (ROT, 30)], [(SX, 0.5), (A, 0)], [(E, 0), (TY, 1)],      # in front of / behind a statistic
               [(SY, 0.1), (E, 0), (TX, 1), (C, 0.7), (P, 5)],                             # between two statistics
               [(ROT, -30), (BLUR, 1.2), (Z, 128)], [(S, 1.1), (SX, 0.3), (BLUR, 4.0)],    # in front of a blur: both halos
               [(A, 0), (TX, 2), (SY, -0.27), (SH, 1.6), (I, 0)],                          # in front of a sharpness
               [(H, 30), (Z, 100)], [(C, 0.8), (BLUR, 0.9)], []]                           # views without a warp in a launch with one


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_sizes_strides_and_formats(jb, ctx, size):
    w, h = size
    images = [content(w, h, i) for i in range(len(SIZE_CHAINS))]
    wants = check(jb, ctx, images, SIZE_CHAINS, pads=(13, 7, 77), in_pads=(5, 11))
    if w * h >= 91:
        assert sum(not np.array_equal(a, b) for a, b in zip(wants, images)) >= len(SIZE_CHAINS) - 3
        assert all(np.array_equal(a, WR.apply_chain(u, c)) for a, u, c in zip(wants[:8], images, SIZE_CHAINS))   # (the host is the restatement's)
    check(jb, ctx, images[4:5], SIZE_CHAINS[4:5], fmts=(0,), wants=wants[4:5])          # one image, tight, its strides unused


def test_pillows_recorded_answers(jb, ctx):
    z = np.load(os.path.join(GOLD, "warp_kat.npz"))
    chains = [[(int(op), float(v)) for op, v in rows if int(op) != 0] for rows in z["chains"]]
    assert len(chains) >= 55
    check(jb, ctx, [z["image"]] * len(chains), chains, wants=list(z["out"]), pads=(3, 5, 7))


def _mixed_chains():
    shapes = [lambda i: [(B, 0.6 + 0.03 * i), (H, (7 * i) % 256)],                                         # the kernels of before
              lambda i: [(ROT, 3.0 * i - 40)],
              lambda i: [(SX, 0.02 * i - 0.3), (P, 1 + i % 7), (TY, i - 16)],
              lambda i: [(C, 0.7 + 0.02 * i), (G, 0), (BLUR, (0.3, 1.1, 4.2)[i % 3]), (Z, 128)],           # a blur, no warp
              lambda i: [(TX, 16 - i), (E, 0), (SY, 0.01 * i), (BLUR, (0.3, 1.1, 4.2)[i % 3])],            # two warps and a blur
              lambda i: [],
              lambda i: [(ROT, 7.5 * i + 1), (C, 1.2), (SH, 1.5)],
              lambda i: [(A, 0), (SH, 0.1 * i)],
              lambda i: [(I, 0), (SY, -0.03 * i), (A, 0), (ROT, -2.0 * i), (E, 0)]]
    chains = [shapes[i % len(shapes)](i) for i in range(33)]
    chains[32] = [(B, 0.9), (Z, 77)]               # the second launch: one view, no warp: the kernels without the warp text
    return chains


def test_33_views_in_one_call_of_mixed_kinds(jb, ctx):
    """two launches (32 + 1): the first mixes chains with no, one and two warps, with and without a blur or a sharpness -- its
    kernels are the WARP instantiations, for the views without a warp too --, the second has no warp: the kernels of before"""
    chains = _mixed_chains()
    jb.color_check(chains)
    assert {sum(op in WR.WARPS for op, _ in c) for c in chains[:32]} == {0, 1, 2} and not any(op in WR.WARPS for op, _ in chains[32])
    assert any(BLUR in [op for op, _ in c] and not any(op in WR.WARPS for op, _ in c) for c in chains)
    images = [content(67, 39, i) for i in range(33)]
    wants = check(jb, ctx, images, chains, fmts=(0, 3), pads=(1, 2, 3))
    assert all(np.array_equal(a, WR.apply_chain(u, c)) for a, u, c in zip(wants, images, chains))
    # the same views in the other order: the launch WITHOUT a warp comes first, then one with
    check(jb, ctx, images[::-1], chains[::-1], fmts=(3,), wants=wants[::-1])


def test_identical_from_run_to_run(jb, ctx):
    u = content(224, 224, 5)
    chains = [[(B, 1.1), (ROT, 17), (E, 0), (SX, -0.2), (C, 1.3), (SH, 1.5), (Z, 128)], [(TX, -45), (A, 0), (ROT, -30), (E, 0)]]
    a, idx, _ = color_device(jb, ctx, [u, u], chains, 3, fr.IMAGENET)
    b, _, _ = color_device(jb, ctx, [u, u], chains, 3, fr.IMAGENET)
    assert np.array_equal(a, b) and not (a[idx[0]] == SENT).all()


def test_refusals_launch_and_write_nothing(jb, ctx):
    u = np.zeros((5, 6, 3), np.uint8)
    nan = float("nan")
    for bad, status in (([(SX, nan)], -2), ([(ROT, float("inf"))], -2), ([(TX, 0.5)], -2), ([(TY, 65536)], -2),
                        ([(SX, 0.1), (SY, 0.1), (ROT, 1)], -9), ([(SH, 1.0), (TX, 1)], -9), ([(BLUR, 1.0), (ROT, 5)], -9),
                        ([(SH, 1.0), (ROT, 5), (H, 300)], -2),
                        ([(B, 1.1), (ROT, 180)], -9), ([(SY, 1e6)], -9)):                  # what depends on the size: the entry point's
        host, _, err = color_device(jb, ctx, [u, u], [[(E, 0), (ROT, 30), (SH, 1.0)], bad], 3, fr.IMAGENET, catch=True)
        assert err is not None and err.status == status and "colour chain 1" in str(err), (bad, err)
        assert (host == SENT).all()
    tall = np.zeros((40000, 2, 3), np.uint8)                                               # a corner beyond 16.16: Pillow's float path
    host, _, err = color_device(jb, ctx, [tall, tall], [[(ROT, 1)], [(TX, 1)]], 0, catch=True)
    assert err is not None and err.status == -9 and "colour chain 0" in str(err) and (host == SENT).all()


# ---- the seam ---------------------------------------------------------------------------------------------------------------
SEAM_CHAINS = [[[(B, 1.3), (ROT, 30), (E, 0), (SX, 0.2), (C, 0.7), (SH, 1.6)], [(TX, 5)], [(G, 0), (SY, -0.3), (BLUR, 1.1), (Z, 128)]],
               [[(H, 240), (A, 0), (ROT, -135), (I, 0)], [(SH, 1.9), (S, 1.8)], None]]
GROUP_CHAINS = [SEAM_CHAINS[0][:2] + SEAM_CHAINS[1], [[(C, 0.3), (TY, -3), (BLUR, 0.9)], [(Z, 10), (ROT, 90)]] + SEAM_CHAINS[0]]


def test_seam_views(jb, ctx):
    s, views = _seam(jb, (100, 37)), SEAM_VIEWS[(100, 37)]
    n_out = s.n * len(views[0])
    plain, pidx = s.run_outputs(ctx, 0, TARGET, n_out, _views_call(views, TARGET, BICUBIC, None))
    us = [plain[pidx[n]].reshape(TARGET[1], TARGET[0], 3) for n in range(n_out)]
    refs = [WR.apply_chain(u, chain) for u, chain in zip(us, [chain for row in SEAM_CHAINS for chain in row])]
    assert sum(not np.array_equal(r, u) for r, u in zip(refs, us)) >= 5
    for fmt in (0, 3):
        sb = _params(fmt)
        host, idx = s.run_outputs(ctx, fmt, TARGET, n_out, _views_call(views, TARGET, BICUBIC, SEAM_CHAINS), sb)
        want = np.full(host.size, SENT, np.uint8)
        for n, ref in enumerate(refs):
            want[idx[n]] = fr.bits(fr.to_format(ref, fmt, *sb)).view(np.uint8).reshape(idx[n].shape)
        bad = np.flatnonzero(host != want)
        assert bad.size == 0, (fmt, bad.size, int((~np.isin(bad, idx.ravel())).sum()), "bytes differ / of them outside the outputs")
    # a rotation by 180 degrees is refused for the view's size, behind the chains' own check, and nothing is written
    s.catch = True
    try:
        broken = [SEAM_CHAINS[0], [None, [(I, 0), (ROT, 180)], None]]
        host, _ = s.run_outputs(ctx, 3, TARGET, n_out, _views_call(views, TARGET, AREA, broken), fr.IMAGENET)
        assert s.error is not None and s.error.status == -9 and "chain 4" in str(s.error) and (host == SENT).all(), s.error
    finally:
        s.catch = False


def test_seam_view_groups(jb, ctx):
    s = _seam(jb, (679, 451))
    plain, play = run_groups(s, ctx, 0, GROUP_VIEWS, GROUPS)
    fmt = 3
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
                ref = fr.to_format(WR.apply_chain(u, GROUP_CHAINS[i][first + v]), fmt, *sb)      # (the warp's size is the group's)
                wants[lay.buf_of[g]][lay.idx[g][i, v]] = fr.bits(ref).view(np.uint8).reshape(lay.idx[g][i, v].shape)
        first += k
    for host, want in zip(hosts, wants):
        assert np.array_equal(host, want), int((host != want).sum())


# ---- the batch decoder ------------------------------------------------------------------------------------------------------
def test_batch_decoder_with_rand_augment(jb):
    import torch
    from jpeg_decoder_amd.color import rand_augment, trivial_augment_wide
    paths = [_gold(n)[0] for n in FILES]
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    rng = np.random.default_rng(9)
    chains = [[rand_augment(rng, BT[0], BT[1], 3, 9 + 2 * i), trivial_augment_wide(rng)] for i in range(len(FILES))]
    chains[0][0] = [(ROT, 27), (E, 0), (TX, -int(150 / 331 * BT[0] * 0.3)), (C, 1.27), (SH, 1.27)]     # (whatever the draws: every kernel runs)
    chains[3][1] = [(SX, 0.27), (A, 0)]
    assert sum(op in WR.WARPS for row in chains for c in row for op, _ in c) >= 6
    us = _u8_views(jb, paths, FILE_VIEWS, resize=BT)
    want = np.stack([np.stack([fr.to_format(WR.apply_chain(u, c), spec.format, list(spec.scale), list(spec.bias)) for u, c in zip(ku, kc)])
                     for ku, kc in zip(us, chains)])
    with jb.BatchDecoder(4, 0, resize=BT, fmt=spec) as dec:
        out = torch.full((len(paths), 2, 3, BT[1], BT[0]), 7.0, dtype=torch.float16, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(paths, out, views=FILE_VIEWS, colors=chains)
        assert ret is out and tm["rc"] == 0 and st == [0] * len(paths)
        assert fr.same_bits(out.cpu().numpy(), want)
        # a rotation by 180 degrees refuses the whole call for the target's size: the tensor keeps its bytes
        broken = [list(r) for r in chains]
        broken[6][1] = [(B, 1.1), (ROT, 180)]
        out.fill_(7.0)
        ret, st, tm = dec.run_to_tensor(paths, out, views=FILE_VIEWS, colors=broken)
        assert tm["rc"] == -9 and bool((out == 7.0).all())
