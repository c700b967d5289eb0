"""Colour chains on the GPU (-m gpu).  Context.color_device feeds the two colour kernels any uint8 image: the colour cube,
odd sizes with padded strides, Pillow's recorded answers (tests/golden/color_kat.npz); the reference is tests/color_ref.py
(the numpy restatement of Pillow) and format_ref.to_format.  At the seam and in the batch decoder the definition is checked:

    out(i, v) = to_format(color_ref.apply_chain(u, chain[i][v]), fmt, scale, bias)

with u what THE SAME CALL WITHOUT colors= writes in format 0, mirror included.  Every comparison is bit-exact, and at the seam
and for color_device the whole sentinel-filled buffer is compared, pads included."""
import os

import numpy as np
import pytest

import color_ref as R
import format_ref as fr
from conftest import GOLD
from seam_harness import DT, NO_PARAMS, SENT
from test_gpu_view_groups import run_groups
from test_gpu_views import BT, NAMES, OTHER, VIEWS, ViewSeam, _gold

pytestmark = pytest.mark.gpu

B, C, S, H, G, Z = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAYSCALE, R.SOLARIZE
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


def _params(fmt):
    return fr.IMAGENET if fmt >= 2 else NO_PARAMS


# ---- color_device --------------------------------------------------------------------------------------------------------
def color_device(jb, ctx, images, chains, fmt, scale_bias=NO_PARAMS, pads=(0, 0, 0), in_pads=(0, 0), catch=False):
    """n images of one size through Context.color_device: the input rows and images padded by in_pads (bytes) behind an odd
    lead, the output in a sentinel-filled buffer laid out as seam_harness lays a batch's out (pads in elements, an odd lead)
    -> (the whole output buffer as host bytes, the index array [n, ...] of the outputs' bytes, the JbError or None)."""
    import torch
    n = len(images)
    h, w = images[0].shape[:2]
    in_row = 3 * w + in_pads[0]
    in_img = in_row * h + in_pads[1]
    in_lead = 256 + 3
    src = np.full(in_lead + n * in_img + 64, 0x3C, np.uint8)
    in_idx = in_lead + np.arange(n)[:, None, None] * in_img + np.arange(h)[None, :, None] * in_row + np.arange(3 * w)[None, None, :]
    src[in_idx] = np.stack(images).reshape(n, h, 3 * w)
    src_t = torch.from_numpy(src).to("cuda:0")
    pad_row, pad_plane, pad_img = pads
    es = np.dtype(DT[fmt]).itemsize
    lead = 256 + 5 if es == 1 else 256 + 3 * es
    if fmt == 0:
        row = 3 * w + pad_row
        img = row * h + pad_img
        spec = None
        idx = lead + np.arange(n)[:, None, None] * img + np.arange(h)[None, :, None] * row + np.arange(3 * w)[None, None, :]
    else:
        row = (w + pad_row) * es
        plane = row * h + pad_plane * es
        img = 3 * plane + pad_img * es
        spec = jb.OutputSpec.make(fmt, *scale_bias, plane_stride=plane if (pad_plane or pad_row) else 0)
        idx = (lead + np.arange(n)[:, None, None, None] * img + np.arange(3)[None, :, None, None] * plane +
               np.arange(h)[None, None, :, None] * row + np.arange(w * es)[None, None, None, :])
    buf = torch.full((lead + n * img + 256,), SENT, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    error = None
    try:
        ctx.color_device(src_t.data_ptr() + in_lead, in_row, in_img, w, h, n, chains, buf.data_ptr() + lead, row, img, fmt=spec)
    except jb.JbError as e:
        if not catch:
            raise
        error = e
    ctx.synchronize()
    return buf.cpu().numpy(), idx, error


def check_color_device(jb, ctx, images, chains, fmt, wants=None, **kw):
    """every output has the bits of to_format(apply_chain(image, chain)) (or of wants[i]), every other byte the sentinel"""
    sb = _params(fmt)
    host, idx, _ = color_device(jb, ctx, images, chains, fmt, sb, **kw)
    want = np.full(host.size, SENT, np.uint8)
    for i, (u, chain) in enumerate(zip(images, chains)):
        ref = fr.to_format(wants[i] if wants is not None else R.apply_chain(u, chain), fmt, *sb)
        want[idx[i]] = fr.bits(ref).view(np.uint8).reshape(idx[i].shape)
    if not np.array_equal(host, want):
        bad = np.flatnonzero(host != want)
        inside = np.isin(bad, idx.ravel())
        first = int(np.argmax((idx.reshape(idx.shape[0], -1) == bad[0]).any(axis=1))) if inside[0] else -1
        raise AssertionError(f"fmt {fmt}: {bad.size} bytes differ, {int((~inside).sum())} of them outside the outputs; first at buffer byte "
                             f"{bad[0]} (image {first}, chain {chains[first] if first >= 0 else None})")


CUBE_CHAINS = [[(H, 37)], [(S, 0.3), (H, 200), (B, 1.4)], [(G, 0)], [(Z, 128)]]
_cube = {}


def _cube_refs():
    """the cube slices (B in {0, 1, 17, 127, 128, 254, 255} x all R, G) and their references, computed once"""
    if not _cube:
        _cube["u"] = R.cube_slices()
        _cube["refs"] = [R.apply_chain(_cube["u"], chain) for chain in CUBE_CHAINS]
    return _cube["u"], _cube["refs"]


@pytest.mark.parametrize("fmt", [0, 3])
def test_color_device_over_the_cube_slices(jb, ctx, fmt):
    u, refs = _cube_refs()
    check_color_device(jb, ctx, [u] * len(CUBE_CHAINS), CUBE_CHAINS, fmt, wants=refs)


SMALL_CHAINS = [[(S, 1.6), (C, 0.7), (H, 100)], [], [(C, 1.5), (Z, 99), (B, 0.6), (G, 0)]]


@pytest.mark.parametrize("size", [(1, 1), (3, 1), (7, 13), (97, 3), (224, 224)], ids=lambda s: "%dx%d" % s)
def test_color_device_sizes_strides_and_formats(jb, ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in SMALL_CHAINS]
    wants = [R.apply_chain(u, chain) for u, chain in zip(images, SMALL_CHAINS)]
    for fmt in (0, 1, 2, 3):
        check_color_device(jb, ctx, images, SMALL_CHAINS, fmt, wants=wants, pads=(13, 7, 77), in_pads=(5, 11))
    check_color_device(jb, ctx, images[:1], SMALL_CHAINS[:1], 0, wants=wants[:1])      # one image, tight, its strides unused


def test_color_device_gives_pillows_recorded_answers(jb, ctx):
    z = np.load(os.path.join(GOLD, "color_kat.npz"))
    chains = [[(int(op), float(v)) for op, v in rows if int(op) != 0] for rows in z["chains"]]
    images = [z["image"]] * len(chains)
    for fmt in (0, 1, 2, 3):
        check_color_device(jb, ctx, images, chains, fmt, wants=list(z["out"]), pads=(3, 5, 7))


def test_contrast_sum_beyond_32_bits(jb, ctx):
    """4200 x 4100 pixels of luma 255: the sum is 4.39e9 > 2^32; the mean must still be 255 and the image stay white"""
    import torch
    w, h = 4200, 4100
    assert 255 * w * h > 1 << 32
    src = torch.full((h, w, 3), 255, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.color_device(src.data_ptr(), 3 * w, 3 * w * h, w, h, 1, [[(C, 0.5)]], out.data_ptr(), 3 * w, 3 * w * h)
    ctx.synchronize()
    assert bool((out == 255).all())


def test_contrast_is_identical_from_run_to_run(jb, ctx):
    rng = np.random.default_rng(224)
    u = rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    chain = [(B, 1.1), (C, 1.3), (S, 0.8)]
    a, idx, _ = color_device(jb, ctx, [u], [chain], 0)
    b, _, _ = color_device(jb, ctx, [u], [chain], 0)
    assert np.array_equal(a, b)
    assert np.array_equal(a[idx[0]].reshape(u.shape), R.apply_chain(u, chain))


def test_33_views_in_one_call_each_with_its_own_chain(jb, ctx):
    """two launches (32 + 1); every other chain has a contrast, at the front, in the middle or at the end"""
    rng = np.random.default_rng(33)
    images, chains = [], []
    for i in range(33):
        images.append(rng.integers(0, 256, (29, 37, 3), dtype=np.uint8))
        chain = [(B, 0.6 + 0.03 * i), (H, (7 * i) % 256), (S, 0.5 + 0.04 * i)]
        if i % 2 == 0:
            chain.insert((i // 2) % 4, (C, 0.5 + 0.05 * i))
        chains.append(chain)
    assert {[op for op, _ in c].index(C) for c in chains if C in [op for op, _ in c]} == {0, 1, 2, 3}
    for fmt in (0, 3):
        check_color_device(jb, ctx, images, chains, fmt, pads=(1, 2, 3))


def test_color_device_refusals_write_nothing(jb, ctx):
    u = np.zeros((5, 6, 3), np.uint8)
    for chains, status in (([[], [(H, 1.5)]], -2), ([[(C, 1.0), (C, 1.0)], []], -9), ([[(9, 0)], []], -2)):
        host, _, err = color_device(jb, ctx, [u, u], chains, 3, fr.IMAGENET, catch=True)
        assert err is not None and err.status == status and "colour chain" in str(err), (chains, err)
        assert (host == SENT).all()
    assert "chain 1" in str(color_device(jb, ctx, [u, u], [[], [(H, 1.5)]], 0, catch=True)[2])


# ---- the seam ---------------------------------------------------------------------------------------------------------------
SEAM_VIEWS = {(100, 37): [[(0, 0, 100, 37), (10, 5, 64, 30, True), (50, 7, 40, 24)], [(3, 2, 90, 33, True), (0, 0, 100, 37), (60, 1, 33, 35)]],
              (679, 451): [[(0, 0, 679, 451), (100, 50, 300, 200, True), (400, 200, 279, 251)],
                           [(17, 3, 600, 400), (0, 0, 679, 451, True), (300, 100, 128, 96)]]}
SEAM_CHAINS = [[[(B, 1.3), (C, 0.7), (S, 1.2), (H, 20)], [], [(G, 0), (Z, 128)]],
               [[(H, 240), (S, 0.4), (C, 1.4), (B, 0.8)], [(S, 1.8)], None]]
TARGET = (32, 24)
_seams = {}


def _seam(jb, size):
    from jpeg_decoder_amd import synth
    if size not in _seams:
        w, h = size
        q = synth.annex_k_qtabs(60)
        coefs = [synth.synth_blocks(w, h, 2, 2, image_index=40 + i, qtabs=q)[0] for i in range(2)]
        _seams[size] = ViewSeam(jb, w, h, 2, 2, coefs, [q, q], pad_row=13, pad_plane=7, pad_img=77)
    return _seams[size]


def _views_call(views, target, filt, colors):
    return lambda c, b, spec: c.blocks_to_rgb_device(b, fmt=spec, resize=target, filter=filt, views=views, colors=colors)


def _check_views_color(s, c, views, target, filt, chains):
    """formats 0..3: the call with colors= against the definition, u from the same call without colors in format 0"""
    n_out = s.n * len(views[0])
    plain, pidx = s.run_outputs(c, 0, target, n_out, _views_call(views, target, filt, None))
    us = [plain[pidx[n]].reshape(target[1], target[0], 3) for n in range(n_out)]
    assert not any((u == SENT).all() for u in us)
    flat = [chain for row in chains for chain in row]
    refs = [R.apply_chain(u, chain) for u, chain in zip(us, flat)]
    assert any(not np.array_equal(r, u) for r, u in zip(refs, us))
    for fmt in (0, 1, 2, 3):
        sb = _params(fmt)
        host, idx = s.run_outputs(c, fmt, target, n_out, _views_call(views, target, filt, chains), sb)
        want = np.full(host.size, SENT, np.uint8)
        for n, ref in enumerate(refs):
            want[idx[n]] = fr.bits(fr.to_format(ref, fmt, *sb)).view(np.uint8).reshape(idx[n].shape)
        bad = np.flatnonzero(host != want)
        assert bad.size == 0, (fmt, filt, bad.size, int((~np.isin(bad, idx.ravel())).sum()), "bytes differ / of them outside the outputs")
        # all-empty colors: byte for byte the call without them
        empty, _ = s.run_outputs(c, fmt, target, n_out, _views_call(views, target, filt, [[None] * len(views[0])] * s.n), sb)
        without, _ = s.run_outputs(c, fmt, target, n_out, _views_call(views, target, filt, None), sb)
        assert np.array_equal(empty, without), (fmt, filt)


@pytest.mark.parametrize("filt", [AREA, BICUBIC], ids=["area", "bicubic"])
@pytest.mark.parametrize("size", list(SEAM_VIEWS), ids=lambda s: "%dx%d" % s)
def test_seam_views_with_colors(jb, ctx, size, filt):
    _check_views_color(_seam(jb, size), ctx, SEAM_VIEWS[size], TARGET, filt, SEAM_CHAINS)


@pytest.mark.parametrize("size", list(SEAM_VIEWS), ids=lambda s: "%dx%d" % s)
def test_seam_views_with_colors_under_libjpeg_arithmetic(jb, size):
    with jb.Context(0, arithmetic=jb.ARITH_LIBJPEG) as c:
        for filt in (AREA, BICUBIC):
            _check_views_color(_seam(jb, size), c, SEAM_VIEWS[size], TARGET, filt, SEAM_CHAINS)


def test_seam_views_with_colors_in_small_sub_batches(jb, monkeypatch):
    """a scratch cap that ends every sub-batch after one image (the stage counts towards it): the same bytes"""
    s = _seam(jb, (100, 37))
    views, n_out = SEAM_VIEWS[(100, 37)], 6
    with jb.Context(0) as c:
        whole, _ = s.run_outputs(c, 3, TARGET, n_out, _views_call(views, TARGET, AREA, SEAM_CHAINS), fr.IMAGENET)
    monkeypatch.setenv("JPEGBLK_RESIZE_TMP_BYTES", str(3 * 100 * 37 + 3 * 3 * 32 * 24 + 100))
    with jb.Context(0) as c:
        split, _ = s.run_outputs(c, 3, TARGET, n_out, _views_call(views, TARGET, AREA, SEAM_CHAINS), fr.IMAGENET)
    assert np.array_equal(whole, split) and not (whole == SENT).all()


GROUPS = [(2, (32, 24)), (3, (24, 16), BICUBIC)]
GROUP_VIEWS = [SEAM_VIEWS[(679, 451)][0][:2] + SEAM_VIEWS[(679, 451)][1], SEAM_VIEWS[(679, 451)][1][:2] + SEAM_VIEWS[(679, 451)][0]]
GROUP_CHAINS = [SEAM_CHAINS[0][:2] + SEAM_CHAINS[1], [[(C, 0.3)], [(Z, 10), (H, 128)]] + SEAM_CHAINS[0]]


@pytest.mark.parametrize("interleaved", [False, True], ids=["own_buffers", "one_block"])
def test_seam_view_groups_with_colors(jb, ctx, interleaved):
    s = _seam(jb, (679, 451))
    plain, play = run_groups(s, ctx, 0, GROUP_VIEWS, GROUPS, interleaved=interleaved)
    for fmt in (0, 3):
        sb = _params(fmt)
        hosts, lay = run_groups(s, ctx, fmt, GROUP_VIEWS, GROUPS, sb, interleaved,
                                call=lambda c, b, spec, outs: c.blocks_to_rgb_device(b, fmt=spec, views=GROUP_VIEWS, view_groups=GROUPS,
                                                                                     view_outputs=outs, colors=GROUP_CHAINS))
        wants = [np.full(h.size, SENT, np.uint8) for h in hosts]
        first = 0
        for g, grp in enumerate(GROUPS):
            k, (w, h) = grp[0], grp[1]
            for i in range(s.n):
                for v in range(k):
                    u = plain[play.buf_of[g]][play.idx[g][i, v]].reshape(h, w, 3)
                    ref = fr.to_format(R.apply_chain(u, GROUP_CHAINS[i][first + v]), fmt, *sb)
                    wants[lay.buf_of[g]][lay.idx[g][i, v]] = fr.bits(ref).view(np.uint8).reshape(lay.idx[g][i, v].shape)
            first += k
        for host, want in zip(hosts, wants):
            assert np.array_equal(host, want), (fmt, interleaved, int((host != want).sum()))
        empty, _ = run_groups(s, ctx, fmt, GROUP_VIEWS, GROUPS, sb, interleaved,
                              call=lambda c, b, spec, outs: c.blocks_to_rgb_device(b, fmt=spec, views=GROUP_VIEWS, view_groups=GROUPS,
                                                                                   view_outputs=outs, colors=[[None] * 5] * 2))
        without, _ = run_groups(s, ctx, fmt, GROUP_VIEWS, GROUPS, sb, interleaved)
        assert all(np.array_equal(a, b) for a, b in zip(empty, without))


def test_seam_refusals_write_nothing(jb, ctx):
    s = _seam(jb, (100, 37))
    views = SEAM_VIEWS[(100, 37)]
    s.catch = True
    try:
        for chains, status in (([[None, None, [(B, -1.0)]], [None] * 3], -2), ([[None] * 3, [[(C, 1), (H, 2), (C, 1)], None, None]], -9)):
            host, _ = s.run_outputs(ctx, 3, TARGET, 6, _views_call(views, TARGET, AREA, chains), fr.IMAGENET)
            assert s.error is not None and s.error.status == status and (host == SENT).all(), s.error
        assert "chain 3" in str(s.error)
        # the sibling's refusals come first: a view outside the frame next to a bad chain is the view's error
        outside = [views[0], [(90, 30, 20, 20), views[1][1], views[1][2]]]
        host, _ = s.run_outputs(ctx, 0, TARGET, 6, _views_call(outside, TARGET, AREA, [[[(9, 9)]] * 3] * 2))
        assert s.error.status == -2 and "colour chain" not in str(s.error) and (host == SENT).all()
        hosts, _ = run_groups(s, ctx, 0, [r + r[:2] for r in views], GROUPS,
                              call=lambda c, b, spec, outs: c.blocks_to_rgb_device(b, fmt=spec, views=[r + r[:2] for r in views], view_groups=GROUPS,
                                                                                   view_outputs=outs, colors=[[None] * 5, [None] * 4 + [[(G, 1)]]]))
        assert s.error.status == -2 and "chain 9" in str(s.error) and all((h == SENT).all() for h in hosts)
    finally:
        s.catch = False


# ---- the batch decoder ------------------------------------------------------------------------------------------------------
FILES = NAMES + ["img4", "img2"]                         # eight files, of four sizes
FILE_VIEWS = VIEWS + [VIEWS[3], VIEWS[0]]
FILE_OTHER = OTHER + [OTHER[3], OTHER[0]]


def _file_chains(seed):
    from jpeg_decoder_amd.color import dino_color
    rng = np.random.default_rng(seed)
    chains = [[dino_color(rng, v) for v in range(2)] for _ in FILES]
    chains[0][0] = [(C, 1.3), (H, 77), (S, 0.5), (Z, 128)]                 # (whatever the draws: some chains are never empty)
    chains[7][1] = [(G, 0), (B, 1.2)]
    return chains


def _u8_views(jb, paths, views, **kw):
    """what the decoder gives without colors in format 0: the definition's u, [K, h, w, 3] per file"""
    with jb.BatchDecoder(4, 0, **kw) as dec:
        imgs, st, tm = dec.run(paths, views=views)[:3]
    assert tm["rc"] == 0 and st == [0] * len(paths)
    return [np.ascontiguousarray(x) for x in imgs]


def test_batch_decoder_views_with_colors(jb):
    import torch
    paths = [_gold(n)[0] for n in FILES]
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    chains_a, chains_b = _file_chains(1), _file_chains(2)
    assert chains_a != chains_b
    us_a, us_b = _u8_views(jb, paths, FILE_VIEWS, resize=BT), _u8_views(jb, paths, FILE_OTHER, resize=BT)

    def want(us, chains):
        return np.stack([np.stack([fr.to_format(R.apply_chain(u, c), spec.format, list(spec.scale), list(spec.bias)) for u, c in zip(ku, kc)])
                         for ku, kc in zip(us, chains)])
    want_a, want_b = want(us_a, chains_a), want(us_b, chains_b)
    with jb.BatchDecoder(4, 0, resize=BT, fmt=spec) as dec:
        out = torch.full((len(paths), 2, 3, BT[1], BT[0]), 7.0, dtype=torch.float16, device="cuda:0")
        ret, st, tm = dec.run_to_tensor(paths, out, views=FILE_VIEWS, colors=chains_a)
        assert ret is out and tm["rc"] == 0 and st == [0] * len(paths)
        assert fr.same_bits(out.cpu().numpy(), want_a)
        # two batches in flight, each with its own views and chains
        t0 = dec.submit(paths, views=FILE_VIEWS, colors=chains_a)
        t1 = dec.submit(paths, views=FILE_OTHER, colors=chains_b)
        for t, w in ((t0, want_a), (t1, want_b)):
            imgs, st, tm = dec.collect(t)[:3]
            assert tm["rc"] == 0 and st == [0] * len(paths)
            assert fr.same_bits(np.stack([np.ascontiguousarray(x) for x in imgs]), w)
        # a file that fails for its own reasons gets its status, the others their colours
        bad_views = [list(r) for r in FILE_VIEWS]
        bad_views[1] = [(0, 0, 5000, 5), bad_views[1][1]]
        imgs, st, tm = dec.run(paths, views=bad_views, colors=chains_a)[:3]
        assert st[1] == -2 and imgs[1] is None and [x for i, x in enumerate(st) if i != 1] == [0] * 7
        assert fr.same_bits(np.ascontiguousarray(imgs[5]), want_a[5])
        # a bad chain refuses the whole call: nothing is decoded, the tensor keeps its bytes
        broken = [list(r) for r in chains_a]
        broken[6][1] = [(H, 0.5)]
        out.fill_(7.0)
        ret, st, tm = dec.run_to_tensor(paths, out, views=FILE_VIEWS, colors=broken)
        assert tm["rc"] == -2 and bool((out == 7.0).all())
        with pytest.raises(jb.JbError) as e:
            dec.submit(paths, views=FILE_VIEWS, colors=broken)
        assert e.value.status == -2 and "chain 13" in str(e.value)
        imgs, st, tm = dec.run(paths, views=FILE_VIEWS, colors=chains_a)[:3]       # and the decoder is as good as before
        assert tm["rc"] == 0 and fr.same_bits(np.stack([np.ascontiguousarray(x) for x in imgs]), want_a)


def test_batch_decoder_view_groups_with_colors(jb):
    import torch
    paths = [_gold(n)[0] for n in FILES]
    spec = jb.OutputSpec.imagenet(fr.FMT_RGB_F16_CHW)
    groups = [(1, (32, 32)), (1, (16, 12), BILINEAR)]
    chains = _file_chains(3)
    with jb.BatchDecoder(4, 0) as dec:
        us, st, tm = dec.run(paths, views=FILE_VIEWS, view_groups=groups)[:3]
    assert tm["rc"] == 0 and st == [0] * len(paths)
    wants = [np.stack([fr.to_format(R.apply_chain(np.ascontiguousarray(us[i][g][0]), chains[i][g]), spec.format, list(spec.scale), list(spec.bias))[None]
                       for i in range(len(paths))]) for g in range(2)]
    with jb.BatchDecoder(4, 0, fmt=spec) as dec:
        outs = [torch.full((len(paths), 1, 3, h, w), 7.0, dtype=torch.float16, device="cuda:0") for _, (w, h), *_ in groups]
        ret, st, tm = dec.run_to_tensor(paths, outs, views=FILE_VIEWS, view_groups=groups, colors=chains)
        assert tm["rc"] == 0 and st == [0] * len(paths)
        for out, w in zip(outs, wants):
            assert fr.same_bits(out.cpu().numpy(), w)
        imgs, st, tm = dec.collect(dec.submit(paths, views=FILE_VIEWS, view_groups=groups, colors=chains))[:3]
        assert tm["rc"] == 0 and st == [0] * len(paths)
        for g in range(2):
            assert fr.same_bits(np.stack([np.ascontiguousarray(imgs[i][g]) for i in range(len(paths))]), wants[g])
