"""The one harness of the device seam's GPU tests (a plain module: no fixtures): n images of one geometry go through
Context.blocks_to_rgb_device into a sentinel-filled buffer with padded strides and an odd lead, and the WHOLE buffer is
compared against "sentinel everywhere, the expected bits where the output lies".  Add the next output option here: one
more keyword of Seam.run, passed on to blocks_to_rgb_device; the layout and the comparison do not change."""
import numpy as np

import format_ref as fr

LAYOUTS = [(1, 1), (2, 2), (2, 1), (1, 2)]
SEAM_SIZES = [(4096, 4096), (1920, 1080), (679, 451), (100, 37), (1, 1), (7, 13)] + \
             [(64 * 8 + a, 16 * 3 + b) for a, b in zip(range(1, 8), range(7, 0, -1))]
SENT = 0xA5
DT = {0: np.uint8, 1: np.uint8, 2: np.float32, 3: np.float16}
NO_PARAMS = ((1, 1, 1), (0, 0, 0))


def _oracle_full(oracle, w, h, hs, vs, coef, q, qtab_id=(0, 1, 1)):
    from oracle.pyoracle import make_desc as odesc
    return oracle.blocks_to_rgb(odesc(w, h, hs, vs, list(qtab_id)), coef, q, nthreads=16)


class Seam:
    """n images of one geometry on the device (uploaded once; per-image quantisation tables, stride 768).  Every launch
    gets a fresh sentinel-filled buffer.  The pads are in elements: pad_row after every row, pad_plane after every plane
    (planar formats), pad_img after every image."""

    def __init__(self, jb, w, h, hs, vs, coefs, qs, qtab_id=(0, 1, 1), pad_row=0, pad_plane=0, pad_img=0):
        import torch
        self.jb, self.n = jb, len(coefs)
        self.desc = jb.make_desc(w, h, hs, vs, qtab_id)
        self.pads = (pad_row, pad_plane, pad_img)
        self.coef_t = torch.from_numpy(np.stack(coefs)).to("cuda:0")
        self.q_t = torch.from_numpy(np.stack([jb.resolve_qtabs(self.desc, q) for q in qs])).to("cuda:0")

    def run(self, ctx, fmt, out_size, scale_bias=NO_PARAMS, *, scale=1, roi=None, resize=None):
        """One launch whose output is `out_size` = (w, h) in format `fmt` (0: interleaved, through the entry points
        without a spec; 1, 2, 3: planar, with OutputSpec.make(fmt, *scale_bias) -- its plane stride explicit when there
        is row or plane padding and 0, "derive it", when there is none) -> (the whole buffer as host bytes, the index
        array [n, ...] of the output's bytes in it)."""
        import torch
        jb = self.jb
        pad_row, pad_plane, pad_img = self.pads
        w, h = out_size
        es = np.dtype(DT[fmt]).itemsize
        lead = 256 + 5 if es == 1 else 256 + 3 * es   # uint8: the output starts at an odd address
        if fmt == 0:
            row = 3 * w + pad_row
            img = row * h + pad_img
            spec = None
            idx = lead + np.arange(self.n)[:, None, None] * img + np.arange(h)[None, :, None] * row + np.arange(3 * w)[None, None, :]
        else:
            row = (w + pad_row) * es
            plane = row * h + pad_plane * es
            img = 3 * plane + pad_img * es
            spec = jb.OutputSpec.make(fmt, *scale_bias, plane_stride=plane if (pad_plane or pad_row) else 0)
            idx = (lead + np.arange(self.n)[:, None, None, None] * img + np.arange(3)[None, :, None, None] * plane +
                   np.arange(h)[None, None, :, None] * row + np.arange(w * es)[None, None, None, :])
        buf = torch.full((lead + self.n * img + 256,), SENT, dtype=torch.uint8, device="cuda:0")
        assert buf.data_ptr() % 256 == 0
        b = jb.DeviceBatch()
        b.desc, b.n_images = self.desc, self.n
        b.d_coef, b.coef_image_stride = self.coef_t.data_ptr(), self.coef_t.stride(0) * 2
        b.d_qtabs, b.qtab_image_stride = self.q_t.data_ptr(), 768
        b.d_rgb, b.rgb_row_stride, b.rgb_image_stride = buf.data_ptr() + lead, row, img
        torch.cuda.synchronize()
        ctx.blocks_to_rgb_device(b, scale=scale, fmt=spec, roi=roi, resize=resize)
        ctx.synchronize()
        return buf.cpu().numpy(), idx

    def check(self, ctx, wants, fmt, scale_bias=NO_PARAMS, *, scale=1, roi=None, resize=None, tag=None):
        """The launch: image i's output has the bits of wants[i] (an array in `fmt`, which also gives the output's
        size), and every other byte of the buffer still holds the sentinel.  -> run()'s (host bytes, index array)."""
        h, w = wants[0].shape[:2] if fmt == 0 else wants[0].shape[1:]
        host, idx = self.run(ctx, fmt, (w, h), scale_bias, scale=scale, roi=roi, resize=resize)
        want = np.full(host.size, SENT, np.uint8)
        for i, ref in enumerate(wants):
            assert ref.dtype == DT[fmt] and ref.shape == ((h, w, 3) if fmt == 0 else (3, h, w)), (ref.dtype, ref.shape)
            want[idx[i]] = fr.bits(ref).view(np.uint8).reshape(idx[i].shape)
        if not np.array_equal(host, want):
            bad = np.flatnonzero(host != want)
            inside = np.isin(bad, idx.ravel())
            raise AssertionError(f"{tag} scale {scale} roi {roi} resize {resize} fmt {fmt}: {bad.size} bytes differ, "
                                 f"{int((~inside).sum())} of them outside the output; first at buffer byte {bad[0]}")
        return host, idx
