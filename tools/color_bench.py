#!/usr/bin/env python3
"""What "colour chains" (include/jpegblk.h) cost in time; bench.py is untouched.  N x 1920 x 1080 4:2:0 files, DINO's
multi-crop (crops.random_multicrop: 2 views at 224 x 224, 8 at 96 x 96, bicubic), normalised f16 CHW, through
BatchDecoder.run_to_tensor in ONE process, three sides alternating in blocks:

  plain   the call without colors=;
  colors  the call with a DINO chain (color.dino_color) on every view;
  torch   the call without colors= into uint8 HWC, then the same chains as per-view torch ops on the device (float
          arithmetic in torchvision's tensor formulas -- close to, not bit-equal to, the PIL bits) and the normalisation.

Every output is checked: `colors` bit for bit against jb.color_host of the plain uint8 views, `torch` within a few grey levels of
it on views without a hue shift or a solarize.  No ratio is a pass / fail criterion: plain and torch of THIS run are the yardsticks.
`kernels` times Context.color_device alone (HIP events, 320 views of 224 x 224 to normalised f16): an identity chain -- the
copy plus format -- a DINO chain without and with the contrast's reduction pass.

Usage: python tools/color_bench.py [--n 1024] [--only files,kernels] [--out profiles/r17/color_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpeg_decoder_amd as jb  # noqa: E402
from jpeg_decoder_amd import color as jc  # noqa: E402

W, H = 1920, 1080
GROUPS = [(2, (224, 224), jb.FILTER_BICUBIC), (8, (96, 96), jb.FILTER_BICUBIC)]
K = sum(g[0] for g in GROUPS)


def _alternate(sides, time_one, reps, blocks):
    for fn in sides.values():                       # untimed: the first runs size buffers and scratches
        for _ in range(2):
            time_one(fn)
    med = {k: [] for k in sides}
    for _ in range(blocks):                         # interleaved blocks: drift hits every side alike
        for k, fn in sides.items():
            med[k].append(float(np.median([time_one(fn) for _ in range(reps)])))
    out = {}
    for k, v in med.items():
        m = np.array(v)
        out[k] = {"block_medians": [round(x, 3) for x in m], "median": round(float(np.median(m)), 3),
                  "spread_pct": round(float((m.max() - m.min()) / np.median(m) * 100), 2)}
    return out


def _files(n, out_dir):
    from jpeg_decoder_amd import synth
    paths = []
    for i in range(8):   # eight distinct files, repeated: as the other benches do
        coef, q = synth.synth_blocks(W, H, 2, 2, i)
        p = os.path.join(out_dir, f"color_{W}x{H}_420_{i}.jpg")
        with open(p, "wb") as f:
            f.write(synth.encode_jpeg(coef, W, H, 2, 2, q, restart_interval=0))
        paths.append(p)
    return [paths[i % 8] for i in range(n)]


def _luma(x):
    return (0.299 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]).unsqueeze(-1)


def _torch_hue(x, d):
    """x [h, w, 3] float 0..255: RGB -> HSV, the hue moved by d / 255 of a turn, back"""
    import torch
    r, g, b = x.unbind(-1)
    mx, mn = x.max(-1).values, x.min(-1).values
    cr = (mx - mn).clamp_min(1e-6)
    rc, gc, bc = (mx - r) / cr, (mx - g) / cr, (mx - b) / cr
    h = torch.where(r == mx, bc - gc, torch.where(g == mx, 2.0 + rc - bc, 4.0 + gc - rc))
    h = ((h / 6.0 + 1.0) % 1.0 + d / 255.0) % 1.0
    s = torch.where(mx > 0, (mx - mn) / mx.clamp_min(1e-6), torch.zeros_like(mx))
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    p, q, t = mx * (1 - s), mx * (1 - s * f), mx * (1 - s * (1 - f))
    i = i.long() % 6
    sel = [(mx, t, p), (q, mx, p), (p, mx, t), (p, q, mx), (t, p, mx), (mx, p, q)]
    return torch.stack([sum((i == k) * sel[k][c] for k in range(6)) for c in range(3)], -1)


def _torch_chain(u8, chain, scale, bias):
    """one view [h, w, 3] uint8 on the device -> [3, h, w] f16: the chain in float, rounded to 0..255 after every op"""
    x = u8.float()
    for op, v in chain:
        if op == jc.COLOR_BRIGHTNESS:
            x = x * v
        elif op == jc.COLOR_CONTRAST:
            m = torch_round(_luma(x).mean())
            x = m + v * (x - m)
        elif op == jc.COLOR_SATURATION:
            lum = _luma(x)
            x = lum + v * (x - lum)
        elif op == jc.COLOR_GRAYSCALE:
            x = _luma(x).expand(-1, -1, 3)
        elif op == jc.COLOR_SOLARIZE:
            x = (x < v) * x + (x >= v) * (255.0 - x)
        else:
            x = _torch_hue(x, v)
        x = x.clamp(0, 255).floor()
    return (x.permute(2, 0, 1) * scale + bias).half()


def torch_round(x):
    import torch
    return torch.floor(x + 0.5)


def files(n, reps, blocks, threads):
    import torch
    from jpeg_decoder_amd.crops import random_multicrop
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    scale = torch.tensor(list(spec.scale), device="cuda:0").view(3, 1, 1)
    bias = torch.tensor(list(spec.bias), device="cuda:0").view(3, 1, 1)
    rng = np.random.default_rng(17)
    views = [random_multicrop(W, H, rng, [(g[0], s) for g, s in zip(GROUPS, ((0.4, 1.0), (0.05, 0.4)))]) for _ in range(n)]
    chains = [[jc.dino_color(rng, v if v < 2 else None) for v in range(K)] for _ in range(n)]

    def time_one(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3   # ms

    def f16_outs():
        return [torch.zeros((n, k, 3, h, w), dtype=torch.float16, device="cuda:0") for k, (w, h), _ in GROUPS]

    with tempfile.TemporaryDirectory() as tmp:
        paths = _files(n, tmp)
        outs = {"plain": f16_outs(), "colors": f16_outs(), "torch": f16_outs()}
        u8 = [torch.zeros((n, k, h, w, 3), dtype=torch.uint8, device="cuda:0") for k, (w, h), _ in GROUPS]
        dec = jb.BatchDecoder(threads, 0, fmt=spec)
        dec_u8 = jb.BatchDecoder(threads, 0)
        try:
            def run(d, out, colors=None):
                _, st, tm = d.run_to_tensor(paths, out, views=views, view_groups=GROUPS, colors=colors)
                assert tm["rc"] == 0 and not any(st), (tm, [s for s in st if s][:4])

            def torch_side():
                run(dec_u8, u8)
                first = 0
                for g, (k, _, _) in enumerate(GROUPS):
                    for i in range(n):
                        for v in range(k):
                            outs["torch"][g][i, v] = _torch_chain(u8[g][i, v], chains[i][first + v], scale, bias)
                    first += k

            sides = {"plain": lambda: run(dec, outs["plain"]), "colors": lambda: run(dec, outs["colors"], chains), "torch": torch_side}
            res = _alternate(sides, time_one, reps, blocks)
            # the checks: `colors` against the host statement on the plain uint8 views, `torch` close to it
            run(dec_u8, u8)
            checked = close = 0
            worst = 0.0
            for i in range(0, n, max(1, n // 16)):
                first = 0
                for g, (k, _, _) in enumerate(GROUPS):
                    for v in range(k):
                        chain = chains[i][first + v]
                        want = jb.color_host(u8[g][i, v].cpu().numpy(), chain)
                        want_t = (torch.from_numpy(want).to("cuda:0").float().permute(2, 0, 1) * scale + bias).half()
                        assert torch.equal(outs["colors"][g][i, v].contiguous().view(torch.int16), want_t.contiguous().view(torch.int16)), (i, g, v, chain)
                        checked += 1
                        if all(op not in (jc.COLOR_HUE, jc.COLOR_SOLARIZE) for op, _ in chain):   # (neither is continuous)
                            back = ((outs["torch"][g][i, v].float() - bias) / scale).permute(1, 2, 0).cpu().numpy()
                            worst = max(worst, float(np.abs(back - want).max()))
                            close += 1
                    first += k
            assert not torch.equal(outs["plain"][0], outs["colors"][0])
            assert worst <= 8.0, worst   # (float formulas against Pillow's integer ones: a few grey levels)
        finally:
            dec.close()
            dec_u8.close()
    r = {"batch": f"{n} files {W}x{H}-420", "views_per_file": K, "groups": [[k, list(t), f] for k, t, f in GROUPS], "format": "RGB_F16_CHW",
         "route": "run_to_tensor", "threads": threads, "unit": "ms per batch", "runs_per_block": reps, "blocks": blocks, "sides": res,
         "views_checked_bit_exact": checked, "torch_views_compared": close, "torch_worst_abs_diff": round(worst, 2),
         "colors_over_plain": round(res["colors"]["median"] / res["plain"]["median"], 3),
         "torch_over_plain": round(res["torch"]["median"] / res["plain"]["median"], 3)}
    for k in res:
        r[f"{k}_files_per_s"] = round(n / (res[k]["median"] * 1e-3))
    return r


def kernels(reps, blocks):
    import torch
    n, w, h = 320, 224, 224
    rng = np.random.default_rng(5)
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda:0")
    out = torch.zeros((n, 3, h, w), dtype=torch.float16, device="cuda:0")
    jitter = jc.color_jitter(rng, 0.4, 0.4, 0.2, 0.1)
    cases = {"identity": [], "jitter_without_contrast": [o for o in jitter if o[0] != jc.COLOR_CONTRAST], "jitter": jitter}
    with jb.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)

        def time_one(fn):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            e.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(e)    # ms

        sides = {name: (lambda c=chain: ctx.color_device(src.data_ptr(), 3 * w, 3 * w * h, w, h, n, [c] * n, out.data_ptr(), 2 * w, 6 * w * h, fmt=spec))
                 for name, chain in cases.items()}
        res = _alternate(sides, time_one, reps, blocks)
    r = {"views": f"{n} x {w}x{h}", "format": "RGB_F16_CHW", "unit": "ms per call (10 launches of 32 views)", "chains": {k: v for k, v in cases.items()},
         "sides": res}
    for k in res:
        r[f"{k}_us_per_view"] = round(res[k]["median"] * 1e3 / n, 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="files,kernels")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    only = a.only.split(",")
    res = {}
    if "kernels" in only:
        res["kernels"] = kernels(10, 5)
    if "files" in only:
        res["files"] = files(a.n, a.reps, a.blocks, a.threads)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
