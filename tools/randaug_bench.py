#!/usr/bin/env python3
"""What the RandAugment colour operations ("colour chains", include/jpegblk.h) cost in time; bench.py is untouched.
Context.color_device alone (HIP events around one call: 320 views, 10 launches of 32), uint8 views of 224 x 224 and of 96 x 96
into normalised f16 CHW, in ONE process, the sides alternating in blocks (tools/color_bench.py's scheme):

  identity      the empty chain: the apply kernel's copy plus format -- the yardstick;
  pointwise     hue + saturation + brightness: the apply kernel alone, through the switch over the operations;
  jitter        a ColorJitter chain (brightness, contrast, saturation, hue): the apply kernel behind the contrast's reduction pass;
  posterize     [(COLOR_POSTERIZE, 4)]: the apply kernel alone;
  autocontrast  [(COLOR_AUTOCONTRAST, 0)]: memset, histogram kernel, table kernel, apply kernel;
  equalize      [(COLOR_EQUALIZE, 0)]: the same four, the table from a prefix sum;
  equalize_2v   the same chain on views of two values: every lane's LDS atomic lands in one of two bins a channel;
  sharpness     [(COLOR_SHARPNESS, 1.27)]: the apply kernel (whose workgroups return at once), then the tile kernel with a halo of 1;
  eq_contrast   equalize + contrast: two rounds (histogram + table, then the mean kernel with the table applied in front);
  ra_longest    autocontrast + equalize: the rand_augment_color pair that costs most launches, two histogram rounds.

No ratio is a pass / fail criterion.  Views 0 and N - 1 of every side are checked bit for bit against jb.color_host.

--legacy-only times identity, pointwise and jitter alone: chains that a build from before these operations takes too, so the
same file can be run against such a build (copied into its tools/) in the same GPU session.

Usage: python tools/randaug_bench.py [--legacy-only] [--out profiles/r24/randaug_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decoder_amd as jb  # noqa: E402
from jpeg_decoder_amd import color as jc  # noqa: E402
from color_bench import _alternate  # noqa: E402

N = 320


def kernels(w, h, reps, blocks, legacy_only=False):
    import torch
    rng = np.random.default_rng(5)
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    scale = torch.tensor(list(spec.scale), device="cuda:0").view(3, 1, 1)
    bias = torch.tensor(list(spec.bias), device="cuda:0").view(3, 1, 1)
    random_src = torch.randint(0, 256, (N, h, w, 3), dtype=torch.uint8, device="cuda:0")
    two_src = torch.where(torch.rand((N, h, w, 3), device="cuda:0") < 0.3, 17, 230).to(torch.uint8)
    out = torch.zeros((N, 3, h, w), dtype=torch.float16, device="cuda:0")
    jitter = jc.color_jitter(rng, 0.4, 0.4, 0.2, 0.1)
    pointwise = [(jc.COLOR_HUE, 37.0), (jc.COLOR_SATURATION, 0.8), (jc.COLOR_BRIGHTNESS, 1.2)]
    cases = {"identity": ([], random_src), "pointwise": (pointwise, random_src), "jitter": (jitter, random_src)}
    if not legacy_only:
        cases.update({"posterize": (jc.posterize(4), random_src), "autocontrast": (jc.autocontrast(), random_src),
                      "equalize": (jc.equalize(), random_src), "equalize_2v": (jc.equalize(), two_src),
                      "sharpness": (jc.sharpness(1.27), random_src), "eq_contrast": (jc.equalize() + [(jc.COLOR_CONTRAST, 1.27)], random_src),
                      "ra_longest": (jc.autocontrast() + jc.equalize(), random_src)})
    jb.color_check([c for c, _ in cases.values()])
    with jb.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)

        def call(chain, src):
            ctx.color_device(src.data_ptr(), 3 * w, 3 * w * h, w, h, N, [chain] * N, out.data_ptr(), 2 * w, 6 * w * h, fmt=spec)

        def time_one(fn):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            e.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(e)    # ms

        for name, (chain, src) in cases.items():       # the check: views 0 and N - 1 of every side, bit for bit
            out.zero_()
            call(chain, src)
            torch.cuda.synchronize()
            for i in (0, N - 1):
                want = torch.from_numpy(jb.color_host(src[i].cpu().numpy(), chain)).to("cuda:0")
                want = (want.float().permute(2, 0, 1) * scale + bias).half()
                assert torch.equal(out[i].view(torch.int16), want.contiguous().view(torch.int16)), (name, i)
        res = _alternate({name: (lambda c=chain, s=src: call(c, s)) for name, (chain, src) in cases.items()}, time_one, reps, blocks)
    r = {"views": f"{N} x {w}x{h}", "format": "RGB_F16_CHW", "unit": "ms per call (10 launches of 32 views)", "runs_per_block": reps, "blocks": blocks,
         "chains": {k: c for k, (c, _) in cases.items()}, "checked_bit_exact": "views 0 and 319 of every side", "sides": res}
    for k in res:
        r[f"{k}_us_per_view"] = round(res[k]["median"] * 1e3 / N, 3)
        r[f"{k}_over_identity"] = round(res[k]["median"] / res["identity"]["median"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legacy-only", action="store_true")
    a = ap.parse_args()
    res = {"224x224": kernels(224, 224, a.reps, a.blocks, a.legacy_only), "96x96": kernels(96, 96, a.reps, a.blocks, a.legacy_only)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
