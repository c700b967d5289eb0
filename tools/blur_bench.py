#!/usr/bin/env python3
"""What JB_COLOR_BLUR ("colour chains", include/jpegblk.h) costs in time; bench.py is untouched.  Context.color_device alone
(HIP events around one call: 320 views, 10 launches of 32), uint8 views of 224 x 224 and of 96 x 96 into normalised f16 CHW,
in ONE process, the sides alternating in blocks (tools/color_bench.py's scheme):

  identity   the empty chain: the apply kernel's copy plus format -- the yardstick;
  jitter     a ColorJitter chain (brightness, contrast, saturation, hue): the apply kernel with the contrast's reduction pass;
  blur_r0    [(COLOR_BLUR, 1.0)]: box radius 0, the kernel with the small halo;
  blur_r1    [(COLOR_BLUR, 2.0)]: box radius 1, the same kernel -- the largest radius the published pipelines draw;
  dino       jitter + grayscale + blur(2.0) + solarize: DINO's longest chain through the blur kernel;
  blur_r7    [(COLOR_BLUR, 8.0)]: box radius 7, the kernel with the large halo.

The expectation on record is about memory alone: the blur kernel reads (tile + halo) / tile times the bytes the apply kernel
reads and writes the same bytes ((64 + 12) (32 + 12) / (64 x 32) = 1.63 at r = 1).  No ratio is a pass / fail criterion.  Every
side's first view is checked bit for bit against jb.color_host.

Usage: python tools/blur_bench.py [--out profiles/r21/blur_bench.json]
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


def kernels(w, h, reps, blocks):
    import torch
    rng = np.random.default_rng(5)
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    scale = torch.tensor(list(spec.scale), device="cuda:0").view(3, 1, 1)
    bias = torch.tensor(list(spec.bias), device="cuda:0").view(3, 1, 1)
    src = torch.randint(0, 256, (N, h, w, 3), dtype=torch.uint8, device="cuda:0")
    out = torch.zeros((N, 3, h, w), dtype=torch.float16, device="cuda:0")
    jitter = jc.color_jitter(rng, 0.4, 0.4, 0.2, 0.1)
    cases = {"identity": [], "jitter": jitter, "blur_r0": [(jc.COLOR_BLUR, 1.0)], "blur_r1": [(jc.COLOR_BLUR, 2.0)],
             "dino": jitter + [(jc.COLOR_GRAYSCALE, 0.0), (jc.COLOR_BLUR, 2.0), (jc.COLOR_SOLARIZE, 128.0)], "blur_r7": [(jc.COLOR_BLUR, 8.0)]}
    assert [jb.blur_params(x)[0] for x in (1.0, 2.0, 8.0)] == [0, 1, 7]
    with jb.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)

        def call(chain):
            ctx.color_device(src.data_ptr(), 3 * w, 3 * w * h, w, h, N, [chain] * N, out.data_ptr(), 2 * w, 6 * w * h, fmt=spec)

        def time_one(fn):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            e.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(e)    # ms

        for name, chain in cases.items():       # the check: views 0 and N - 1 of every side, bit for bit
            out.zero_()
            call(chain)
            torch.cuda.synchronize()
            for i in (0, N - 1):
                want = torch.from_numpy(jb.color_host(src[i].cpu().numpy(), chain)).to("cuda:0")
                want = (want.float().permute(2, 0, 1) * scale + bias).half()
                assert torch.equal(out[i].view(torch.int16), want.contiguous().view(torch.int16)), (name, i)
        res = _alternate({name: (lambda c=chain: call(c)) for name, chain in cases.items()}, time_one, reps, blocks)
    r = {"views": f"{N} x {w}x{h}", "format": "RGB_F16_CHW", "unit": "ms per call (10 launches of 32 views)", "runs_per_block": reps, "blocks": blocks,
         "chains": cases, "checked_bit_exact": "views 0 and 319 of every side", "sides": res}
    for k in res:
        r[f"{k}_us_per_view"] = round(res[k]["median"] * 1e3 / N, 3)
        r[f"{k}_over_identity"] = round(res[k]["median"] / res["identity"]["median"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"224x224": kernels(224, 224, a.reps, a.blocks), "96x96": kernels(96, 96, a.reps, a.blocks)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
