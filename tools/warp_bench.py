#!/usr/bin/env python3
"""What the geometric operations of the colour chains ("colour chains", include/jpegblk.h) cost in time; bench.py is untouched.
Context.color_device alone (HIP events around one call: 320 views, 10 launches of 32), uint8 views of 224 x 224 and of 96 x 96
into normalised f16 CHW, in ONE process, the sides alternating in blocks (tools/color_bench.py's scheme):

  identity      the empty chain: the apply kernel's copy plus format, 12-byte loads -- the yardstick;
  shear_x       [(COLOR_SHEAR_X, 0.27)]: the table kernel, then the apply kernel's WARP instantiation -- three byte loads a pixel at
  shear_y       [(COLOR_SHEAR_Y, 0.27)]  gathered positions (along a row for shear_x and the translations, across rows otherwise);
  translate_x   [(COLOR_TRANSLATE_X, 45)]: Pillow's shift path;
  translate_y   [(COLOR_TRANSLATE_Y, 45)]
  rotate        [(COLOR_ROTATE, 27)]
  rotate_color  rotate + brightness: RandAugment's typical pair of a geometric and a colour entry;
  shear_eq      shear_x + equalize: the pair with a statistic behind the warp (the histogram kernel gathers too);
  two_warps     rotate + shear_x: two positions mapped back, one gather;
  mixed_1_of_32 the empty chain on 31 views of every launch and rotate on one: what the views WITHOUT a geometric operation pay in a
                launch with one (the table kernel, and the WARP instantiation's byte loads in place of the 12-byte loads).

No ratio is a pass / fail criterion.  Views 0 and N - 1 of every side are checked bit for bit against jb.color_host.

Usage: python tools/warp_bench.py [--out profiles/r25/warp_bench.json]
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
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    scale = torch.tensor(list(spec.scale), device="cuda:0").view(3, 1, 1)
    bias = torch.tensor(list(spec.bias), device="cuda:0").view(3, 1, 1)
    src = torch.randint(0, 256, (N, h, w, 3), dtype=torch.uint8, device="cuda:0")
    out = torch.zeros((N, 3, h, w), dtype=torch.float16, device="cuda:0")
    move = int(150.0 / 331.0 * w * 0.3)                      # RandAugment's translation at magnitude 9
    cases = {"identity": [], "shear_x": jc.shear_x(0.27), "shear_y": jc.shear_y(0.27), "translate_x": jc.translate_x(move),
             "translate_y": jc.translate_y(move), "rotate": jc.rotate(27.0),
             "rotate_color": jc.rotate(27.0) + [(jc.COLOR_BRIGHTNESS, 1.27)], "shear_eq": jc.shear_x(0.27) + jc.equalize(),
             "two_warps": jc.rotate(27.0) + jc.shear_x(0.27)}
    per_view = {name: [chain] * N for name, chain in cases.items()}
    per_view["mixed_1_of_32"] = [jc.rotate(27.0) if i % 32 == 0 else [] for i in range(N)]
    jb.color_check(list(cases.values()))
    with jb.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)

        def call(chains):
            ctx.color_device(src.data_ptr(), 3 * w, 3 * w * h, w, h, N, chains, out.data_ptr(), 2 * w, 6 * w * h, fmt=spec)

        def time_one(fn):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            e.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(e)    # ms

        for name, chains in per_view.items():          # the check: views 0 and N - 1 of every side, bit for bit
            out.zero_()
            call(chains)
            torch.cuda.synchronize()
            for i in (0, N - 1):
                want = torch.from_numpy(jb.color_host(src[i].cpu().numpy(), chains[i])).to("cuda:0")
                want = (want.float().permute(2, 0, 1) * scale + bias).half()
                assert torch.equal(out[i].view(torch.int16), want.contiguous().view(torch.int16)), (name, i)
        res = _alternate({name: (lambda c=chains: call(c)) for name, chains in per_view.items()}, time_one, reps, blocks)
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
