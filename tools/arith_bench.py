#!/usr/bin/env python3
"""What JB_ARITH_LIBJPEG costs at the seam against the reference arithmetic of the same build; bench.py is untouched.
Every comparison runs in ONE process over the same device-resident coefficients, on one stream, the two arithmetics
alternating in blocks, HIP events around every call; reported are the block medians, their median, their spread and the
ratio libjpeg / reference.  The reference-arithmetic kernels are the ones every other tool and bench.py measure.

  full    8 x 4096 x 4096 and one 1920 x 1080 image, 4:4:4 and 4:2:0, interleaved uint8
  crops   N x 1080p 4:2:0 with crops= (seeded random_resized_crop) -> 224 x 224 f16 CHW (ImageNet), bicubic

Usage: python tools/arith_bench.py [--only full,crops] [--n-1080p 1024] [--out profiles/r11/arith_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpeg_decoder_amd as jb  # noqa: E402
from jpeg_decoder_amd.api import torch_batch  # noqa: E402

FULL = [(8, 4096, 4096, 1, 1), (8, 4096, 4096, 2, 2), (1, 1920, 1080, 1, 1), (1, 1920, 1080, 2, 2)]
TW, TH = 224, 224


def _block(stream, fn, launches):
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, e in evs:
        a.record(stream)
        fn()
        e.record(stream)
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(e) for a, e in evs])


def _alternate(stream, sides, launches, repeats):
    """-> {side: (block medians in us, their median, their spread in % of it)}"""
    for fn in sides.values():
        _block(stream, fn, max(1, launches // 2))   # pre-conditioning, untimed
    med = {k: [] for k in sides}
    for _ in range(repeats):                        # interleaved blocks: drift hits both sides alike
        for k, fn in sides.items():
            med[k].append(float(np.median(_block(stream, fn, launches))) * 1e3)
    out = {}
    for k, v in med.items():
        m = np.array(v)
        out[k] = ([round(x, 1) for x in m], round(float(np.median(m)), 1), round(float((m.max() - m.min()) / np.median(m) * 100), 2))
    return out


def _report(m):
    r = {}
    for k, (blocks, med, spread) in m.items():
        r[k + "_block_medians_us"], r[k + "_us"], r[k + "_spread_pct"] = blocks, med, spread
    r["libjpeg_over_reference"] = round(r["libjpeg_us"] / r["reference_us"], 3)
    return r


def _coefficients(n, desc, seed):
    """n images of small random coefficients (the kernels' time does not depend on the values) and quality-90 tables"""
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    g = jb.geometry_of(desc)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(seed)
    coef = torch.randint(-8, 9, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
    q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
    return coef, q


def run(ref, lj, n_1080p, launches, repeats, only):
    import torch
    stream = torch.cuda.ExternalStream(ref.stream)
    ctxs = {"reference": ref, "libjpeg": lj}
    res = {"launches_per_block": launches, "blocks": repeats}
    if "full" in only:
        for n, w, h, hs, vs in FULL:
            desc = jb.make_desc(w, h, hs, vs)
            coef, q = _coefficients(n, desc, n + w + hs)
            out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda:0")
            batch = torch_batch(desc, n, coef, q, out)
            sides = {k: (lambda c=c: c.blocks_to_rgb_device(batch, stream=ref.stream)) for k, c in ctxs.items()}
            r = _report(_alternate(stream, sides, launches, repeats))
            r["output_bytes_per_s_reference"] = round(out.numel() / (r["reference_us"] * 1e-6) / 1e9, 1)
            res[f"{n}x{w}x{h}-{'444' if hs == 1 else '420'}"] = r
            del coef, out, batch
            torch.cuda.empty_cache()
    if "crops" in only:
        n = n_1080p
        desc = jb.make_desc(1920, 1080, 2, 2)
        coef, q = _coefficients(n, desc, n)
        spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
        out = torch.zeros((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")
        batch = torch_batch(desc, n, coef, q, out, fmt=spec, resize=(TW, TH), filter=jb.FILTER_BICUBIC)
        rng = np.random.default_rng(n)
        crops = [jb.random_resized_crop(1920, 1080, rng) for _ in range(n)]
        sides = {k: (lambda c=c: c.blocks_to_rgb_device(batch, stream=ref.stream, fmt=spec, resize=(TW, TH), crops=crops, filter=jb.FILTER_BICUBIC))
                 for k, c in ctxs.items()}
        r = _report(_alternate(stream, sides, max(2, launches // 2), repeats))
        r["rectangles"] = "random_resized_crop, numpy default_rng(%d)" % n
        res[f"{n}x1920x1080-420 crops -> {TW}x{TH} f16 bicubic"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="full,crops")
    ap.add_argument("--n-1080p", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with jb.Context(0) as ref, jb.Context(0, arithmetic=jb.ARITH_LIBJPEG) as lj:
        res = run(ref, lj, a.n_1080p, a.launches, a.repeats, a.only.split(","))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
