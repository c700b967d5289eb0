#!/usr/bin/env python3
"""What a rectangle per image costs and saves at the seam (jb_blocks_to_rgb_device_crops); bench.py is untouched.
Both comparisons run in ONE process over the same N x 1080p 4:2:0 coefficients -> 224 x 224 f16 CHW (ImageNet), in
alternating blocks, HIP events around every call; reported are the block medians and the medians of the block medians.

  table   the cost of the table: every rectangle equal to the centre 224 x 224, through crops= (launch pairs of at most
          32 images, the rectangles in the kernel arguments) against the shipped roi= + resize= (one rectangle in
          JbLaunch, launch pairs as large as the scratch allows) -- the same bits.  Also the spread the shipped side
          shows against itself between its own blocks: the yardstick for "no slower".
  random  what the feature is for: seeded random_resized_crop rectangles, one batched crops= call against one roi= +
          resize= call per image (the same bits; the only way to get them without crops=); the ratio, and the share of
          the pixel kernel's launched workgroups that find nothing to do (every image of a launch gets as many
          workgroups as the launch's largest rectangle needs).

Usage: python tools/crops_bench.py [--only table,random] [--n-1080p 1024] [--out profiles/r09/crops_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpeg_decoder_amd as jb  # noqa: E402
from jpeg_decoder_amd.api import torch_batch  # noqa: E402

W, H, TW, TH = 1920, 1080, 224, 224
CROPS_PER_LAUNCH = 32            # kJbCropsPerLaunch (csrc/jb_knobs.h)
TMP_BYTES = 128 << 20            # kJbResizeTmpBytes, unless JPEGBLK_RESIZE_TMP_BYTES says otherwise
MCU, MCUS_PER_TILE = 16, 32      # 4:2:0: 16 x 16 pixels per MCU, 32 MCUs per row-bound tile


def _block(stream, fn, launches):
    """-> the times (ms) of `launches` calls, events around each"""
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
    for _ in range(repeats):                        # interleaved blocks: drift hits every side alike
        for k, fn in sides.items():
            med[k].append(float(np.median(_block(stream, fn, launches))) * 1e3)
    out = {}
    for k, v in med.items():
        m = np.array(v)
        out[k] = ([round(x, 1) for x in m], round(float(np.median(m)), 1), round(float((m.max() - m.min()) / np.median(m) * 100), 2))
    return out


def _tiles(r):
    x, y, w, h = r
    mx, my = x // MCU, y // MCU
    return ((y + h - 1) // MCU - my + 1) * -(-((x + w - 1) // MCU - mx + 1) // MCUS_PER_TILE)


def empty_share(crops):
    """the seam's packing (csrc/jb_seam.cpp seam_launch_crops), replayed: -> (launch pairs, workgroups launched by the
    pixel kernel, those of them with work)"""
    cap = int(os.environ.get("JPEGBLK_RESIZE_TMP_BYTES", TMP_BYTES))
    pairs = launched = useful = 0
    i = 0
    while i < len(crops):
        m, size = 1, 3 * crops[i][2] * crops[i][3]
        while i + m < len(crops) and m < CROPS_PER_LAUNCH and size + 3 * crops[i + m][2] * crops[i + m][3] <= cap:
            size += 3 * crops[i + m][2] * crops[i + m][3]
            m += 1
        t = [_tiles(r) for r in crops[i:i + m]]
        pairs, launched, useful = pairs + 1, launched + m * max(t), useful + sum(t)
        i += m
    return pairs, launched, useful


def run(ctx, n, launches, repeats, only):
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    stream = torch.cuda.ExternalStream(ctx.stream)
    desc = jb.make_desc(W, H, 2, 2)
    g = jb.geometry_of(desc)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(n + W)
    coef = torch.randint(-48, 49, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
    q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    out_a = torch.zeros((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")
    out_b = torch.zeros((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")
    ba = torch_batch(desc, n, coef, q, out_a, fmt=spec, resize=(TW, TH))
    bb = torch_batch(desc, n, coef, q, out_b, fmt=spec, resize=(TW, TH))
    res = {"batch": f"{n}x{W}x{H}-420", "target": [TW, TH], "format": "RGB_F16_CHW", "launches_per_block": launches, "blocks": repeats}

    if "table" in only:
        centre = ((W - TW) // 2, (H - TH) // 2, TW, TH)
        crops = [centre] * n
        sides = {"shipped_roi_resize": lambda: ctx.blocks_to_rgb_device(ba, fmt=spec, roi=centre, resize=(TW, TH)),
                 "crops_all_equal": lambda: ctx.blocks_to_rgb_device(bb, fmt=spec, crops=crops, resize=(TW, TH))}
        m = _alternate(stream, sides, launches, repeats)
        assert torch.equal(out_a, out_b), "crops= and roi= + resize= differ"
        r = {"rectangle": list(centre), "same_bits": True, "crops_launch_pairs": empty_share(crops)[0]}
        for k, (blocks, med, spread) in m.items():
            r[k + "_block_medians_us"], r[k + "_us"], r[k + "_spread_pct"] = blocks, med, spread
        r["crops_over_shipped"] = round(r["crops_all_equal_us"] / r["shipped_roi_resize_us"], 3)
        r["slower_by_pct"] = round((r["crops_over_shipped"] - 1) * 100, 2)
        r["within_shipped_spread"] = bool(r["slower_by_pct"] <= r["shipped_roi_resize_spread_pct"])
        res["table"] = r

    if "random" in only:
        rng = np.random.default_rng(n)
        crops = [jb.random_resized_crop(W, H, rng) for _ in range(n)]
        singles = [torch_batch(desc, 1, coef[i], q, out_a[i:i + 1], fmt=spec, resize=(TW, TH)) for i in range(n)]

        def per_image():
            for i in range(n):
                ctx.blocks_to_rgb_device(singles[i], fmt=spec, roi=crops[i], resize=(TW, TH))

        sides = {"one_call_per_image": per_image,
                 "one_batched_call": lambda: ctx.blocks_to_rgb_device(bb, fmt=spec, crops=crops, resize=(TW, TH))}
        m = _alternate(stream, sides, max(2, launches // 3), repeats)
        assert torch.equal(out_a, out_b), "crops= and one roi= + resize= call per image differ"
        pairs, launched, useful = empty_share(crops)
        r = {"rectangles": "random_resized_crop, numpy default_rng(%d)" % n, "same_bits": True, "crops_launch_pairs": pairs,
             "pixel_workgroups_launched": launched, "pixel_workgroups_with_work": useful,
             "empty_workgroup_share_pct": round((launched - useful) / launched * 100, 2),
             "mean_rectangle_pixels": round(float(np.mean([c[2] * c[3] for c in crops])))}
        for k, (blocks, med, spread) in m.items():
            r[k + "_block_medians_us"], r[k + "_us"], r[k + "_spread_pct"] = blocks, med, spread
        r["speedup_batched_over_per_image"] = round(r["one_call_per_image_us"] / r["one_batched_call_us"], 2)
        r["batched_us_per_image"] = round(r["one_batched_call_us"] / n, 3)
        res["random"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="table,random")
    ap.add_argument("--n-1080p", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with jb.Context(0) as ctx:
        res = run(ctx, a.n_1080p, a.launches, a.repeats, a.only.split(","))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
