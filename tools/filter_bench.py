#!/usr/bin/env python3
"""What the bilinear and bicubic filters cost at the seam against the area filter, and against the alternative a user
has without them; bench.py is untouched.  Every comparison runs in ONE process over the same N x 1080p 4:2:0
coefficients -> 224 x 224 f16 CHW (ImageNet), sides alternating in blocks, HIP events around every call; reported are
the block medians, their median and their spread.

  resize  (a) resize=(224, 224) with filter = area / bilinear / bicubic: the ratios to the area filter (unchanged code)
  crops   (b) the same three through crops= with seeded random_resized_crop rectangles
  torch   (c) a full-size f16 CHW launch followed by torch.nn.functional.interpolate(mode="bilinear" / "bicubic",
          antialias=True) on the same stream, in chunks of 64 images: timing only, its values differ

Also the loads per output pixel that the kernels' loop structure gives for (a)'s shapes (area: one per pixel of the
footprint; two-pass: taps_x per source row of a workgroup's span, shared by its 8 output rows), and with the split of the
area call's time into pixel kernel and resample kernel (2.44 + 5.0 ms) the ratio they predict.

Usage: python tools/filter_bench.py [--only resize,crops,torch] [--n-1080p 1024] [--out profiles/r10/filter_bench.json]
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
FILTERS = {"area": jb.FILTER_AREA, "bilinear": jb.FILTER_BILINEAR, "bicubic": jb.FILTER_BICUBIC}
ROWS_PER_WG = 8                      # kFilterRows (csrc/jb_resample.hip)
PIXEL_MS, RESAMPLE_MS = 2.44, 5.0    # the area call's two halves per 1,024 images


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
    for _ in range(repeats):                        # interleaved blocks: drift hits every side alike
        for k, fn in sides.items():
            med[k].append(float(np.median(_block(stream, fn, launches))) * 1e3)
    out = {}
    for k, v in med.items():
        m = np.array(v)
        out[k] = ([round(x, 1) for x in m], round(float(np.median(m)), 1), round(float((m.max() - m.min()) / np.median(m) * 100), 2))
    return out


def _report(m, base):
    r = {}
    for k, (blocks, med, spread) in m.items():
        r[k + "_block_medians_us"], r[k + "_us"], r[k + "_spread_pct"] = blocks, med, spread
    for k in m:
        if k != base:
            r[k + "_over_" + base] = round(r[k + "_us"] / r[base + "_us"], 3)
    return r


def load_counts():
    """loads per output pixel of the whole frame -> the target, from the kernels' loops"""
    def area_axis(n_in, n_out):
        return float(np.mean([((j + 1) * n_in - 1) // n_out - j * n_in // n_out + 1 for j in range(n_out)]))
    out = {"area": round(area_axis(W, TW) * area_axis(H, TH), 1)}
    for name, S in (("bilinear", 1.0), ("bicubic", 2.0)):
        sx, sy = W / TW, H / TH
        taps_x = int(2.0 * S * sx) + 2              # the tap loop's length (jb_filter_taps)
        spans = []
        for k0 in range(0, TH, ROWS_PER_WG):
            lo = max(int((k0 + 0.5) * sy - S * sy + 0.5), 0)
            hi = min(int((min(k0 + ROWS_PER_WG, TH) - 0.5) * sy + S * sy + 0.5), H)
            spans.append(hi - lo)
        out[name] = round(float(np.sum(spans)) * taps_x / TH, 1)
    pred = {k: round((PIXEL_MS + RESAMPLE_MS * out[k] / out["area"]) / (PIXEL_MS + RESAMPLE_MS), 2) for k in ("bilinear", "bicubic")}
    return out, pred


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
    outs = {k: torch.zeros((n, 3, TH, TW), dtype=torch.float16, device="cuda:0") for k in FILTERS}
    batches = {k: torch_batch(desc, n, coef, q, outs[k], fmt=spec, resize=(TW, TH), filter=f) for k, f in FILTERS.items()}
    loads, predicted = load_counts()
    res = {"batch": f"{n}x{W}x{H}-420", "target": [TW, TH], "format": "RGB_F16_CHW", "launches_per_block": launches, "blocks": repeats,
           "loads_per_output_pixel": loads, "predicted_call_ratio_to_area": predicted}

    def call(k, **kw):
        return lambda: ctx.blocks_to_rgb_device(batches[k], fmt=spec, resize=(TW, TH), filter=FILTERS[k], **kw)

    if "resize" in only:
        r = _report(_alternate(stream, {k: call(k) for k in FILTERS}, launches, repeats), "area")
        for k in ("bilinear", "bicubic"):
            r[k + "_measured_over_predicted"] = round(r[k + "_over_area"] / predicted[k], 3)
        res["resize"] = r

    if "crops" in only:
        rng = np.random.default_rng(n)
        crops = [jb.random_resized_crop(W, H, rng) for _ in range(n)]
        r = _report(_alternate(stream, {k: call(k, crops=crops) for k in FILTERS}, launches, repeats), "area")
        r["rectangles"] = "random_resized_crop, numpy default_rng(%d)" % n
        res["crops"] = r

    if "torch" in only:
        import torch.nn.functional as F
        full = torch.zeros((n, 3, H, W), dtype=torch.float16, device="cuda:0")
        small = torch.zeros((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")
        spec_full = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)      # (torch_batch writes the tensor's plane stride into the spec)
        bfull = torch_batch(desc, n, coef, q, full, fmt=spec_full)

        def two_step(mode):
            def fn():
                ctx.blocks_to_rgb_device(bfull, fmt=spec_full)
                with torch.cuda.stream(stream):
                    for i in range(0, n, 64):
                        small[i:i + 64] = F.interpolate(full[i:i + 64], size=(TH, TW), mode=mode, antialias=True, align_corners=False)
            return fn

        sides = {"bilinear": call("bilinear"), "torch_bilinear_two_step": two_step("bilinear"),
                 "bicubic": call("bicubic"), "torch_bicubic_two_step": two_step("bicubic")}
        m = _alternate(stream, sides, max(2, launches // 3), repeats)
        r = {}
        for k, (blocks, med, spread) in m.items():
            r[k + "_block_medians_us"], r[k + "_us"], r[k + "_spread_pct"] = blocks, med, spread
        for k in ("bilinear", "bicubic"):
            r[f"torch_{k}_two_step_over_{k}"] = round(r[f"torch_{k}_two_step_us"] / r[k + "_us"], 2)
        res["torch"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="resize,crops,torch")
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
