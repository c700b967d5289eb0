#!/usr/bin/env python3
"""Kernel time of the seam at full size and at 1/2, 1/4, 1/8 (jb_blocks_to_rgb_device[_scaled]) on large batches.

For every batch and every K: `--precondition` untimed launches, then `--launches` launches with HIP events around
each one (torch.cuda.Event on the context's stream, as bench.py times the kernel); the median is reported, in us and
in TB/s of the launch's own traffic = coefficient bytes + output bytes (ceil(W/K) x ceil(H/K) x 3 per image).  The
coefficients are random int16 in [-48, 48] generated on the device: the kernel's time does not depend on their values.
Usage: python tools/seam_timer.py [--launches 200] [--precondition 50] [--scales 1,2,4,8] [--out file.json]

--formats: the output formats instead of the scales (jb_blocks_to_rgb_device_fmt: planar u8, f32, f16 with ImageNet's
scale / bias), each next to what it replaces: the format-0 launch followed by the plain torch conversion on the same
stream (TWO_STEP below), timed as ONE interval by the same events.  TBps_vs_fmt0: the fused launch's bytes/s on its own
traffic against the format-0 launch's in the same run; fused_vs_two_step: two-step median / fused median.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpeg_decoder_amd as jb  # noqa: E402
from jpeg_decoder_amd.api import torch_batch  # noqa: E402

# (images, width, height, hs, vs)
BATCHES = [(32, 4096, 4096, 1, 1), (8, 4096, 4096, 2, 2), (8, 4096, 4096, 2, 1), (8, 4096, 4096, 1, 2), (128, 1920, 1080, 1, 1)]
NAMES = {(1, 1): "444", (2, 2): "420", (2, 1): "422", (1, 2): "440"}


def time_batch(ctx, n, w, h, hs, vs, scales, launches, precondition):
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    desc = jb.make_desc(w, h, hs, vs)
    g = jb.geometry_of(desc)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(n * 7 + w + hs * 3 + vs)
    coef = torch.randint(-48, 49, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
    q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.stream)
    rows = []
    for k in scales:
        ow, oh = jb.scaled_size(w, h, k)
        out = torch.empty((n, oh, 3 * ow), dtype=torch.uint8, device="cuda:0")
        b = torch_batch(desc, n, coef, q, out, scale=k)
        torch.cuda.synchronize()
        for _ in range(precondition):
            ctx.blocks_to_rgb_device(b, scale=k)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, e in evs:
            a.record(stream)
            ctx.blocks_to_rgb_device(b, scale=k)
            e.record(stream)
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(e) for a, e in evs])
        med = float(np.median(ms))
        traffic = n * (g.coef_bytes + 3 * ow * oh)
        rows.append({"batch": f"{n}x{w}x{h}-{NAMES[(hs, vs)]}", "scale": k, "out": [ow, oh], "us_median": round(med * 1e3, 1),
                     "us_min": round(float(ms.min()) * 1e3, 1), "coef_GB": round(n * g.coef_bytes / 1e9, 3),
                     "out_GB": round(n * 3 * ow * oh / 1e9, 3), "TBps": round(traffic / (med * 1e-3) / 1e12, 3)})
        del out
    full = rows[0] if rows and rows[0]["scale"] == 1 else None
    for r in rows:
        if full is not None:
            r["speedup_vs_k1"] = round(full["us_median"] / r["us_median"], 3)
            # where the launch sits against the bytes/s the full-size launch reaches on its own traffic
            r["TBps_vs_k1"] = round(r["TBps"] / full["TBps"], 3)
    return rows


FMT_NAMES = {0: "RGB_U8_HWC", 1: "RGB_U8_CHW", 2: "RGB_F32_CHW", 3: "RGB_F16_CHW"}
TWO_STEP = {1: "x.view(N,H,W,3).permute(0,3,1,2).contiguous()",
            2: "y = x.view(N,H,W,3).permute(0,3,1,2).to(torch.float32, memory_format=torch.contiguous_format); y.mul_(scale.view(1,3,1,1)); y.add_(bias.view(1,3,1,1))",
            3: "y = x.view(N,H,W,3).permute(0,3,1,2).to(torch.float16, memory_format=torch.contiguous_format); y.mul_(scale.view(1,3,1,1)); y.add_(bias.view(1,3,1,1))"}


def _timed(stream, fn, launches, precondition):
    import torch
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(precondition):
            fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, e in evs:
            a.record(stream)
            fn()
            e.record(stream)
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(e) for a, e in evs])


def time_formats(ctx, n, w, h, hs, vs, launches, precondition):
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    desc = jb.make_desc(w, h, hs, vs)
    g = jb.geometry_of(desc)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(n * 7 + w + hs * 3 + vs)
    coef = torch.randint(-48, 49, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
    q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.stream)
    name = f"{n}x{w}x{h}-{NAMES[(hs, vs)]}"
    x = torch.empty((n, h, 3 * w), dtype=torch.uint8, device="cuda:0")
    b0 = torch_batch(desc, n, coef, q, x)
    ms = _timed(stream, lambda: ctx.blocks_to_rgb_device(b0), launches, precondition)
    med0 = float(np.median(ms))
    tb0 = n * (g.coef_bytes + 3 * w * h) / (med0 * 1e-3) / 1e12
    rows = [{"batch": name, "format": FMT_NAMES[0], "us_median": round(med0 * 1e3, 1), "us_min": round(float(ms.min()) * 1e3, 1),
             "coef_GB": round(n * g.coef_bytes / 1e9, 3), "out_GB": round(n * 3 * w * h / 1e9, 3), "TBps": round(tb0, 3)}]
    tdt = {1: torch.uint8, 2: torch.float32, 3: torch.float16}
    for fmt in (1, 2, 3):
        spec = jb.OutputSpec.imagenet(fmt)
        out = torch.empty((n, 3, h, w), dtype=tdt[fmt], device="cuda:0")
        bf = torch_batch(desc, n, coef, q, out, fmt=spec)
        ms = _timed(stream, lambda: ctx.blocks_to_rgb_device(bf, fmt=spec), launches, precondition)
        med = float(np.median(ms))
        out_bytes = n * jb.output_bytes(w, h, fmt)
        tb = (n * g.coef_bytes + out_bytes) / (med * 1e-3) / 1e12
        del out
        # what the fused launch replaces: the format-0 launch, then torch's permute / convert / normalise, same stream
        scale = torch.tensor(list(spec.scale), dtype=tdt[fmt] if fmt != 1 else torch.float32, device="cuda:0").view(1, 3, 1, 1)
        bias = torch.tensor(list(spec.bias), dtype=tdt[fmt] if fmt != 1 else torch.float32, device="cuda:0").view(1, 3, 1, 1)

        def two_step():
            ctx.blocks_to_rgb_device(b0)
            v = x.view(n, h, w, 3).permute(0, 3, 1, 2)
            if fmt == 1:
                return v.contiguous()
            y = v.to(tdt[fmt], memory_format=torch.contiguous_format)
            y.mul_(scale)
            y.add_(bias)
            return y

        ms2 = _timed(stream, two_step, launches, precondition)
        med2 = float(np.median(ms2))
        rows.append({"batch": name, "format": FMT_NAMES[fmt], "us_median": round(med * 1e3, 1), "us_min": round(float(ms.min()) * 1e3, 1),
                     "coef_GB": round(n * g.coef_bytes / 1e9, 3), "out_GB": round(out_bytes / 1e9, 3), "TBps": round(tb, 3),
                     "TBps_vs_fmt0": round(tb / tb0, 3), "two_step_us_median": round(med2 * 1e3, 1),
                     "two_step_us_min": round(float(ms2.min()) * 1e3, 1), "fused_vs_two_step": round(med2 / med, 3),
                     "fused_below_two_step": bool(med < med2), "two_step": TWO_STEP[fmt]})
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--precondition", type=int, default=50)
    ap.add_argument("--scales", default="1,2,4,8")
    ap.add_argument("--out", default="")
    ap.add_argument("--formats", action="store_true", help="time the output formats (and the two-step they replace) instead of the scales")
    args = ap.parse_args()
    scales = [int(x) for x in args.scales.split(",")]
    res = []
    with jb.Context(0) as ctx:
        for n, w, h, hs, vs in BATCHES:
            rows = (time_formats(ctx, n, w, h, hs, vs, args.launches, args.precondition) if args.formats
                    else time_batch(ctx, n, w, h, hs, vs, scales, args.launches, args.precondition))
            for r in rows:
                print(json.dumps(r), flush=True)
                res.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
