#!/usr/bin/env python3
"""Kernel time of the seam at full size and at 1/2, 1/4, 1/8 (jb_blocks_to_rgb_device[_scaled]) on large batches.

For every batch and every K: `--precondition` untimed launches, then `--launches` launches with HIP events around
each one (torch.cuda.Event on the context's stream, as bench.py times the kernel); the median is reported, in us and
in TB/s of the launch's own traffic = coefficient bytes + output bytes (ceil(W/K) x ceil(H/K) x 3 per image).  The
coefficients are random int16 in [-48, 48] generated on the device: the kernel's time does not depend on their values.
Usage: python tools/seam_timer.py [--launches 200] [--precondition 50] [--scales 1,2,4,8] [--out file.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--precondition", type=int, default=50)
    ap.add_argument("--scales", default="1,2,4,8")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    scales = [int(x) for x in args.scales.split(",")]
    res = []
    with jb.Context(0) as ctx:
        for n, w, h, hs, vs in BATCHES:
            for r in time_batch(ctx, n, w, h, hs, vs, scales, args.launches, args.precondition):
                print(json.dumps(r), flush=True)
                res.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
