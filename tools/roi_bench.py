#!/usr/bin/env python3
"""What a region of interest costs and saves (jb_blocks_to_rgb_device_roi, BatchDecoder(roi=)); bench.py is untouched.

  parity  N x 4096^2 4:4:4 and 4:2:0 at the seam, format 0: the rectangle = the whole image (the ROI instantiation of
          the kernel) against the launch without a rectangle, alternating in ONE process; `--repeats` blocks of
          `--launches` launches each, HIP events around every launch.  Reported: the median of every block, the spread
          of the block medians of each side, and the ratio of the medians of medians.
  crop    a 224 x 224 centre crop of N x 1080p 4:2:0 in f16 CHW (ImageNet) against the full-size launch of that
          format, next to the ratio of the two grids (workgroups launched), which is what the crop should save.
  e2e     N x 1080p files (8 distinct writer files, repeated) through a BatchDecoder, entropy stage on the device:
          to the pinned arena (format 0) and into one CUDA tensor (run_to_tensor, f16 CHW), each with and without the
          224 x 224 centre crop; best and median wall time of `--passes` passes after one warm pass.

Usage: python tools/roi_bench.py [--only parity,crop,e2e] [--n-big 32] [--n-1080p 1024] [--out file.json]
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
from jpeg_decoder_amd.api import torch_batch  # noqa: E402

NAMES = {(1, 1): "444", (2, 2): "420"}


def _inputs(n, w, h, hs, vs):
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    desc = jb.make_desc(w, h, hs, vs)
    g = jb.geometry_of(desc)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(n + w + 3 * hs + vs)
    coef = torch.randint(-48, 49, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
    q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
    return desc, g, coef, q


def _block(stream, fn, launches):
    """-> the times (ms) of `launches` launches, events around each"""
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, e in evs:
        a.record(stream)
        fn()
        e.record(stream)
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(e) for a, e in evs])


def parity(ctx, n, launches, repeats):
    import torch
    stream = torch.cuda.ExternalStream(ctx.stream)
    rows = []
    for hs, vs in ((1, 1), (2, 2)):
        w = h = 4096
        desc, g, coef, q = _inputs(n, w, h, hs, vs)
        out = torch.empty((n, h, 3 * w), dtype=torch.uint8, device="cuda:0")
        b = torch_batch(desc, n, coef, q, out)
        sides = {"no_roi": lambda: ctx.blocks_to_rgb_device(b), "roi_whole": lambda: ctx.blocks_to_rgb_device(b, roi=(0, 0, w, h))}
        for fn in sides.values():
            _block(stream, fn, launches)   # pre-conditioning, untimed
        med = {k: [] for k in sides}
        for _ in range(repeats):           # interleaved blocks: drift hits both sides alike
            for k, fn in sides.items():
                med[k].append(float(np.median(_block(stream, fn, launches))) * 1e3)
        r = {"batch": f"{n}x{w}x{h}-{NAMES[(hs, vs)]}", "launches_per_block": launches}
        for k in sides:
            m = np.array(med[k])
            r[k + "_block_medians_us"] = [round(v, 1) for v in m]
            r[k + "_us"] = round(float(np.median(m)), 1)
            r[k + "_spread_pct"] = round(float((m.max() - m.min()) / np.median(m) * 100), 2)
        r["roi_over_no_roi"] = round(r["roi_whole_us"] / r["no_roi_us"], 4)
        rows.append(r)
        del out, coef
        torch.cuda.empty_cache()
    return rows


def crop(ctx, n, launches, repeats):
    import torch
    stream = torch.cuda.ExternalStream(ctx.stream)
    w, h, hs, vs, cw, ch = 1920, 1080, 2, 2, 224, 224
    roi = ((w - cw) // 2, (h - ch) // 2, cw, ch)
    desc, g, coef, q = _inputs(n, w, h, hs, vs)
    full = torch.empty((n, 3, h, w), dtype=torch.float16, device="cuda:0")
    small = torch.empty((n, 3, ch, cw), dtype=torch.float16, device="cuda:0")
    spec_f, spec_c = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW), jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    bf = torch_batch(desc, n, coef, q, full, fmt=spec_f)
    bc = torch_batch(desc, n, coef, q, small, fmt=spec_c, roi=roi)
    sides = {"full_fmt": lambda: ctx.blocks_to_rgb_device(bf, fmt=spec_f), "roi_224": lambda: ctx.blocks_to_rgb_device(bc, fmt=spec_c, roi=roi)}
    for fn in sides.values():
        _block(stream, fn, launches)
    med = {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            med[k].append(float(np.median(_block(stream, fn, launches))) * 1e3)
    # the grids: row-bound tiles of 32 MCUs of 16 x 16 pixels (4:2:0)
    per_tile, mw, mh = 32, 8 * hs, 8 * vs
    tiles_full = -(-g.mcus_x // per_tile) * g.mcus_y
    mcx = (roi[0] + cw - 1) // mw - roi[0] // mw + 1
    mcy = (roi[1] + ch - 1) // mh - roi[1] // mh + 1
    tiles_roi = -(-mcx // per_tile) * mcy
    r = {"batch": f"{n}x{w}x{h}-420", "roi": list(roi), "format": "RGB_F16_CHW", "tiles_per_image_full": tiles_full, "tiles_per_image_roi": tiles_roi,
         "predicted_speedup_grid": round(tiles_full / tiles_roi, 2)}
    for k in sides:
        m = np.array(med[k])
        r[k + "_block_medians_us"] = [round(v, 1) for v in m]
        r[k + "_us"] = round(float(np.median(m)), 1)
    r["measured_speedup"] = round(r["full_fmt_us"] / r["roi_224_us"], 2)
    del full, small, coef
    torch.cuda.empty_cache()
    return [r]


def e2e(n, threads, passes):
    import torch
    from jpeg_decoder_amd import synth
    w, h, cw, ch = 1920, 1080, 224, 224
    roi = ((w - cw) // 2, (h - ch) // 2, cw, ch)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        distinct = []
        for j in range(8):
            coef, q = synth.synth_blocks(w, h, 2, 2, image_index=j)
            p = os.path.join(d, f"f{j}.jpg")
            with open(p, "wb") as f:
                f.write(synth.encode_jpeg(coef, w, h, 2, 2, q, restart_interval=0))
            distinct.append(p)
        paths = [distinct[i % 8] for i in range(n)]

        def timed(fn):
            fn()   # warm pass: buffers sized, pages pinned
            ts = []
            for _ in range(passes):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            return {"best_ms": round(min(ts) * 1e3, 2), "median_ms": round(float(np.median(ts)) * 1e3, 2),
                    "images_per_s_best": round(n / min(ts))}

        for name, r in (("whole", None), ("roi_224", roi)):
            per = jb.output_bytes(cw, ch, 0) if r else jb.output_bytes(w, h, 0)
            with jb.BatchDecoder(threads, 0, arena_bytes=n * (per + 256) + (1 << 20), roi=r) as dec:
                def run():
                    _, st, tm = dec.run(paths, keep_pixels=False)
                    assert tm["rc"] == 0 and all(s == 0 for s in st), tm
                row = {"route": "pinned_arena_u8_hwc", "output": name, "files": n, "threads": threads, **timed(run)}
                row["device_entropy_images"] = dec.device_entropy_images
            rows.append(row)
        spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
        for name, r in (("whole", None), ("roi_224", roi)):
            oh, ow = (ch, cw) if r else (h, w)
            with jb.BatchDecoder(threads, 0, fmt=spec, roi=r) as dec:
                out = torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda:0")

                def run():
                    _, st, tm = dec.run_to_tensor(paths, out)
                    assert all(s == 0 for s in st), tm
                row = {"route": "run_to_tensor_f16_chw", "output": name, "files": n, "threads": threads, **timed(run)}
                row["device_entropy_images"] = dec.device_entropy_images
                del out
                torch.cuda.empty_cache()
            rows.append(row)
    for route in ("pinned_arena_u8_hwc", "run_to_tensor_f16_chw"):
        a, b = [x for x in rows if x["route"] == route]
        b["speedup_vs_whole_best"] = round(a["best_ms"] / b["best_ms"], 2)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="parity,crop,e2e")
    ap.add_argument("--n-big", type=int, default=32)
    ap.add_argument("--n-1080p", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    only = a.only.split(",")
    if "parity" in only or "crop" in only:
        with jb.Context(0) as ctx:
            if "parity" in only:
                res["parity"] = parity(ctx, a.n_big, a.launches, a.repeats)
            if "crop" in only:
                res["crop"] = crop(ctx, a.n_1080p, a.launches, a.repeats)
    if "e2e" in only:
        res["e2e"] = e2e(a.n_1080p, a.threads, a.passes)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
