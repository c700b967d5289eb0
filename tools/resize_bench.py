#!/usr/bin/env python3
"""What decoding to a fixed output size costs and saves (jb_blocks_to_rgb_device_resized, BatchDecoder(resize=));
bench.py is untouched.  Every comparison runs in ONE process and alternates its sides.

  pair    N x 1080p 4:2:0 -> 224 x 224 f16 CHW (ImageNet) at the seam: the launch pairs of resize= (pixel kernel into
          the context's scratch, jb_resample_kernel from there) against the full-size f16 CHW launch followed by
          torch.nn.functional.adaptive_avg_pool2d on the same stream -- a timing baseline only, its values differ --
          and against the full-size uint8 launch alone (what the pair's first half costs: the difference estimates the
          resample kernel).  `--repeats` blocks of `--launches` calls each, HIP events around every call; the median of
          every block, and the medians of the block medians.
  e2e     N x 1080p files (8 distinct writer files, repeated) through a BatchDecoder, entropy stage on the device: to
          the pinned arena (format 0) and into one CUDA tensor (run_to_tensor, f16 CHW), at full size and with
          resize=(224, 224), passes alternating; best and median wall time of `--passes` passes after one warm pass;
          and the share of the resample kernel (the estimate of `pair`, per image) in the device-resident pass.

Usage: python tools/resize_bench.py [--only pair,e2e] [--n-1080p 1024] [--out profiles/r08/resize_bench.json]
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

W, H, TW, TH = 1920, 1080, 224, 224


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


def pair(ctx, n, launches, repeats):
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    stream = torch.cuda.ExternalStream(ctx.stream)
    desc = jb.make_desc(W, H, 2, 2)
    g = jb.geometry_of(desc)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(n + W)
    coef = torch.randint(-48, 49, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
    q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
    full = torch.empty((n, 3, H, W), dtype=torch.float16, device="cuda:0")
    pooled = torch.empty((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")
    small = torch.empty((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")
    u8 = torch.empty((n, H, 3 * W), dtype=torch.uint8, device="cuda:0")
    spec_f, spec_r = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW), jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    bf = torch_batch(desc, n, coef, q, full, fmt=spec_f)
    br = torch_batch(desc, n, coef, q, small, fmt=spec_r, resize=(TW, TH))
    bu = torch_batch(desc, n, coef, q, u8)

    def baseline():
        ctx.blocks_to_rgb_device(bf, fmt=spec_f)
        with torch.cuda.stream(stream):
            pooled.copy_(torch.nn.functional.adaptive_avg_pool2d(full, (TH, TW)))

    sides = {"full_f16_then_avg_pool": baseline,
             "resize_224": lambda: ctx.blocks_to_rgb_device(br, fmt=spec_r, resize=(TW, TH)),
             "full_u8_only": lambda: ctx.blocks_to_rgb_device(bu)}
    for fn in sides.values():
        _block(stream, fn, launches)   # pre-conditioning, untimed
    med = {k: [] for k in sides}
    for _ in range(repeats):           # interleaved blocks: drift hits every side alike
        for k, fn in sides.items():
            med[k].append(float(np.median(_block(stream, fn, launches))) * 1e3)
    r = {"batch": f"{n}x{W}x{H}-420", "target": [TW, TH], "format": "RGB_F16_CHW", "launches_per_block": launches}
    for k in sides:
        m = np.array(med[k])
        r[k + "_block_medians_us"] = [round(v, 1) for v in m]
        r[k + "_us"] = round(float(np.median(m)), 1)
        r[k + "_spread_pct"] = round(float((m.max() - m.min()) / np.median(m) * 100), 2)
    r["speedup_vs_avg_pool"] = round(r["full_f16_then_avg_pool_us"] / r["resize_224_us"], 2)
    r["resample_estimate_us_per_image"] = round((r["resize_224_us"] - r["full_u8_only_us"]) / n, 3)
    r["resize_us_per_image"] = round(r["resize_224_us"] / n, 3)
    # the intermediate: 3 B written and 3 B read per source pixel
    r["intermediate_bytes_per_image"] = 6 * W * H
    return r


def e2e(n, threads, passes, resample_us_per_image):
    import torch
    from jpeg_decoder_amd import synth
    rows = []
    with tempfile.TemporaryDirectory() as d:
        distinct = []
        for j in range(8):
            coef, q = synth.synth_blocks(W, H, 2, 2, image_index=j)
            p = os.path.join(d, f"f{j}.jpg")
            with open(p, "wb") as f:
                f.write(synth.encode_jpeg(coef, W, H, 2, 2, q, restart_interval=0))
            distinct.append(p)
        paths = [distinct[i % 8] for i in range(n)]

        def timed(fns):
            """fns: {name: pass}; one warm pass each, then `passes` timed passes, alternating"""
            for fn in fns.values():
                fn()
            ts = {k: [] for k in fns}
            for _ in range(passes):
                for k, fn in fns.items():
                    t0 = time.perf_counter()
                    fn()
                    ts[k].append(time.perf_counter() - t0)
            return {k: {"best_ms": round(min(v) * 1e3, 2), "median_ms": round(float(np.median(v)) * 1e3, 2),
                        "images_per_s_best": round(n / min(v))} for k, v in ts.items()}

        # pinned host, format 0
        decs = {"whole": jb.BatchDecoder(threads, 0, arena_bytes=n * (jb.output_bytes(W, H, 0) + 256) + (1 << 20)),
                "resize_224": jb.BatchDecoder(threads, 0, arena_bytes=n * (jb.output_bytes(TW, TH, 0) + 256) + (1 << 20), resize=(TW, TH))}

        def host_pass(dec):
            def run():
                _, st, tm = dec.run(paths, keep_pixels=False)
                assert tm["rc"] == 0 and all(s == 0 for s in st), tm
            return run
        res = timed({k: host_pass(v) for k, v in decs.items()})
        for k, v in decs.items():
            rows.append({"route": "pinned_arena_u8_hwc", "output": k, "files": n, "threads": threads, **res[k],
                         "device_entropy_images": v.device_entropy_images})
            v.close()
        # device-resident, f16 CHW
        spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
        decs = {"whole": jb.BatchDecoder(threads, 0, fmt=spec), "resize_224": jb.BatchDecoder(threads, 0, fmt=spec, resize=(TW, TH))}
        outs = {"whole": torch.empty((n, 3, H, W), dtype=torch.float16, device="cuda:0"),
                "resize_224": torch.empty((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")}

        def dev_pass(dec, out):
            def run():
                _, st, tm = dec.run_to_tensor(paths, out)
                assert all(s == 0 for s in st), tm
            return run
        res = timed({k: dev_pass(v, outs[k]) for k, v in decs.items()})
        for k, v in decs.items():
            rows.append({"route": "run_to_tensor_f16_chw", "output": k, "files": n, "threads": threads, **res[k],
                         "device_entropy_images": v.device_entropy_images})
            v.close()
    for route in ("pinned_arena_u8_hwc", "run_to_tensor_f16_chw"):
        a, b = [x for x in rows if x["route"] == route]
        b["speedup_vs_whole_best"] = round(a["best_ms"] / b["best_ms"], 2)
    if resample_us_per_image is not None:
        b = rows[-1]
        b["resample_share_of_pass_pct"] = round(resample_us_per_image * n / (b["best_ms"] * 1e3) * 100, 2)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="pair,e2e")
    ap.add_argument("--n-1080p", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    only = a.only.split(",")
    est = None
    if "pair" in only:
        with jb.Context(0) as ctx:
            res["pair"] = pair(ctx, a.n_1080p, a.launches, a.repeats)
        est = res["pair"]["resample_estimate_us_per_image"]
        import torch
        torch.cuda.empty_cache()
    if "e2e" in only:
        res["e2e"] = e2e(a.n_1080p, a.threads, a.passes, est)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
