#!/usr/bin/env python3
"""What "draft decode" (include/jpegblk.h) changes in time under JB_ARITH_LIBJPEG; bench.py is untouched.  The draft image
is another image than the full-size decode, so there is no pass / fail ratio here: draft 1 -- the parent's behaviour -- is
the one yardstick, and draft 2 and 4 are reported next to it.

  seam    N x 1920 x 1080 4:2:0 -> 224 x 224 f16 CHW (ImageNet), bicubic, through blocks_to_rgb_device: draft 1, 2, 4 in ONE
          process over the same device-resident coefficients, on one stream, alternating in blocks, HIP events around every
          call; the block medians, their median, their spread and the ratio to draft 1.
  files   the same files through BatchDecoder.run_to_tensor (entropy stage, upload, pixel and filter launches, device
          output), one decoder per draft, alternating; wall time per batch.

Usage: python tools/draft_bench.py [--only seam,files] [--n 1024] [--out profiles/r15/draft_bench.json]
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
DRAFTS = (1, 2, 4)


def _alternate(sides, time_one, reps, blocks):
    """-> {side: {block medians, their median, their spread in % of it}}; two untimed blocks per side first (the first
    runs of a decoder size its buffers and its contexts' scratches)"""
    for _ in range(2):
        for fn in sides.values():
            for _ in range(reps):
                time_one(fn)
    med = {k: [] for k in sides}
    for _ in range(blocks):                         # interleaved blocks: drift hits every side alike
        for k, fn in sides.items():
            med[k].append(float(np.median([time_one(fn) for _ in range(reps)])))
    out = {}
    for k, v in med.items():
        m = np.array(v)
        out[k] = {"block_medians": [round(x, 3) for x in m], "median": round(float(np.median(m)), 3),
                  "spread_pct": round(float((m.max() - m.min()) / np.median(m) * 100), 2)}
    return out


def _ratios(res):
    base = res["draft1"]["median"]
    return {k + "_over_draft1": round(v["median"] / base, 3) for k, v in res.items() if k != "draft1"}


def seam(n, reps, blocks):
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    desc = jb.make_desc(W, H, 2, 2)
    g = jb.geometry_of(desc)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(n)
    # small random coefficients (the kernels' time does not depend on the values) and quality-90 tables
    coef = torch.randint(-8, 9, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
    q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    out = torch.zeros((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")
    batch = torch_batch(desc, n, coef, q, out, fmt=spec, resize=(TW, TH), filter=jb.FILTER_BICUBIC)
    ctxs = {K: jb.Context(0, arithmetic=jb.ARITH_LIBJPEG, draft=K) for K in DRAFTS}
    try:
        stream = torch.cuda.ExternalStream(ctxs[1].stream)

        def time_one(fn):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            e.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(e)    # ms

        sides = {f"draft{K}": (lambda c=c: c.blocks_to_rgb_device(batch, stream=ctxs[1].stream, fmt=spec, resize=(TW, TH), filter=jb.FILTER_BICUBIC))
                 for K, c in ctxs.items()}
        res = _alternate(sides, time_one, reps, blocks)
    finally:
        for c in ctxs.values():
            c.close()
    r = {"batch": f"{n} x {W}x{H}-420", "target": [TW, TH], "filter": "bicubic", "format": "RGB_F16_CHW", "unit": "ms per launch sequence",
         "launches_per_block": reps, "blocks": blocks, "sides": res, **_ratios(res)}
    for K in DRAFTS:
        r[f"draft{K}_frame"] = list(jb.scaled_size(W, H, K))
        r[f"draft{K}_us_per_image"] = round(res[f"draft{K}"]["median"] * 1e3 / n, 3)
    return r


def _files(n, out_dir):
    from jpeg_decoder_amd import synth
    paths = []
    for i in range(8):   # eight distinct files, repeated: as the other benches do
        coef, q = synth.synth_blocks(W, H, 2, 2, i)
        p = os.path.join(out_dir, f"draft_{W}x{H}_420_{i}.jpg")
        with open(p, "wb") as f:
            f.write(synth.encode_jpeg(coef, W, H, 2, 2, q, restart_interval=0))
        paths.append(p)
    return [paths[i % 8] for i in range(n)]


def files(n, reps, blocks, threads):
    import torch
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)

    def time_one(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3   # ms

    with tempfile.TemporaryDirectory() as tmp:
        paths = _files(n, tmp)
        out = torch.zeros((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")
        decs = {K: jb.BatchDecoder(threads, 0, fmt=spec, resize=(TW, TH), filter=jb.FILTER_BICUBIC, arithmetic=jb.ARITH_LIBJPEG, draft=K) for K in DRAFTS}
        try:
            def run(dec):
                _, st, tm = dec.run_to_tensor(paths, out)
                assert tm["rc"] == 0 and not any(st), (tm, [s for s in st if s][:4])

            res = _alternate({f"draft{K}": (lambda d=d: run(d)) for K, d in decs.items()}, time_one, reps, blocks)
        finally:
            for d in decs.values():
                d.close()
    r = {"batch": f"{n} files {W}x{H}-420", "target": [TW, TH], "filter": "bicubic", "format": "RGB_F16_CHW", "route": "run_to_tensor",
         "threads": threads, "unit": "ms per batch", "runs_per_block": reps, "blocks": blocks, "sides": res, **_ratios(res)}
    for K in DRAFTS:
        r[f"draft{K}_images_per_s"] = round(n / (res[f"draft{K}"]["median"] * 1e-3))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="seam,files")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    only = a.only.split(",")
    res = {}
    if "seam" in only:
        res["seam"] = seam(a.n, a.reps, a.blocks)
    if "files" in only:
        res["files"] = files(a.n, max(3, a.reps // 2), a.blocks, a.threads)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
