#!/usr/bin/env python3
"""What view_groups= saves: the multi-crop of DINO / DINOv2 / iBOT / SwAV -- 2 "global" crops at 224 x 224 and 8 "local" crops
at 96 x 96 of every file (jb.random_multicrop) -- from ONE decode, against what a user does without it: one views= call per
group, each with its own target size (two entropy decodes, two pixel launches and two unions per file).  bench.py is
untouched.  All runs in ONE process on one device, in alternating blocks of at least five repetitions after two untimed
calls of every side; reported are the block medians, their median and the block-to-block spread of every side.  A
difference is real only where it exceeds the larger spread of the two sides ("beyond_spread").

  files  BatchDecoder with device output over N 1080p 4:2:0 files, normalised f16 CHW left in device memory:
         run_to_device(paths, views=, view_groups=) against two run_to_device(paths, views=) calls (K = 2 at 224, K = 8 at
         96) over the same paths.  Wall clock around the call(s) and a device synchronize; device_entropy_images per batch
         for both sides.
  seam   the same over N device-resident images: one view_groups= call against two views= calls; HIP events around
         every side; the outputs are compared bit for bit.

Usage: python tools/view_groups_bench.py [--only files,seam] [--n 1024] [--reps 5] [--blocks 3] [--threads 16] [--out profiles/r16/view_groups_bench.json]
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
from views_bench import _alternate, _files  # noqa: E402

W, H = 1920, 1080
GROUPS = [(2, (224, 224)), (8, (96, 96))]
K = sum(g[0] for g in GROUPS)


def _verdict(res, a, b):
    """the ratio b / a of the medians, and whether the difference exceeds the larger spread of the two sides"""
    ratio = res[b]["median"] / res[a]["median"]
    spread = max(res[a]["spread_pct"], res[b]["spread_pct"])
    return {"speedup": round(ratio, 3), "larger_spread_pct": spread, "beyond_spread": bool(abs(ratio - 1) * 100 > spread)}


def files(n, reps, blocks, threads):
    import torch
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    offsets, block = jb.view_groups_bytes(GROUPS, spec)
    out = {"batch": f"{n} files {W}x{H}-420", "groups": GROUPS, "format": "RGB_F16_CHW", "threads": threads, "unit": "ms per batch"}
    with tempfile.TemporaryDirectory() as tmp:
        paths = _files(n, tmp)
        rng = np.random.default_rng(n)
        views = [jb.random_multicrop(W, H, rng) for _ in range(n)]
        split = [[row[:2] for row in views], [row[2:] for row in views]]
        region = torch.zeros((n * block + 256 * (n + 2),), dtype=torch.uint8, device="cuda:0")
        n_dev = {}
        with jb.BatchDecoder(threads, 0, fmt=spec) as dec, jb.BatchDecoder(threads, 0, fmt=spec) as old:
            dec.set_device_output(region.data_ptr(), region.numel())
            old.set_device_output(region.data_ptr(), region.numel())

            def grouped():
                n0 = dec.device_entropy_images
                _, _, st, tm = dec.run_to_device(paths, views=views, view_groups=GROUPS)
                n_dev["view_groups"] = dec.device_entropy_images - n0
                assert tm["rc"] == 0 and not any(st), (tm, [s for s in st if s][:4])

            def two_calls():
                n0 = old.device_entropy_images
                for (k, target), mine in zip(GROUPS, split):
                    old.set_resize(target)
                    _, _, st, tm = old.run_to_device(paths, views=mine)
                    assert tm["rc"] == 0 and not any(st), (tm, [s for s in st if s][:4])
                n_dev["two_views_calls"] = old.device_entropy_images - n0

            def time_one(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3   # ms

            res = _alternate({"view_groups": grouped, "two_views_calls": two_calls}, time_one, reps, blocks)
    out["sides"] = res
    out["device_entropy_images_per_batch"] = dict(n_dev)
    for side, s in res.items():
        out[side + "_views_per_s"] = round(n * K / (s["median"] * 1e-3))
    out["view_groups_over_two_views_calls"] = _verdict(res, "view_groups", "two_views_calls")
    return out


def seam(n, reps, blocks):
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    with jb.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        desc = jb.make_desc(W, H, 2, 2)
        g = jb.geometry_of(desc)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(n + W)
        coef = torch.randint(-48, 49, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
        q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
        spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
        rng = np.random.default_rng(n)
        views = [jb.random_multicrop(W, H, rng) for _ in range(n)]
        new = [torch.zeros((n, k, 3, h, w), dtype=torch.float16, device="cuda:0") for k, (w, h) in GROUPS]
        old = [torch.zeros((n, k, 3, h, w), dtype=torch.float16, device="cuda:0") for k, (w, h) in GROUPS]
        # (torch_batch writes the planes' stride into the spec it is given; the grouped call wants 0 there: a spec of its own)
        batch = torch_batch(desc, n, coef, q, old[0].view(n * 2, 3, 224, 224), fmt=jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW), resize=(224, 224))   # (its d_rgb is not read)
        outs = [(t.data_ptr(), t.stride(0) * 2, t.stride(1) * 2, t.shape[4] * 2) for t in new]
        calls, first = [], 0
        for (k, (w, h)), t in zip(GROUPS, old):
            mine = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)   # (its plane stride is this group's)
            calls.append((torch_batch(desc, n, coef, q, t.view(n * k, 3, h, w), fmt=mine, resize=(w, h)), mine, (w, h), [row[first:first + k] for row in views]))
            first += k

        def grouped():
            ctx.blocks_to_rgb_device(batch, fmt=spec, views=views, view_groups=GROUPS, view_outputs=outs)

        def two_calls():
            for b, its_spec, target, mine in calls:
                ctx.blocks_to_rgb_device(b, fmt=its_spec, resize=target, views=mine)

        def time_one(fn):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            e.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(e) * 1e3   # us

        res = _alternate({"view_groups": grouped, "two_views_calls": two_calls}, time_one, reps, blocks)
        grouped(), two_calls()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(new, old)), "view_groups= and two views= calls differ"
        return {"batch": f"{n}x{W}x{H}-420", "groups": GROUPS, "format": "RGB_F16_CHW", "unit": "us per batch", "same_bits": True, "sides": res,
                "view_groups_over_two_views_calls": _verdict(res, "view_groups", "two_views_calls"),
                "us_per_view": round(res["view_groups"]["median"] / (n * K), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="files,seam")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5, "blocks of at least five repetitions"
    res = {}
    if "files" in a.only.split(","):
        res["files"] = files(a.n, a.reps, a.blocks, a.threads)
    if "seam" in a.only.split(","):
        res["seam"] = seam(a.n, a.reps, a.blocks)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
