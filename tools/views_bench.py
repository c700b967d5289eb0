#!/usr/bin/env python3
"""What views= saves: K crops of a file from ONE decode, the mirror in the resample kernel's store; bench.py is untouched.
All runs in ONE process on one device, in alternating blocks of at least five repetitions; reported are the block
medians, their median, and the block-to-block spread of every side (the baseline's is the yardstick).

  seam   N device-resident 1920x1080 4:2:0 images, K = 2 random_views each -> 224 x 224 normalised f16 CHW.  One
         views= call against (baseline) the shipped crops= route over every image once per view -- the same
         coefficients listed K times, without the copy -- and against that route plus torch.flip on the mirrored
         outputs (what a user does today).  The outputs are compared bit for bit.  HIP events around every side.
  files  BatchDecoder with device output over N 1080p 4:2:0 files, K = 1 with mirrors and K = 2: run_to_device(paths,
         views=) against run_to_device(paths * K, crops=) (baseline: K entropy decodes per file) and that plus the flip
         of the mirrored outputs.  Wall clock around the call and a device synchronize; views per second.

  --sides views (or another side's name): the seam workload with that side alone and no comparison -- for a kernel trace
  of its own (rocprofv3 --kernel-trace --stats -- python tools/views_bench.py --only seam --sides views), whose
  per-kernel times then belong to one side.

Usage: python tools/views_bench.py [--only seam,files] [--n 1024] [--reps 5] [--blocks 3] [--sides a,b] [--out profiles/r13/views_bench.json]
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
PER = 3 * TW * TH * 2   # bytes of one f16 CHW output (a multiple of 256)


def _summary(blocks):
    m = np.array(blocks)
    return {"block_medians": [round(float(x), 3) for x in m], "median": round(float(np.median(m)), 3),
            "spread_pct": round(float((m.max() - m.min()) / np.median(m) * 100), 2)}


def _alternate(sides, time_one, reps, blocks):
    """-> {side: _summary of its block medians}; interleaved blocks: drift hits every side alike"""
    for fn in sides.values():
        time_one(fn), time_one(fn)   # pre-conditioning, untimed
    med = {k: [] for k in sides}
    for _ in range(blocks):
        for k, fn in sides.items():
            med[k].append(float(np.median([time_one(fn) for _ in range(reps)])))
    return {k: _summary(v) for k, v in med.items()}


def seam(n, reps, blocks, only_sides=None):
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    k = 2
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
        views = [jb.random_views(W, H, rng, k) for _ in range(n)]
        out_v = torch.zeros((n, k, 3, TH, TW), dtype=torch.float16, device="cuda:0")
        out_c = torch.zeros((n, k, 3, TH, TW), dtype=torch.float16, device="cuda:0")
        bv = torch_batch(desc, n, coef, q, out_v.view(n * k, 3, TH, TW), fmt=spec, resize=(TW, TH))
        # the baseline's batches: view v of every image, the outputs K apart
        bc = []
        for v in range(k):
            b = torch_batch(desc, n, coef, q, out_c[:, v], fmt=spec, resize=(TW, TH))
            bc.append((b, [row[v][:4] for row in views]))
        mirrored = torch.tensor([[bool(v[4]) for v in row] for row in views], device="cuda:0")
        mi, mv = mirrored.nonzero(as_tuple=True)   # (made once: the flip below costs no synchronisation)

        def with_views():
            ctx.blocks_to_rgb_device(bv, fmt=spec, resize=(TW, TH), views=views)

        def crops_per_view():
            for b, crops in bc:
                ctx.blocks_to_rgb_device(b, fmt=spec, resize=(TW, TH), crops=crops)

        def crops_and_flip():
            crops_per_view()
            with torch.cuda.stream(stream):
                out_c[mi, mv] = out_c[mi, mv].flip(-1)

        def time_one(fn):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            e.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(e) * 1e3   # us

        sides = {"views": with_views, "crops_per_view": crops_per_view, "crops_per_view_and_flip": crops_and_flip}
        if only_sides:
            return {"sides": _alternate({k: sides[k] for k in only_sides}, time_one, reps, blocks), "unit": "us per batch"}
        res = _alternate(sides, time_one, reps, blocks)
        with_views(), crops_and_flip()
        torch.cuda.synchronize()
        assert torch.equal(out_v, out_c), "views= and crops= + flip differ"
        out = {"batch": f"{n}x{W}x{H}-420", "views_per_image": k, "target": [TW, TH], "format": "RGB_F16_CHW", "unit": "us per batch",
               "same_bits": True, "mirrored_views": int(mirrored.sum()), "sides": res}
        for side in ("crops_per_view", "crops_per_view_and_flip"):
            out["views_speedup_over_" + side] = round(res[side]["median"] / res["views"]["median"], 3)
        out["us_per_view"] = round(res["views"]["median"] / (n * k), 3)
        return out


def _files(n, out_dir):
    from jpeg_decoder_amd import synth
    paths = []
    for i in range(8):   # eight distinct files, repeated: as the other benches do
        coef, q = synth.synth_blocks(W, H, 2, 2, i)
        p = os.path.join(out_dir, f"views_{W}x{H}_420_{i}.jpg")
        with open(p, "wb") as f:
            f.write(synth.encode_jpeg(coef, W, H, 2, 2, q, restart_interval=0))
        paths.append(p)
    return [paths[i % 8] for i in range(n)]


def files(n, reps, blocks, threads):
    import torch
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    out = {"batch": f"{n} files {W}x{H}-420", "target": [TW, TH], "format": "RGB_F16_CHW", "threads": threads, "unit": "ms per batch"}
    with tempfile.TemporaryDirectory() as tmp:
        paths = _files(n, tmp)
        for k in (1, 2):
            rng = np.random.default_rng(n + k)
            views = [jb.random_views(W, H, rng, k, p_mirror=0.5) for _ in range(n)]
            flat_paths = [p for p in paths for _ in range(k)]
            flat_crops = [v[:4] for row in views for v in row]
            flat_mirror = np.array([bool(v[4]) for row in views for v in row])
            region = torch.zeros((n * k * PER + 256 * (n + 2),), dtype=torch.uint8, device="cuda:0")
            elems = torch.arange(PER // 2, device="cuda:0")
            with jb.BatchDecoder(threads, 0, resize=(TW, TH), fmt=spec) as dec:
                dec.set_device_output(region.data_ptr(), region.numel())
                n_dev = {}

                def with_views():
                    n0 = dec.device_entropy_images
                    _, _, st, tm = dec.run_to_device(paths, views=views)
                    n_dev["views"] = dec.device_entropy_images - n0
                    assert tm["rc"] == 0 and not any(st), (tm, [s for s in st if s][:4])

                def crops_k_times(flip=False):
                    n0 = dec.device_entropy_images
                    ptrs, _, st, tm = dec.run_to_device(flat_paths, crops=flat_crops)
                    n_dev["crops"] = dec.device_entropy_images - n0
                    assert tm["rc"] == 0 and not any(st), (tm, [s for s in st if s][:4])
                    if flip:   # the mirrored outputs, gathered, flipped, put back
                        off = torch.tensor([(p - region.data_ptr()) // 2 for p, m in zip(ptrs, flat_mirror) if m], device="cuda:0")
                        at = off[:, None] + elems[None, :]
                        r16 = region[:region.numel() // 2 * 2].view(torch.float16)
                        r16[at] = r16[at].view(-1, 3, TH, TW).flip(-1).reshape(at.shape)

                def time_one(fn):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3   # ms

                res = _alternate({"views": with_views, "crops_k_times": crops_k_times, "crops_k_times_and_flip": lambda: crops_k_times(True)},
                                 time_one, reps, blocks)
            r = {"sides": res, "device_entropy_images_per_batch": dict(n_dev), "mirrored_views": int(flat_mirror.sum())}
            for side, s in res.items():
                r[side + "_views_per_s"] = round(n * k / (s["median"] * 1e-3))
            for side in ("crops_k_times", "crops_k_times_and_flip"):
                r["views_speedup_over_" + side] = round(res[side]["median"] / res["views"]["median"], 3)
            out[f"k{k}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="seam,files")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sides", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5, "blocks of at least five repetitions"
    res = {}
    if "seam" in a.only.split(","):
        res["seam"] = seam(a.n, a.reps, a.blocks, a.sides.split(",") if a.sides else None)
    if "files" in a.only.split(","):
        res["files"] = files(a.n, a.reps, a.blocks, a.threads)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
