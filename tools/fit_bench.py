#!/usr/bin/env python3
"""What fit= costs and saves: a letterboxed target against the stretched one, and against the torch route a user takes
today for a letterbox; bench.py is untouched.  All runs in ONE process on one device, in alternating blocks of at least
five repetitions; reported are the block medians, their median, and the block-to-block spread of every side (the
baseline's is the yardstick).  Nothing here is a gate.

  seam   N device-resident 1920x1080 4:2:0 images -> 224 x 224 normalised f16 CHW.  Fit.pad (a 224 x 126 inner rectangle
         and two bands of 49 rows: the resample kernel computes 126 of 224 rows, jb_fit_fill_kernel stores the other 98)
         against (baseline) the stretch to 224 x 224, against Fit.cover, and against the torch route: the full-size decode,
         then torch.nn.functional.interpolate to 224 x 126, the normalisation, and the paste into a filled canvas.  The
         letterbox's border is checked to hold the fill.  HIP events around every side.  (The torch route always
         interpolates bilinear with antialias=True, whatever --filter says: torch has no exact area filter for these
         sizes, so its values differ and with the default area filter it is not like for like -- timing only.)
  files  BatchDecoder with device output over N 1080p 4:2:0 files: run_to_device(paths) with Fit.pad against the stretch
         (baseline) and against the torch route over full-size device output.  Wall clock around the call and a device
         synchronize; images per second.

  --sides pad (or another side's name): the seam workload with that side alone and no check -- for a kernel trace of its
  own (rocprofv3 --kernel-trace --stats -- python tools/fit_bench.py --only seam --sides pad).

Usage: python tools/fit_bench.py [--only seam,files] [--n 1024] [--reps 5] [--blocks 3] [--filter 0] [--sides a,b] [--out profiles/r14/fit_bench.json]
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
FILL = (124, 116, 104)
PER = 3 * TW * TH * 2   # bytes of one f16 CHW output (a multiple of 256)
CHUNK = 64              # images the torch route holds as float32 at a time


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


def _torch_letterbox(full_u8, out, inner, scale, bias, fill):
    """full_u8 [n, H, W, 3] uint8 -> out [n, 3, TH, TW] f16: what a user writes today, CHUNK images at a time"""
    import torch
    ix, iy, iw, ih = inner
    out[:] = fill
    for i in range(0, full_u8.shape[0], CHUNK):
        x = full_u8[i:i + CHUNK].permute(0, 3, 1, 2).float()
        y = torch.nn.functional.interpolate(x, size=(ih, iw), mode="bilinear", antialias=True)
        out[i:i + CHUNK, :, iy:iy + ih, ix:ix + iw] = (y * scale + bias).half()


def seam(n, reps, blocks, filt, only_sides=None):
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    inner = jb.fit_geometry(W, H, (TW, TH), jb.FIT_PAD, filter=filt)[1]
    with jb.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        desc = jb.make_desc(W, H, 2, 2)
        g = jb.geometry_of(desc)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(n + W)
        coef = torch.randint(-48, 49, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
        q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
        spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
        scale = torch.tensor(list(spec.scale), device="cuda:0").view(1, 3, 1, 1)
        bias = torch.tensor(list(spec.bias), device="cuda:0").view(1, 3, 1, 1)
        fill = (torch.tensor(FILL, dtype=torch.float32, device="cuda:0").view(1, 3, 1, 1) * scale + bias).half()
        out = {k: torch.zeros((n, 3, TH, TW), dtype=torch.float16, device="cuda:0") for k in ("pad", "stretch", "cover", "torch")}
        full = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda:0")
        b = {k: torch_batch(desc, n, coef, q, out[k], fmt=spec, resize=(TW, TH)) for k in ("pad", "stretch", "cover")}
        b_full = torch_batch(desc, n, coef, q, full.view(n, H, 3 * W))
        pad, cover = jb.Fit.pad(FILL), jb.Fit.cover()

        def torch_route():
            ctx.blocks_to_rgb_device(b_full)
            with torch.cuda.stream(stream):
                _torch_letterbox(full, out["torch"], inner, scale, bias, fill)

        sides = {"pad": lambda: ctx.blocks_to_rgb_device(b["pad"], fmt=spec, resize=(TW, TH), filter=filt, fit=pad),
                 "stretch": lambda: ctx.blocks_to_rgb_device(b["stretch"], fmt=spec, resize=(TW, TH), filter=filt),
                 "cover": lambda: ctx.blocks_to_rgb_device(b["cover"], fmt=spec, resize=(TW, TH), filter=filt, fit=cover),
                 "torch_decode_interpolate_pad": torch_route}

        def time_one(fn):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            e.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(e) * 1e3   # us

        if only_sides:
            return {"sides": _alternate({k: sides[k] for k in only_sides}, time_one, reps, blocks), "unit": "us per batch"}
        res = _alternate(sides, time_one, reps, blocks)
        ix, iy, iw, ih = inner
        border = torch.ones((TH, TW), dtype=torch.bool, device="cuda:0")
        border[iy:iy + ih, ix:ix + iw] = False
        assert bool((out["pad"][:, :, border] == fill.view(1, 3, 1)).all()), "the letterbox's border does not hold the fill"
        r = {"batch": f"{n}x{W}x{H}-420", "target": [TW, TH], "inner": list(inner), "filter": filt, "format": "RGB_F16_CHW",
             "unit": "us per batch", "border_holds_fill": True, "sides": res,
             "torch_route": "bilinear, antialias=True whatever the filter: timing only, its values differ"}
        for side in ("stretch", "torch_decode_interpolate_pad"):
            r["pad_speedup_over_" + side] = round(res[side]["median"] / res["pad"]["median"], 3)
        r["us_per_image_pad"] = round(res["pad"]["median"] / n, 3)
        return r


def _files(n, out_dir):
    from jpeg_decoder_amd import synth
    paths = []
    for i in range(8):   # eight distinct files, repeated: as the other benches do
        coef, q = synth.synth_blocks(W, H, 2, 2, i)
        p = os.path.join(out_dir, f"fit_{W}x{H}_420_{i}.jpg")
        with open(p, "wb") as f:
            f.write(synth.encode_jpeg(coef, W, H, 2, 2, q, restart_interval=0))
        paths.append(p)
    return [paths[i % 8] for i in range(n)]


def files(n, reps, blocks, threads, filt):
    import torch
    spec = jb.OutputSpec.imagenet(jb.FMT_RGB_F16_CHW)
    inner = jb.fit_geometry(W, H, (TW, TH), jb.FIT_PAD, filter=filt)[1]
    scale = torch.tensor(list(spec.scale), device="cuda:0").view(1, 3, 1, 1)
    bias = torch.tensor(list(spec.bias), device="cuda:0").view(1, 3, 1, 1)
    fill = (torch.tensor(FILL, dtype=torch.float32, device="cuda:0").view(1, 3, 1, 1) * scale + bias).half()

    def time_one(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3   # ms

    with tempfile.TemporaryDirectory() as tmp:
        paths = _files(n, tmp)
        region = torch.zeros((n * PER + 256 * (n + 2),), dtype=torch.uint8, device="cuda:0")
        full_bytes = 3 * W * H
        full_region = torch.zeros((n * full_bytes + 256 * (n + 2),), dtype=torch.uint8, device="cuda:0")
        out_t = torch.zeros((n, 3, TH, TW), dtype=torch.float16, device="cuda:0")
        with jb.BatchDecoder(threads, 0, resize=(TW, TH), fmt=spec, filter=filt) as dec, jb.BatchDecoder(threads, 0) as plain:
            dec.set_device_output(region.data_ptr(), region.numel())
            plain.set_device_output(full_region.data_ptr(), full_region.numel())

            def run(fit):
                dec.set_fit(fit)
                _, _, st, tm = dec.run_to_device(paths)
                assert tm["rc"] == 0 and not any(st), (tm, [s for s in st if s][:4])

            def torch_route():
                ptrs, _, st, tm = plain.run_to_device(paths)
                assert tm["rc"] == 0 and not any(st), (tm, [s for s in st if s][:4])
                # (an image's address is its own: CHUNK of them stacked, as a user's collate step would)
                off = [p - full_region.data_ptr() for p in ptrs]
                for i in range(0, n, CHUNK):
                    imgs = torch.stack([full_region[o:o + full_bytes].view(H, W, 3) for o in off[i:i + CHUNK]])
                    _torch_letterbox(imgs, out_t[i:i + CHUNK], inner, scale, bias, fill)

            res = _alternate({"pad": lambda: run(jb.Fit.pad(FILL)), "stretch": lambda: run(None), "torch_decode_interpolate_pad": torch_route},
                             time_one, reps, blocks)
    r = {"batch": f"{n} files {W}x{H}-420", "target": [TW, TH], "inner": list(inner), "filter": filt, "format": "RGB_F16_CHW",
         "threads": threads, "unit": "ms per batch", "sides": res}
    for side, s in res.items():
        r[side + "_images_per_s"] = round(n / (s["median"] * 1e-3))
    for side in ("stretch", "torch_decode_interpolate_pad"):
        r["pad_speedup_over_" + side] = round(res[side]["median"] / res["pad"]["median"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="seam,files")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--filter", type=int, default=jb.FILTER_AREA)
    ap.add_argument("--sides", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5, "blocks of at least five repetitions"
    res = {}
    if "seam" in a.only.split(","):
        res["seam"] = seam(a.n, a.reps, a.blocks, a.filter, a.sides.split(",") if a.sides else None)
    if "files" in a.only.split(","):
        res["files"] = files(a.n, a.reps, a.blocks, a.threads, a.filter)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
