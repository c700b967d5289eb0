#!/usr/bin/env python3
"""What an orientation other than 1 costs at the seam; bench.py is untouched (it measures orientation 1, whose launches
do not change).  ONE process, device-resident coefficients, one stream, every side of a comparison alternating in
blocks, HIP events around every call; reported are the block medians' median and spread.  Per shape and format:

  baseline     the orientation-1 launch in that format: the path as it was, never the code under test
  pixel_fmt0   the orientation-1 launch in format 0, tight: what an oriented launch runs first, into its scratch
  o2 .. o8     the oriented launch (pixel kernel into the scratch + jb_orient_kernel into the output)
  torch_o*     what a user does without the feature: the orientation-1 launch, then torch flip / transpose(...).contiguous()
  memcpy       hipMemcpyAsync device-to-device moving the bytes jb_orient_kernel moves (3 B read + the output's bytes
               written per pixel): the math-free ceiling

and derived from them: orient_kernel_us = o* - pixel_fmt0, its share of the memcpy ceiling, o* / baseline next to the
byte-count prediction (4:4:4, format 0: 6 + 3 B of the pixel kernel, + 3 + 3 B of the extra pass = 15 / 9 = 1.67x), and
the slowest transposing over the slowest mirroring orientation (above 1.25x a counter run is owed: DESIGN.md 5.14).

Usage: python tools/orient_bench.py [--out profiles/r12/orient_bench.json] [--launches 10] [--repeats 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpeg_decoder_amd as jb  # noqa: E402
from jpeg_decoder_amd.api import torch_batch  # noqa: E402

SHAPES = [(8, 4096, 4096, 1, 1), (32, 1920, 1080, 2, 2)]
MIRRORING, TRANSPOSING = (2, 3, 4), (5, 6, 7, 8)


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
    """-> {side: (the median of its block medians in us, their spread in % of it)}"""
    for fn in sides.values():
        _block(stream, fn, max(1, launches // 2))   # pre-conditioning, untimed
    med = {k: [] for k in sides}
    for _ in range(repeats):                        # interleaved blocks: drift hits every side alike
        for k, fn in sides.items():
            med[k].append(float(np.median(_block(stream, fn, launches))) * 1e3)
    return {k: (round(float(np.median(v)), 1), round(float((max(v) - min(v)) / np.median(v) * 100), 2)) for k, v in med.items()}


def _coefficients(n, desc, seed):
    """n images of small random coefficients (the kernels' time does not depend on the values) and quality-90 tables"""
    import torch
    from jpeg_decoder_amd.synth import annex_k_qtabs
    g = jb.geometry_of(desc)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(seed)
    coef = torch.randint(-8, 9, (n, g.n_coded_blocks, 64), dtype=torch.int16, device="cuda:0", generator=gen)
    q = torch.from_numpy(jb.resolve_qtabs(desc, annex_k_qtabs(90))).to("cuda:0")
    return coef, q


def _torch_orient(t, o, planar):
    """T_o of a batch [n, H, W, 3] (planar: [n, 3, H, W]) as a user writes it in torch"""
    y, x = (2, 3) if planar else (1, 2)
    r = {2: lambda: t.flip(x), 3: lambda: t.flip(y, x), 4: lambda: t.flip(y), 5: lambda: t.transpose(y, x),
         6: lambda: t.transpose(y, x).flip(x), 7: lambda: t.flip(y, x).transpose(y, x), 8: lambda: t.transpose(y, x).flip(y)}[o]()
    return r.contiguous()


def run(launches, repeats):
    import torch
    res = {"launches_per_block": launches, "blocks": repeats}
    with jb.Context(0) as plain:
        ctxs = {o: jb.Context(0, orientation=o) for o in range(2, 9)}
        stream = torch.cuda.ExternalStream(plain.stream)
        try:
            for n, w, h, hs, vs in SHAPES:
                desc = jb.make_desc(w, h, hs, vs)
                coef, q = _coefficients(n, desc, n + w)
                for fmt in (jb.FMT_RGB_U8_HWC, jb.FMT_RGB_F16_CHW):
                    planar = fmt != jb.FMT_RGB_U8_HWC
                    spec = jb.OutputSpec.imagenet(fmt) if planar else None
                    dt = torch.float16 if planar else torch.uint8

                    def out_of(ow, oh):
                        return torch.zeros((n, 3, oh, ow) if planar else (n, oh, ow, 3), dtype=dt, device="cuda:0")

                    stored, turned = out_of(w, h), out_of(h, w)
                    tight = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda:0")

                    def batch_for(o, out):
                        # torch_batch reads the output's strides from `out` and checks them against the descriptor it is
                        # given: hand it the ORIENTED size for that, then put the stored frame's descriptor back -- the
                        # launch wants the stored frame and strides of the oriented output
                        ow, oh = jb.oriented_size(w, h, o)
                        b = torch_batch(jb.make_desc(ow, oh, hs, vs), n, coef, q, out, fmt=spec)   # (strides of the oriented output)
                        b.desc = desc
                        return b

                    b1 = batch_for(1, stored)
                    b0 = torch_batch(desc, n, coef, q, tight)
                    sides = {"baseline": lambda: plain.blocks_to_rgb_device(b1, stream=plain.stream, fmt=spec),
                             "pixel_fmt0": lambda: plain.blocks_to_rgb_device(b0, stream=plain.stream)}
                    moved = (tight.numel() + stored.numel() * stored.element_size()) // 2    # a copy of B bytes moves 2 B
                    src = torch.zeros(moved, dtype=torch.uint8, device="cuda:0")
                    dst = torch.empty_like(src)

                    def memcpy():
                        with torch.cuda.stream(stream):
                            dst.copy_(src)

                    sides["memcpy"] = memcpy
                    for o in range(2, 9):
                        bo = batch_for(o, turned if o >= 5 else stored)
                        sides[f"o{o}"] = lambda o=o, bo=bo: ctxs[o].blocks_to_rgb_device(bo, stream=plain.stream, fmt=spec)

                        def user(o=o):
                            plain.blocks_to_rgb_device(b1, stream=plain.stream, fmt=spec)
                            with torch.cuda.stream(stream):
                                _torch_orient(stored, o, planar)

                        sides[f"torch_o{o}"] = user
                    m = _alternate(stream, sides, launches, repeats)
                    r = {k + "_us": v[0] for k, v in m.items()}
                    r.update({k + "_spread_pct": v[1] for k, v in m.items()})
                    for o in range(2, 9):
                        k_us = m[f"o{o}"][0] - m["pixel_fmt0"][0]
                        r[f"o{o}_orient_kernel_us"] = round(k_us, 1)
                        r[f"o{o}_share_of_memcpy_ceiling"] = round(m["memcpy"][0] / k_us, 3) if k_us > 0 else None
                        r[f"o{o}_over_baseline"] = round(m[f"o{o}"][0] / m["baseline"][0], 3)
                        r[f"o{o}_over_torch"] = round(m[f"o{o}"][0] / m[f"torch_o{o}"][0], 3)
                    px = 6.0 if hs == 1 else 3.0                 # coefficient bytes per pixel
                    es = stored.element_size()
                    r["predicted_over_baseline_by_bytes"] = round((px + 3 + 3 + 3 * es) / (px + 3 * es), 3)
                    r["memcpy_bytes"] = int(moved)
                    r["slowest_transposing_over_slowest_mirroring"] = round(max(m[f"o{o}"][0] for o in TRANSPOSING) / max(m[f"o{o}"][0] for o in MIRRORING), 3)
                    res[f"{n}x{w}x{h}-{'444' if hs == 1 else '420'}-fmt{fmt}"] = r
                    del stored, turned, tight, src, dst
                    torch.cuda.empty_cache()
                del coef
                torch.cuda.empty_cache()
        finally:
            for c in ctxs.values():
                c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run(a.launches, a.repeats)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
