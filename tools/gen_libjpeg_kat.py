#!/usr/bin/env python3
"""Known-answer vectors of "decoder arithmetic" JB_ARITH_LIBJPEG (include/jpegblk.h) from Pillow itself: writes
tests/golden/libjpeg_decode_kat.npz -- per case k the file's bytes jpeg_k, its name name_k and rgb_k =
Image.open(jpeg).convert("RGB"), and the Pillow version that decoded them -- so that a machine without Pillow still
tests against libjpeg's own bits (tests/test_libjpeg_cpu.py, tests/test_gpu_libjpeg.py).  Before anything is written,
tests/libjpeg_ref.py must give Pillow's bits for every case from the host front end's coefficients: only cases inside
the contract's domain are kept.  Run it where Pillow is installed; the file stays under 256 KB."""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
OUT = os.path.join(ROOT, "tests", "golden", "libjpeg_decode_kat.npz")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SUB = {"444": 0, "422": 1, "420": 2}   # Pillow's subsampling= values


def pixels(w, h, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    # smooth: gradients with a little noise (compresses well; chroma still varies from sample to sample)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + 2 * y) * 7) % 256], axis=-1)
    return np.clip(base + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


def pillow_file(w, h, kind, sub, quality, seed, mode="RGB", **save):
    from PIL import Image
    px = pixels(w, h, kind, seed)
    im = Image.fromarray(px if mode == "RGB" else px[:, :, 0], mode)
    f = io.BytesIO()
    if mode == "RGB":
        save["subsampling"] = SUB[sub]
    im.save(f, "JPEG", quality=quality, **save)
    return f.getvalue()


def synth_file(w, h, hs, vs, seed):
    from jpeg_decoder_amd import synth
    coef, q = synth.synth_blocks(w, h, hs, vs, image_index=seed)
    return synth.encode_jpeg(coef, w, h, hs, vs, q)


def cases():
    """-> [(name, jpeg bytes)]"""
    out = [("420_521x37_noise_q95", pillow_file(521, 37, "noise", "420", 95, 1)),   # 33 MCUs: two tiles per row; 3 MCU rows; odd W, H
           ("444_521x19", pillow_file(521, 19, "smooth", "444", 90, 2)),
           ("422_1033x11", pillow_file(1033, 11, "smooth", "422", 90, 3)),             # 65 MCUs: across the 64-MCU tile
           ("440_515x37_synth", synth_file(515, 37, 1, 2, 4))]                         # Pillow cannot write 4:4:0; it reads it
    for i, (w, h) in enumerate(((1, 1), (2, 1), (3, 5), (4, 4), (5, 3), (17, 1))):
        out.append((f"420_{w}x{h}", pillow_file(w, h, "noise", "420", 90, 10 + i)))
    for i, (w, h) in enumerate(((3, 5), (5, 3))):
        out.append((f"422_{w}x{h}", pillow_file(w, h, "noise", "422", 90, 20 + i)))
    out.append(("420_40x24_binary_q100", pillow_file(40, 24, "binary", "420", 100, 30)))   # both clamps, IDCT and colour
    out.append(("420_40x24_binary_q30", pillow_file(40, 24, "binary", "420", 30, 31)))
    out.append(("gray_33x21", pillow_file(33, 21, "smooth", None, 90, 40, mode="L")))
    out.append(("420_45x35_progressive", pillow_file(45, 35, "smooth", "420", 85, 41, progressive=True)))
    out.append(("420_70x40_restart", pillow_file(70, 40, "smooth", "420", 85, 42, restart_marker_blocks=2)))
    return out


def main():
    import PIL
    from PIL import Image
    import jpeg_decoder_amd as jb
    import libjpeg_ref
    data = {"pillow_version": np.array(PIL.__version__)}
    all_cases = cases()
    for k, (name, jpeg) in enumerate(all_cases):
        rgb = np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))
        desc, q, coef = jb.entropy_decode(jpeg)
        ours = libjpeg_ref.decode_blocks(desc, q, coef.reshape(-1, 64))   # (raises outside the domain)
        assert ours.shape == rgb.shape and np.array_equal(ours, rgb), f"{name}: libjpeg_ref differs from Pillow in {int((ours != rgb).sum())} bytes"
        data[f"name_{k}"] = np.array(name)
        data[f"jpeg_{k}"] = np.frombuffer(jpeg, np.uint8)
        data[f"rgb_{k}"] = rgb
    data["n"] = np.array(len(all_cases))
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    assert size < 256 * 1024, size
    print(f"{len(all_cases)} cases from Pillow {PIL.__version__} -> {OUT} ({size} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
