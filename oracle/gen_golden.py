#!/usr/bin/env python3
"""Generate tests/golden/ from the GENUINE reference (oracle/_ref/libjpegref.so).

Run in the authoring container (needs /root/reference):   python oracle/gen_golden.py
The reference itself cannot travel to the GPU box; these vectors (inputs + expected outputs,
plain data) do.  Nothing here is reference source text.

Fixtures written:
  tests/golden/images/*.jpg      the reference's own sample files (data files, images/)
  tests/golden/<name>.npz        per baseline image: desc, qtabs, coefficient blocks after
                                 decodeHuffman() (int16, decode order), RGB after
                                 YCbCrToRGB() (cropped), sha256 of the RGB bytes; where
                                 that file would pass 1 MiB, the RGB rows go to bands
                                 <name>.rgb<k>.npz, k = 0, 1, ... instead
  tests/golden/kat_blocks.npz    known-answer vectors through the reference hot path on
                                 synthetic blocks: DC-only, single-coefficient impulses,
                                 max-magnitude, truncation-stress and full-range random blocks
                                 in 4:4:4 / 4:2:2 / 4:4:0 / 4:2:0 with ragged sizes
  tests/golden/manifest.json     sizes + hashes + reference timings measured here
  tests/golden/ref_results.json  sha256 digests of what the reference returns in the cases of
                                 tests/test_oracle.py that compare with it directly (random blocks,
                                 the build's writer streams through its reader), for runs without it
"""
import glob
import hashlib
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.pyoracle import Ref, make_desc  # noqa: E402
from jpeg_decoder_amd import synth  # noqa: E402

REF_IMAGES = "/root/reference/images"
GOLD = os.path.join(ROOT, "tests", "golden")
BASELINE = ["img", "img2", "img3", "img4", "img5", "img6"]
MAX_FIXTURE_BYTES = 1 << 20   # no fixture file above 1 MiB


def kat_cases():
    """-> list of (name, width, height, hs, vs, qtab_id, coef, qtabs)."""
    q = synth.annex_k_qtabs(90)
    q[2] = np.arange(1, 65, dtype=np.uint16)   # a third, distinct table
    q[3] = 255                                 # the largest table the reference can hold
    cases = []
    layouts = [(1, 1), (2, 1), (1, 2), (2, 2)]
    for hs, vs in layouts:
        tag = f"{hs}x{vs}"
        for (w, h) in [(8, 8), (17, 9), (33, 47), (64, 40)]:
            _, _, bpm, n = synth.geometry(w, h, hs, vs)
            cases.append((f"rand_full_{tag}_{w}x{h}", w, h, hs, vs, (0, 1, 2),
                          synth.random_blocks(n, 1000 + w + h + hs * 7 + vs), q))
            cases.append((f"rand_small_{tag}_{w}x{h}", w, h, hs, vs, (0, 1, 1),
                          synth.random_blocks(n, 2000 + w + h + hs * 7 + vs, -255, 255), q))
            c, _ = synth.synth_blocks(w, h, hs, vs, image_index=w + h, qtabs=q, qtab_id=(0, 1, 2))
            cases.append((f"stat_{tag}_{w}x{h}", w, h, hs, vs, (0, 1, 2), c, q))
        # q = 255 everywhere with extreme coefficients: the largest magnitudes the reference
        # can produce without signed overflow
        _, _, bpm, n = synth.geometry(24, 16, hs, vs)
        ext = synth.random_blocks(n, 77 + hs + vs)
        ext[::3] = 32767
        ext[1::3] = -32768
        cases.append((f"extreme_{tag}", 24, 16, hs, vs, (3, 3, 3), ext, q))
    # impulse / DC-only blocks, 4:4:4, one MCU per impulse position (64 MCUs in a row)
    n = 64 * 3
    imp = np.zeros((n, 64), np.int16)
    for k in range(64):
        imp[3 * k + 0, k] = 37          # luma impulse at natural index k
        imp[3 * k + 1, k] = -19         # Cb
        imp[3 * k + 2, 63 - k] = 23     # Cr
    cases.append(("impulse_1x1", 512, 8, 1, 1, (0, 1, 1), imp, q))
    dc = np.zeros((n, 64), np.int16)
    dc[:, 0] = np.arange(n) * 11 - 1000
    cases.append(("dc_only_1x1", 512, 8, 1, 1, (0, 1, 1), dc, q))
    return cases


def save_image_fixture(name, desc, q, coef, rgb):
    """<name>.npz with every array, or, where that file would pass MAX_FIXTURE_BYTES, <name>.npz without the
    pixels and as few row bands <name>.rgb<k>.npz as keep each file within it (tests/conftest.py load_golden)."""
    path = os.path.join(GOLD, name + ".npz")
    for stale in glob.glob(os.path.join(GOLD, name + ".rgb*.npz")):
        os.remove(stale)
    np.savez_compressed(path, desc=desc, qtabs=q, coef=coef, rgb=rgb)
    if os.path.getsize(path) <= MAX_FIXTURE_BYTES:
        return
    np.savez_compressed(path, desc=desc, qtabs=q, coef=coef)
    for bands in range(2, rgb.shape[0] + 1):
        edges = np.linspace(0, rgb.shape[0], bands + 1).astype(int)
        parts = [os.path.join(GOLD, f"{name}.rgb{k}.npz") for k in range(bands)]
        for part, a, b in zip(parts, edges[:-1], edges[1:]):
            np.savez_compressed(part, rgb=rgb[a:b])
        if all(os.path.getsize(part) <= MAX_FIXTURE_BYTES for part in parts):
            return
        for part in parts:
            os.remove(part)
    raise RuntimeError(f"{name}: no split of the pixels keeps every fixture file within {MAX_FIXTURE_BYTES} bytes")


# the cases of tests/test_oracle.py that call the reference build itself (keep the two in step)
RANDOM_BLOCK_SAMPLINGS = [(1, 1), (2, 1), (1, 2), (2, 2)]
RANDOM_BLOCK_SIZES = [(8, 8, 1), (100, 52, 2), (257, 131, 3)]
WRITER_CASES = [(679, 451, 2, 2, 0), (333, 211, 1, 1, 0), (100, 60, 2, 1, 0), (64, 80, 1, 2, 0), (640, 360, 1, 1, 2), (512, 256, 2, 2, 1)]


def sha256_of(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def write_ref_results(ref):
    """tests/golden/ref_results.json: the reference's answers in the cases of tests/test_oracle.py that ask it directly."""
    import tempfile
    from oracle.pyoracle import Oracle
    ora = Oracle()
    out = {"random_blocks": {}, "writer_streams": {}}
    for hs, vs in RANDOM_BLOCK_SAMPLINGS:
        q = synth.annex_k_qtabs(75)
        q[2] = 255
        q[3] = 1
        for (w, h, seed) in RANDOM_BLOCK_SIZES:
            d = make_desc(w, h, hs, vs, (0, 1, 2))
            n = ora.geometry(d).n_coded_blocks
            for kind, coef in (("full", synth.random_blocks(n, seed)), ("small", synth.random_blocks(n, seed + 10, -64, 64))):
                out["random_blocks"][f"{hs}x{vs}/{w}x{h}/seed{seed}/{kind}"] = sha256_of(ref.blocks_to_rgb(d, coef, q))
    with tempfile.TemporaryDirectory() as tmp:
        for (w, h, hs, vs, rows) in WRITER_CASES:
            coef, q = synth.synth_blocks(w, h, hs, vs, 21)
            data = synth.encode_jpeg(coef, w, h, hs, vs, q, restart_interval=rows * synth.geometry(w, h, hs, vs)[0])
            path = os.path.join(tmp, "w.jpg")
            with open(path, "wb") as f:
                f.write(data)
            info, rcoef, rq, rrgb = ref.decode_file(path)
            assert np.array_equal(rcoef.astype(coef.dtype), rcoef) and np.array_equal(rq.astype(q.dtype), rq)
            out["writer_streams"][f"{w}x{h}/{hs}x{vs}/rows{rows}"] = {
                "stream_sha256": sha256_of(np.frombuffer(data, np.uint8)),
                "frame": [info.width, info.height, info.hs, info.vs],
                "coef_sha256": sha256_of(rcoef.astype(coef.dtype)), "qtabs01_sha256": sha256_of(rq[:2].astype(q.dtype)),
                "rgb_sha256": sha256_of(rrgb)}
    with open(os.path.join(GOLD, "ref_results.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


def main():
    ref = Ref()
    os.makedirs(os.path.join(GOLD, "images"), exist_ok=True)
    manifest = {"constants_f32_bits": [int(x) for x in ref.constants()], "images": {}, "kat": {}}
    for name in BASELINE + ["prograssive-sample-2"]:
        shutil.copyfile(os.path.join(REF_IMAGES, name + ".jpg"), os.path.join(GOLD, "images", name + ".jpg"))
        os.chmod(os.path.join(GOLD, "images", name + ".jpg"), 0o644)
    for name in BASELINE:
        path = os.path.join(REF_IMAGES, name + ".jpg")
        info, coef, q, rgb = ref.decode_file(path)
        sha = hashlib.sha256(rgb.tobytes()).hexdigest()
        desc = np.array([info.width, info.height, info.hs, info.vs, *info.qtab_id, info.restart_interval,
                         info.mcu_w_real, info.mcu_h_real], np.int32)
        save_image_fixture(name, desc, q, coef, rgb)
        manifest["images"][name] = {
            "file_sha256": hashlib.sha256(open(path, "rb").read()).hexdigest(),
            "width": info.width, "height": info.height, "hs": info.hs, "vs": info.vs,
            "qtab_id": list(info.qtab_id), "restart_interval": info.restart_interval,
            "mcu_w_real": info.mcu_w_real, "mcu_h_real": info.mcu_h_real,
            "n_coded_blocks": info.n_coded_blocks, "coef_range": [info.coef_min, info.coef_max],
            "rgb_sha256": sha,
            "ref_ms": {"huffman": round(info.ms_huffman, 3), "dequant": round(info.ms_dequant, 3),
                       "idct": round(info.ms_idct, 3), "colour": round(info.ms_colour, 3)},
        }
        print(name, info.width, info.height, sha[:16])
    kat = {}
    for (name, w, h, hs, vs, qid, coef, q) in kat_cases():
        d = make_desc(w, h, hs, vs, qid)
        rgb = ref.blocks_to_rgb(d, coef, q)
        kat[name + "__desc"] = np.array([w, h, hs, vs, *qid], np.int32)
        kat[name + "__qtabs"] = q
        kat[name + "__coef"] = coef
        kat[name + "__rgb"] = rgb
        manifest["kat"][name] = hashlib.sha256(rgb.tobytes()).hexdigest()
    np.savez_compressed(os.path.join(GOLD, "kat_blocks.npz"), **kat)
    write_ref_results(ref)
    with open(os.path.join(GOLD, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("kat cases:", len(manifest["kat"]))


if __name__ == "__main__":
    main()
