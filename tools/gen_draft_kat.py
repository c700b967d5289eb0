#!/usr/bin/env python3
"""Known-answer vectors of "draft decode" (include/jpegblk.h) from Pillow itself: writes
tests/golden/libjpeg_draft_kat.npz -- per case k its name name_k and, for K = 2, 4, 8, rgb_k_K = Pillow's decode of the
file at libjpeg scale 1 / K (forced the way JpegImageFile.draft sets it: tests/draft_ref.py pillow_draft), and the Pillow
version that decoded them.  The cases are every file of libjpeg_decode_kat.npz -- taken from that file by name, not stored
again -- plus, with their bytes jpeg_k, one Pillow-written file per layout of about 131 x 70 and a 4:4:0 one from synth.
Before anything is written tests/draft_ref.py must give Pillow's bits for every case at every K from the host front
end's coefficients: a case that differs or leaves the contract's domain fails the run, none is dropped.  Run it where
Pillow is installed; the file stays under 256 KB."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
OUT = os.path.join(ROOT, "tests", "golden", "libjpeg_draft_kat.npz")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)


def own_cases():
    """-> [(name, jpeg bytes)]: the files this KAT stores itself"""
    from gen_libjpeg_kat import pillow_file, synth_file
    return [("draft_444_131x70", pillow_file(131, 70, "smooth", "444", 90, 50)),
            ("draft_422_131x70", pillow_file(131, 70, "smooth", "422", 90, 51)),
            ("draft_420_131x70", pillow_file(131, 70, "smooth", "420", 90, 52)),
            ("draft_gray_131x70", pillow_file(131, 70, "smooth", None, 90, 53, mode="L")),
            ("draft_440_131x70_synth", synth_file(131, 70, 1, 2, 54))]


def main():
    import PIL
    import jpeg_decoder_amd as jb
    import draft_ref
    import libjpeg_ref
    data = {"pillow_version": np.array(PIL.__version__)}
    cases = [(name, jpeg, False) for name, jpeg, _ in libjpeg_ref.load_kat()] + [(name, jpeg, True) for name, jpeg in own_cases()]
    for k, (name, jpeg, store) in enumerate(cases):
        desc, q, coef = jb.entropy_decode(jpeg)
        data[f"name_{k}"] = np.array(name)
        if store:
            data[f"jpeg_{k}"] = np.frombuffer(jpeg, np.uint8)
        for K in draft_ref.DENOMS:
            rgb = draft_ref.pillow_draft(jpeg, K)
            ours = draft_ref.decode_blocks(desc, q, coef.reshape(-1, 64), K)   # (raises outside the domain)
            assert ours.shape == rgb.shape and np.array_equal(ours, rgb), \
                f"{name} at 1/{K}: draft_ref {ours.shape} differs from Pillow {rgb.shape} in {int((ours != rgb).sum()) if ours.shape == rgb.shape else -1} bytes"
            data[f"rgb_{k}_{K}"] = rgb
    data["n"] = np.array(len(cases))
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    assert size < 256 * 1024, size
    print(f"{len(cases)} cases x {len(draft_ref.DENOMS)} drafts from Pillow {PIL.__version__} -> {OUT} ({size} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
