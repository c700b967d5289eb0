import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
BASELINE_IMAGES = ["img", "img2", "img3", "img4", "img5", "img6"]


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run on the GPU box with -m gpu)")


@pytest.fixture(scope="session")
def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def load_golden(name):
    """-> (desc, coef, qtabs, rgb) of one baseline image fixture.  A fixture too large for one file keeps
    its RGB rows in bands <name>.rgb<k>.npz (oracle/gen_golden.py): joined here, and checked against the
    digest manifest.json records."""
    from oracle.pyoracle import make_desc
    z = np.load(os.path.join(GOLD, name + ".npz"))
    d = z["desc"]
    if "rgb" in z.files:
        rgb = z["rgb"]
    else:
        bands = []
        while os.path.exists(os.path.join(GOLD, f"{name}.rgb{len(bands)}.npz")):
            bands.append(np.load(os.path.join(GOLD, f"{name}.rgb{len(bands)}.npz"))["rgb"])
        rgb = np.concatenate(bands, axis=0)
        with open(os.path.join(GOLD, "manifest.json")) as f:
            want = json.load(f)["images"][name]["rgb_sha256"]
        assert hashlib.sha256(rgb.tobytes()).hexdigest() == want, f"{name}: the RGB bands do not join to the recorded image"
    return make_desc(d[0], d[1], d[2], d[3], d[4:7]), z["coef"], z["qtabs"], rgb


def load_kat():
    """-> {case: (desc, coef, qtabs, rgb)} of the known-answer block vectors."""
    from oracle.pyoracle import make_desc
    z = np.load(os.path.join(GOLD, "kat_blocks.npz"))
    names = sorted({k.split("__")[0] for k in z.files})
    out = {}
    for n in names:
        d = z[n + "__desc"]
        out[n] = (make_desc(d[0], d[1], d[2], d[3], d[4:7]), z[n + "__coef"], z[n + "__qtabs"], z[n + "__rgb"])
    return out
