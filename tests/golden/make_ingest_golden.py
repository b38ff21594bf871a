"""Writes tests/golden/ingest.npz from Pillow: for every case of tests/ingest_cases.py the cropped uint8 image Pillow
gives for the case's input (in full when it is at most 32 KB, else its sha256) and the geometry. Needs Pillow; the
tests read the file and do not.

    python tests/golden/make_ingest_golden.py
"""
import hashlib
import os
import sys

import numpy as np
import PIL
import PIL.Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ingest_cases as IC  # noqa: E402

FULL_BYTES = 32 * 1024


def pillow_crop(u8, g):
    """Pillow's resize to the geometry's size with its filter, then its crop: the cropped uint8 array."""
    img = PIL.Image.fromarray(u8)
    img = img.resize(g["resized"], PIL.Image.LANCZOS if g["filter"] == IC.LANCZOS else PIL.Image.BICUBIC)
    return np.asarray(img.crop(g["crop"]))


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for c in IC.CASES + [IC.LEVELS]:
        src = IC.levels_image() if c == IC.LEVELS else IC.make_image(c[0], c[1])
        g = IC.geometry(*c)
        crop = pillow_crop(src, g)
        cid = IC.case_id(c)
        out[cid + "/shape"] = np.array(crop.shape, dtype=np.int32)
        out[cid + "/resized"] = np.array(g["resized"], dtype=np.int32)
        out[cid + "/crop"] = np.array(g["crop"], dtype=np.int32)
        out[cid + "/transformation"] = np.array(g["transformation"], dtype=np.float64)
        out[cid + "/sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(crop).tobytes()).hexdigest())
        if crop.nbytes <= FULL_BYTES:
            out[cid + "/rgb"] = crop
    path = os.path.join(HERE, "ingest.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
