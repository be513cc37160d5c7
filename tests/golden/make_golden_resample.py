"""Writes g16_pillow_bicubic.npz: small 8-bit images and the bytes PIL's Image.resize(size, BICUBIC) returns for them
(Pillow 12.2.0 when this was recorded), so that tests/resample_reference.py is held against Pillow where Pillow is not
installed.  Needs Pillow; seeded.

  python tests/golden/make_golden_resample.py
"""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# (in_h, in_w, out_h, out_w, channels, kind)
CASES = [(16, 16, 8, 8, 3, "random"), (12, 18, 8, 12, 3, "random"), (33, 47, 22, 31, 1, "random"),
         (64, 40, 16, 10, 3, "binary"), (65, 65, 9, 9, 1, "binary"), (7, 5, 1, 1, 3, "random"),
         (30, 20, 30, 10, 3, "random"), (20, 30, 10, 30, 1, "binary"), (8, 8, 12, 12, 3, "random"),
         (1, 9, 1, 3, 1, "random"), (24, 24, 12, 12, 3, "edges"), (40, 24, 5, 3, 3, "binary")]


def make_input(g, h, w, c, kind):
    if kind == "random":
        img = g.integers(0, 256, (h, w, c), dtype=np.uint8)
    elif kind == "binary":
        img = (g.integers(0, 2, (h, w, c)) * 255).astype(np.uint8)
    else:   # hard vertical and horizontal edges
        img = np.zeros((h, w, c), np.uint8)
        img[:, w // 3:] = 255
        img[h // 2:, : w // 2] = 128
    return img[..., 0] if c == 1 else img


def main():
    g = np.random.default_rng(16)
    out = {"pillow_version": np.array(PIL.__version__)}
    for i, (ih, iw, oh, ow, c, kind) in enumerate(CASES):
        img = make_input(g, ih, iw, c, kind)
        out[f"in_{i}"] = img
        out[f"out_{i}"] = np.asarray(Image.fromarray(img).resize((ow, oh), Image.Resampling.BICUBIC))
        assert out[f"out_{i}"].shape[:2] == (oh, ow)
    path = os.path.join(HERE, "g16_pillow_bicubic.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(CASES), "cases")


if __name__ == "__main__":
    main()
