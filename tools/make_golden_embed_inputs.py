#!/usr/bin/env python3
"""Writes tests/golden/g23_reid_crops.npz: frames, boxes and what ``numpy.pad(mode='mean')`` followed by
``PIL.Image.fromarray(...).resize((ow, oh), Image.BILINEAR)`` returns for them -- the two library calls of the reference's
``BoundingBoxDataset.__getitem__`` (utils/rgb.py:51-62) before ``ToTensor``.  Needs Pillow; nothing that runs on the GPU does.

Groups (``<group>_boxes`` float64 [n, 4] = left, top, right, bottom; ``<group>_frame`` int64 [n]; ``<group>_crops`` uint8
[n, oh, ow, 3]) over ``small_frames`` (two of 37 x 53: noise, and a 0 / 255 checkerboard with a smooth ramp band) and
``big_frames`` (one of 300 x 200): ``small_128x64``, ``small_16x8``, ``small_5x3``, ``big_128x64``."""
import os

import numpy as np
import PIL
from PIL import Image

H, W = 37, 53
BH, BW = 300, 200

# (name, frame, box): every box goes to (16, 8) and (5, 3); those of TO_128 also to (128, 64)
SMALL = [
    ("inside 9 x 5, upscaled", 0, (20, 10, 25, 19)),
    ("whole frame", 1, (0, 0, 53, 37)),
    ("width 8 = ow", 0, (10, 3, 18, 30)),
    ("height 16 = oh", 1, (5, 8, 40, 24)),
    ("width 3 = ow", 1, (7, 2, 10, 30)),
    ("height 5 = oh", 0, (4, 20, 44, 25)),
    ("1 x 1", 0, (30, 20, 31, 21)),
    ("fractional corners", 1, (12.7, 3.2, 30.4, 20.9)),
    ("over the left edge", 0, (-6.5, 5, 20, 30)),
    ("over the top edge", 1, (10, -4.2, 40, 20)),
    ("over the right edge", 0, (35, 6, 60.3, 31)),
    ("over the bottom edge", 1, (8, 15, 33, 45.8)),
    ("over all four edges", 1, (-5, -7, 58, 44)),
    ("pad larger than the crop", 0, (-30, 10, 8, 25)),
    ("top = -0.5: no pad", 1, (10, -0.5, 30, 20)),
    ("bottom = H + 0.6: no pad", 0, (10, 5, 30, 37.6)),
    ("padded width 64 = ow", 1, (-11, 5, 53, 30)),
    ("padded height 128 = oh", 0, (10, -50, 30, 78)),
]
TO_128 = ("inside 9 x 5, upscaled", "1 x 1", "fractional corners", "over all four edges", "padded width 64 = ow", "padded height 128 = oh")
BIG = [
    ("290 x 190", 0, (5, 5, 195, 295)),
    ("over the left and bottom edges", 0, (-9.5, 40, 150, 306.2)),
]


def small_frames():
    rng = np.random.default_rng(23)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    board = np.where((y + x) % 2 == 0, 255, 0).astype(np.uint8)[:, :, None].repeat(3, axis=2)
    band = (slice(14, 24), slice(None))
    board[band] = np.stack([(x[band] * 255) // (W - 1), (y[band] - 14) * 25, 255 - (x[band] * 255) // (W - 1)], axis=-1).astype(np.uint8)
    return np.stack([noise, board])


def big_frames():
    rng = np.random.default_rng(24)
    y, x = np.mgrid[0:BH, 0:BW]
    base = np.stack([(x * 255) // (BW - 1), (y * 255) // (BH - 1), ((x // 8 + y // 8) % 2) * 200], axis=-1)
    return np.clip(base + rng.integers(0, 16, (BH, BW, 3)), 0, 255).astype(np.uint8)[None]


def library_crop(frame, box, oh, ow):
    left, top, right, bot = box
    h, w = frame.shape[:2]
    img = frame[int(max(0, top)):int(max(0, bot)), int(max(0, left)):int(max(0, right))]
    pads = ((int(abs(top - max(top, 0))), int(abs(bot - min(bot, h)))), (int(abs(left - max(left, 0))), int(abs(right - min(right, w)))), (0, 0))
    img = np.pad(img, pads, mode="mean")
    return np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))


def main():
    out = {"small_frames": small_frames(), "big_frames": big_frames(), "pillow_version": np.array(PIL.__version__),
           "numpy_version": np.array(np.__version__), "small_names": np.array([c[0] for c in SMALL]),
           "big_names": np.array([c[0] for c in BIG])}
    groups = [("small_128x64", "small_frames", [c for c in SMALL if c[0] in TO_128], (128, 64)), ("small_16x8", "small_frames", SMALL, (16, 8)),
              ("small_5x3", "small_frames", SMALL, (5, 3)), ("big_128x64", "big_frames", BIG, (128, 64))]
    for name, frames, cases, (oh, ow) in groups:
        out[name + "_boxes"] = np.asarray([c[2] for c in cases], np.float64)
        out[name + "_frame"] = np.asarray([c[1] for c in cases], np.int64)
        out[name + "_crops"] = np.stack([library_crop(out[frames][c[1]], c[2], oh, ow) for c in cases])
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g23_reid_crops.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__, "numpy", np.__version__)


if __name__ == "__main__":
    main()
