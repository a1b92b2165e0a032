"""Record scikit-image's convex_hull_image on small masks -> tests/golden/slice_convex_hull_skimage_<version>.npz.

Run once where scikit-image is installed (the committed file came from 0.18.3); the test suite only reads the file.
shapes int16 [N, 2]; masks / hulls: np.packbits of the N flattened arrays, concatenated."""
import os

import numpy as np
import skimage
from skimage.morphology import convex_hull_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    rng = np.random.default_rng(20240607)
    out = []
    for k in range(184):
        ny, nx = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        density = (0.03, 0.1, 0.3, 0.7)[k % 4]
        m = rng.random((ny, nx)) < density
        if not m.any():
            m[rng.integers(0, ny), rng.integers(0, nx)] = True
        out.append(m)
    for slope_y, slope_x in ((1, 2), (3, 1), (1, 1), (2, 3)):          # isolated pixels on a line: centres exactly on edges
        m = np.zeros((13, 13), bool)
        for t in range(13):
            y, x = t * slope_y, t * slope_x
            if y < 13 and x < 13:
                m[y, x] = True
        out += [m, m[::-1].copy(), m.T.copy()]
    ring = np.zeros((11, 12), bool)
    ring[2:9, 2:10] = True
    ring[4:7, 4:8] = False
    c = np.zeros((9, 9), bool)
    c[1:8, 1:8] = True
    c[3:6, 3:8] = False
    two = np.zeros((13, 13), bool)
    two[0, 0] = two[12, 12] = True
    out += [ring, c, two, np.indices((8, 9)).sum(0) % 2 == 0]
    return out


def main():
    ms = cases()
    hulls = [convex_hull_image(m) for m in ms]
    shapes = np.array([m.shape for m in ms], dtype=np.int16)
    path = os.path.join(ROOT, "tests", "golden", f"slice_convex_hull_skimage_{skimage.__version__}.npz")
    np.savez_compressed(path, shapes=shapes, masks=np.packbits(np.concatenate([m.ravel() for m in ms])),
                        hulls=np.packbits(np.concatenate([h.ravel() for h in hulls])), skimage_version=np.array(skimage.__version__))
    print(path, len(ms), "masks", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
