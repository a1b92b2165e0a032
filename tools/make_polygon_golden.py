"""Record scikit-image's skimage.draw.polygon on the polygons of tests/test_contours.py ->
tests/golden/polygon_skimage_<version>.npz.

Run once where scikit-image is installed; nothing in the test suite reads such a file yet (none is committed: parity of
pa.dicom with scikit-image is unpinned).  The polygons are the degenerate ones and the seeded random ones of the test file.
x is passed as `r` and y as `c`, as dicom/io/rtstruct_to_nifti.py:204-207 does, but with shape = (nx, ny), the true extent of
that orientation, so the recorded masks are clipped to the slice and not by the reference's transposed shape.
shapes int16 [N, 2] (ny, nx); counts int16 [N] vertices per polygon; vertices int32 [sum, 2] (x, y); masks: np.packbits of the
N flattened [ny, nx] arrays, concatenated."""
import os
import sys

import numpy as np
import skimage
from skimage.draw import polygon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_contours import DEGENERATE, SLICES, random_polygons  # noqa: E402


def cases():
    out = [((13, 13), pts) for pts in DEGENERATE.values()] + [((7, 19), pts) for pts in DEGENERATE.values()]
    for ny, nx in SLICES:
        out += [((ny, nx), pts) for _, _, pts in random_polygons(ny, nx, 1, 60, seed=1000 * ny + nx + 1)]
    return out


def main():
    cs = cases()
    masks = []
    for (ny, nx), pts in cs:
        xs, ys = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
        fx, fy = polygon(xs, ys, shape=(nx, ny))
        m = np.zeros((ny, nx), dtype=bool)
        m[fy, fx] = True
        masks.append(m)
    path = os.path.join(ROOT, "tests", "golden", f"polygon_skimage_{skimage.__version__}.npz")
    np.savez_compressed(path, shapes=np.array([c[0] for c in cs], dtype=np.int16), counts=np.array([len(c[1]) for c in cs], dtype=np.int16),
                        vertices=np.array([p for c in cs for p in c[1]], dtype=np.int32), masks=np.packbits(np.concatenate([m.ravel() for m in masks])),
                        skimage_version=np.array(skimage.__version__))
    print(path, len(cs), "polygons", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
