"""Generates tests/golden/reference_files.npz: the bytes of the reference's own asset files that the CPU tests read as files,
so that the suite needs nothing outside this repository:

  prototype/data/models/CornellBox-Original.gltf   (16 kB, buffers embedded as base64)
  prototype/data/models/sphere.gltf                (141 kB, embedded)
  utopian/data/textures/defaults/white_texture.png
  prototype/data/models/Sponza/glTF/<name>.jpg     the four smallest of Sponza's 65 JPEG textures (0.45 MB; all 65 are 38 MB)

Each file is one uint8 array keyed by its file name. The files are data: nothing here is the reference's code.

  python tests/golden/make_reference_file_fixtures.py <reference checkout>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SPONZA = "prototype/data/models/Sponza/glTF"
SPONZA_SAMPLE = 4


def main(ref):
    files = ["prototype/data/models/CornellBox-Original.gltf", "prototype/data/models/sphere.gltf", "utopian/data/textures/defaults/white_texture.png"]
    names = [str(n) for n in np.load(os.path.join(HERE, "jpeg_fixtures.npz"))["sponza_names"]]  # the 65 textures recorded there
    files += sorted((os.path.join(SPONZA, n) for n in names), key=lambda p: os.path.getsize(os.path.join(ref, p)))[:SPONZA_SAMPLE]
    out = {os.path.basename(p): np.frombuffer(open(os.path.join(ref, p), "rb").read(), dtype=np.uint8) for p in files}
    dst = os.path.join(HERE, "reference_files.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
