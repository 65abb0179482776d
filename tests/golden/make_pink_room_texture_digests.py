#!/usr/bin/env python3
"""Writes tests/golden/pink_room_texture_digests.json: for every texture file the reference ships for its one scene
(CommonPasses/Data/pink_room/textures/*: 26 PNG + 2 JPEG; the WoodFloor base-colour pair is among the blobs missing from
the checkout), its size, format, whether it carries alpha, and the SHA-256 of its texels as decoded by Pillow
(libpng / libjpeg-turbo) — an independent decoder.  tests/test_image_decode.py writes a stand-in of each file's size,
format and alpha verdict.  Data in, digests out: no reference source is read.
Usage: python tests/golden/make_pink_room_texture_digests.py <pink_room/textures directory of a reference checkout>"""
import glob
import hashlib
import json
import os
import sys

import numpy as np
from PIL import Image

SRC = sys.argv[1]
out = {}
for f in sorted(glob.glob(os.path.join(SRC, "*"))):
    im = Image.open(f)
    has_alpha = im.mode in ("RGBA", "LA") or "transparency" in im.info
    px = np.asarray(im.convert("RGBA"))
    texels = px if has_alpha else px[..., :3]
    out[os.path.basename(f)] = {"width": im.size[0], "height": im.size[1], "format": im.format, "alpha": bool(has_alpha),
                                "sha256": hashlib.sha256(np.ascontiguousarray(texels).tobytes()).hexdigest()}
json.dump(out, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "pink_room_texture_digests.json"), "w"), indent=1, sort_keys=True)
print(len(out), "files")
