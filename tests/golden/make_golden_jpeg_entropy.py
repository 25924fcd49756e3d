#!/usr/bin/env python3
"""Generates tests/golden/jpeg_entropy_cases.npz: JPEG streams large enough to span several workgroups of the device
entropy decoder (restart intervals, custom tables, ragged MCUs, long codes) and the pixels Pillow's libjpeg-turbo decodes
from them, after make_golden_codec.py:
    python tests/golden/make_golden_jpeg_entropy.py
The fixture holds data only (compressed bytes in, decoded bytes out).  It has to stay below 256 KB and the pictures are noisy, so
only a case whose pixels fit carries them (<name>_rgb); the 320-wide cases carry the SHA-256 of Pillow's pixel bytes instead
(<name>_rgb_sha256, with <name>_shape), which holds a decoder to the same bytes, and a CRC-32 per pixel row
(<name>_rgb_rowcrc), which says where a decoder differs."""
import hashlib
import io
import zlib
import os

import numpy as np
from PIL import Image, features

from make_golden_codec import picture

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [("c420_q90_320", 240, 320, 3, dict(quality=90, subsampling=2)),                                  # ~35 KB: more than one workgroup at the default size
         ("c444_q100_96", 96, 96, 3, dict(quality=100, subsampling=0)),                                    # long codes, dense blocks
         ("grey_rst7_320", 240, 320, 1, dict(quality=90, restart_marker_blocks=7)),                        # restart intervals, grey
         ("c422_opt_323", 241, 323, 3, dict(quality=92, subsampling=1, optimize=True)),                    # custom tables, ragged MCUs
         ("c420_rstrow_320", 240, 320, 3, dict(quality=85, subsampling=2, restart_marker_rows=1))]         # restart intervals, three components


def main():
    assert features.check("libjpeg_turbo"), "Pillow without libjpeg-turbo"
    rng = np.random.default_rng(20261018)
    out = {"names": np.array([c[0] for c in CASES]), "libjpeg_turbo": np.frombuffer(features.version("jpg").encode(), np.uint8)}
    for name, h, w, c, kw in CASES:
        img = picture(rng, h, w, c)
        b = io.BytesIO()
        Image.fromarray(img[..., 0] if c == 1 else img).save(b, "JPEG", **kw)
        data = b.getvalue()
        out[name + "_jpeg"] = np.frombuffer(data, np.uint8)
        dec = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data))))   # RGB order (cv::imdecode returns the same bytes as BGR)
        if dec.nbytes <= 32768:
            out[name + "_rgb"] = dec
        else:
            out[name + "_rgb_sha256"] = np.frombuffer(hashlib.sha256(dec.tobytes()).digest(), np.uint8)
            out[name + "_shape"] = np.array(dec.shape, np.int32)
            out[name + "_rgb_rowcrc"] = np.array([zlib.crc32(row.tobytes()) for row in dec], np.uint32)      # locates a failure: one CRC-32 per pixel row
        print(name, len(data), "bytes")
    path = os.path.join(HERE, "jpeg_entropy_cases.npz")
    np.savez(path, **out)
    print("wrote jpeg_entropy_cases.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
