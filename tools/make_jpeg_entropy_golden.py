"""Writes tests/golden/jpeg_entropy.npz with Pillow: JPEG byte strings for the device entropy decode (include/ivit_jpeg_entropy.h),
beside the files of tests/golden/jpeg.npz.  Chosen for what the small files there do not reach:

  noise_q100_s0      160 x 120 noise at quality 100, 4:4:4: a block spans several subsequences, and the file has more
                     subsequences than the workgroup has lanes at the smallest subsequence
  grad_q30_s2        256 x 192 gradient at quality 30, 4:2:0: flat blocks of a few bits, many blocks in one subsequence, slow
                     synchronisation
  *_rst1, *_rstrow   the same two with a restart marker behind every MCU and behind every MCU row
  grey_q85           160 x 120 noise, one component

    python tools/make_jpeg_entropy_golden.py            # needs Pillow; rewrites the file

Keys: `names`, `jpg_<name>` uint8.  Byte strings only: the expected coefficients are the host decoder's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_jpeg_golden import ROOT, encode, picture  # noqa: E402


def main():
    noise, grad = picture("noise", 160, 120, 2000), picture("grad", 256, 192, 0)
    out = {}
    for tag, kw in (("", {}), ("_rst1", {"restart_marker_blocks": 1}), ("_rstrow", {"restart_marker_rows": 1})):
        out["noise_q100_s0" + tag] = encode(noise, quality=100, subsampling=0, **kw)
        out["grad_q30_s2" + tag] = encode(grad, quality=30, subsampling=2, **kw)
    out["grey_q85"] = encode(noise, "L", quality=85)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_entropy.npz")
    np.savez_compressed(path, names=np.array(sorted(out)), **{"jpg_" + k: np.frombuffer(v, np.uint8) for k, v in out.items()})
    print("%s: %d files, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    sys.exit(main())
