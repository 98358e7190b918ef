#!/usr/bin/env python3
"""Generate golden fixture F16 -- the reference's own `do_range_projection_new` + `do_label_projection_new` on 40 random
float64 clouds and its `MultiSemLaserScan.create_rays` for 30 random sensor models (auxiliary/laserscan.py:1092-1119), the
random inputs of tests/pin_cases.py (projection_fuzz_cases, create_rays_fuzz_cases: regenerated from their seeds, not stored).

    python tests/golden/make_golden_live_fuzz.py        # needs the reference checkout (LT_REFERENCE)

`f16_live_fuzz.npz`: `proj_sha256` [40, 6, 32] -- per cloud the digests (pin_cases.projection_fuzz_digests) of the range,
index, remission, proj_x / proj_y and label images; `proj_filled` [40] -- the filled pixels per cloud; `rays_sha256`
[30, 32] -- the digest of each `create_rays` array (shape, dtype, bytes).  tests/test_oracle_cpu.py runs oracle/projection.py
and lidar_transfer_amd.laserscan.create_rays on the same inputs and compares the digests.  Only data is written."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden  # noqa: E402
import pin_cases as pc  # noqa: E402


def main():
    ls, _ = make_golden.import_reference()
    proj, filled = [], []
    for H, W, fu, fd, pts, rem, lab, remove, beams in pc.projection_fuzz_cases():
        s = ls.SemLaserScan(H, W, 300, pc.PROJ_FUZZ_COLOR_DICT, None, beams)
        s.points, s.remissions, s.label = pts.copy(), rem.copy(), lab.copy()
        s.colorize()
        s.do_range_projection_new(fu, fd, remove=remove)
        s.do_label_projection_new()
        proj.append(pc.projection_fuzz_digests(np.asarray(s.range_image), np.asarray(s.index), np.asarray(s.proj_remissions),
                                               np.asarray(s.proj_x), np.asarray(s.proj_y), np.asarray(s.label_image)[..., 0]))
        filled.append(int((np.asarray(s.index) >= 0).sum()))
    rays = [pc.array_digest(ls.MultiSemLaserScan.create_rays(None, fu, fd, H, W))
            for fu, fd, H, W in pc.create_rays_fuzz_cases()]
    out = os.path.join(HERE, "f16_live_fuzz.npz")
    np.savez_compressed(out, proj_sha256=np.stack(proj), proj_filled=np.array(filled, np.int64), rays_sha256=np.stack(rays))
    print(f"{out}: {len(proj)} clouds ({sum(filled)} filled pixels), {len(rays)} sensor models")


if __name__ == "__main__":
    main()
