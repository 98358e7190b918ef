"""What the two ``TargetModel`` tests share (TEST INFRASTRUCTURE): the 8 x 33 sensor, its models and its one cloud.  The
restatements are tests/beam_az_cases.py's; nothing here imports ``lidar_transfer_amd``."""
from __future__ import annotations

import numpy as np

import beam_az_cases as ac

#: eight unevenly spaced beams inside (FOV_UP, FOV_DOWN); W is odd and no multiple of anything
TABLE = np.array([10.0, 6.0, 3.0, 1.0, -1.0, -4.0, -9.0, -15.0], np.float64)
FOV = (12.0, -18.0)
H, W = len(TABLE), 33
#: name -> (beam_table, sector, beam_azimuth): the keywords of ``Projector.project`` / ``DeviceDeform(t_...)``
MODELS = {
    "A": (TABLE, None, ac.offsets("mixed", H)),                    # a table and offsets
    "B": (TABLE, ac.SEAM_SECTOR, ac.offsets("ninety", H)),         # the same table, other offsets, a sector
    "plain": (None, None, None),
    "sector": (None, ac.SEAM_SECTOR, None),                        # (the reverse projection's second branch)
    "table": (TABLE, None, None),                                  # (and its third)
}
#: the order in which ONE projector sees them
SEQUENCE = ("A", "B", "plain", "A")
N_POINTS, SEED = 2000, 4


def cloud():
    """float64 (the ``cp`` path's dtype), full circle: tests/beam_cases.py's seeded cloud with tests/beam_az_cases.py's chosen
    point whose own offset carries it across the seam"""
    return ac.seeded_cloud(TABLE, FOV, MODELS["A"][2], N_POINTS, np.float64, SEED)[:3]
