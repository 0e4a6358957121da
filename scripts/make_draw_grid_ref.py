"""Record the mpmath reference of the draw grid (tests/draw_reference.py draw_grid_cells) as
tests/golden/draw_grid_ref.npy: the exact truncated-normal inverse at 50 digits, rounded to
double, for every (alpha, u) cell.  Takes a minute or two; tests/test_oracle_rng.py re-derives a
sample of the record on every run.

    python scripts/make_draw_grid_ref.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import draw_reference as D  # noqa: E402
from oracle.rng import trunc_normal_lower  # noqa: E402

if __name__ == "__main__":
    a, u = D.draw_grid_cells()
    ref = D.as_double(D.tn_reference(a, u, trunc_normal_lower(a, u)))
    assert np.isfinite(ref).all()
    np.save(D.GRID_REF, ref)
    print(D.GRID_REF, ref.shape)
