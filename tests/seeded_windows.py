"""The seeded 8 x 8 windows that the full-spp window tests (test_golden.py, test_book2.py) compare with the oracle besides their fixed
ones."""
import numpy as np


def seeded_windows(W, H, seed):
    """8 x 8 windows (x0, y0) that the full-spp window tests add to their fixed ones: the four frame corners (last column, last row),
    one window straddling the corner of four 8 x 8 tiles (x0 = y0 = 4 mod 8) and three positions aligned to no tile, from
    np.random.default_rng(seed)"""
    rng = np.random.default_rng(seed)
    out = [(0, 0), (W - 8, 0), (0, H - 8), (W - 8, H - 8)]
    out.append((int(rng.integers(0, (W - 12) // 8 + 1)) * 8 + 4, int(rng.integers(0, (H - 12) // 8 + 1)) * 8 + 4))
    while len(out) < 8:
        x0, y0 = int(rng.integers(0, W - 7)), int(rng.integers(0, H - 7))
        if x0 % 8 and y0 % 8:
            out.append((x0, y0))
    return out
