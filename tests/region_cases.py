"""The region sets that tests/test_region.py (no device) and tests/test_region_gpu.py share, and a plain-Python restatement of the
lowering rt_region_tiles does (include/rtamd.h)."""


def case_regions(W, H):
    """One call's worth of regions (x0, y0, x1, y1) of a W x H frame: the whole frame, the first pixel, the last pixel (in the partial
    corner tile when W or H is no multiple of 8), an unaligned 8 x 8 window, a one-pixel-wide column on a tile boundary over the full
    height, a one-pixel-high row, two overlapping windows, one window twice -- and then all of them once more in descending order of y0."""
    base = small_regions(W, H)
    base.insert(0, (0, 0, W, H))
    return base + sorted(base, key=lambda r: -r[1])


def small_regions(W, H):
    """case_regions without the whole frame (and without the repetition): a call that leaves tiles untouched"""
    return [(0, 0, 1, 1), (W - 1, H - 1, W, H), (5, 3, 13, 11), (8, 0, 9, H), (0, 7, W, 8),
            (10, 10, 30, 25), (20, 5, 41, 20), (33, 17, 50, 30), (33, 17, 50, 30)]


def python_tiles(W, H, regions):
    """the image tiles (ty * tiles_x + tx) any region touches, ascending and unique"""
    tiles_x = (W + 7) // 8
    touched = set()
    for (x0, y0, x1, y1) in regions:
        for y in range(y0, y1):
            for x in range(x0, x1):
                touched.add((y // 8) * tiles_x + x // 8)
    return sorted(touched)


def in_image_pixels(W, H, tiles):
    """pixels of the given image tiles that lie inside the W x H frame"""
    tiles_x = (W + 7) // 8
    return sum(min(8, W - (t % tiles_x) * 8) * min(8, H - (t // tiles_x) * 8) for t in tiles)
