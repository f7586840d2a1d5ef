"""Seeded test images for lld_orb_extract and its restatement (tests/orb_extract_ref.py), shared by the GPU tests and
tools/fuzz_orb_extract.py."""
import numpy as np

KINDS = ("textured", "flat", "busy", "constant", "corner", "checker")


def scene(kind, cols, rows, seed):
    """'textured' (polygons on a smooth texture plus noise), 'flat' (a constant image with a few faint shapes), 'busy' (strong pixel
    noise: tens of thousands of level-0 candidates), 'constant' (one grey value: no FAST candidate at any level), 'corner' (one
    bright spot on a constant background: exactly one FAST corner at level 0), 'checker' (5-px squares of two values: runs of
    equal FAST scores and octree nodes of equal size)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    if kind == "busy":
        img = rng.integers(0, 256, (rows, cols)).astype(np.float64)
    elif kind == "flat":
        img = np.full((rows, cols), 118.0)
        for _ in range(3):
            cx, cy, r = rng.uniform(min(60, cols / 2), max(cols - 60, cols / 2)), rng.uniform(min(40, rows / 2), max(rows - 40, rows / 2)), rng.uniform(8, 25)
            img[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] += rng.uniform(10, 30)
        img += rng.integers(0, 2, (rows, cols))
    elif kind == "constant":
        img = np.full((rows, cols), float(rng.integers(0, 256)))
    elif kind == "corner":
        cx, cy = int(rng.uniform(0.3, 0.7) * cols), int(rng.uniform(0.3, 0.7) * rows)
        img = np.full((rows, cols), 60.0)
        img[cy - 1:cy + 2, cx - 1:cx + 2] = 150.0          # a 3x3 spot brightest at its centre: its circle is all background, so
        img[cy, cx] = 220.0                                # (cx, cy) is the one FAST corner of level 0 and beats its 8 neighbours
    elif kind == "checker":
        off = int(rng.integers(0, 5))
        img = np.where((((xx + off) // 5) + ((yy + off) // 5)) % 2 == 0, 60.0, 190.0)
    else:
        img = 90 + 40 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
        for _ in range(60):
            cx, cy = rng.uniform(0, cols), rng.uniform(0, rows)
            w, h = rng.uniform(5, 60, 2)
            a = rng.uniform(0, np.pi)
            u = (xx - cx) * np.cos(a) + (yy - cy) * np.sin(a); v = -(xx - cx) * np.sin(a) + (yy - cy) * np.cos(a)
            img[(np.abs(u) < w) & (np.abs(v) < h)] = rng.uniform(0, 255)
        img += rng.normal(0, 4, (rows, cols))
    return np.clip(np.round(img), 0, 255).astype(np.uint8)
