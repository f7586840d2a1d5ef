"""Crafted scenes for Frame::ComputeStereoMatches (src/Frame.cc:530-704): named, deterministic, small, each aimed at exits of the
routine that a generated stereo pair never reaches.  numpy and scipy only; `frames()` alone touches the library, for its Frame
record.  tests/test_oracle_stereo_exits.py proves from the oracle's exit census that every scene does what it says here, and
tests/test_gpu_stereo_exits.py runs both device routes on them.

How a scene is made.  The routine never relates two pyramid levels, so every level is its own texture, and the right level is the
left one moved by `shift` whole pixels (R(x) = L(x + shift)) plus, where wanted, a little noise, so that SAD distances are not
all zero (a median of 0 clears every match).  A pair is a left keypoint on the level pixel (x0, y0) and a right keypoint on the
level pixel (xr, y0 + dy): the SAD search then has its minimum at incR = x0 - shift - xr.  Descriptors are random per pair, the
right one a copy with `flips` bits flipped, so a wrong candidate (distance around 128) never wins the Hamming stage.

Exit codes (the oracle's census): 1 row outside the image, 2 empty row, 3 maxU < 0, 4 no candidate passed the octave and u gates,
5 bestDist >= thOrbDist, 6 iniu < 0 || endu >= cols, 7 patch leaves the image, 8 bestincR == +-L, 9 disparity outside [minD, maxD),
10 matched with disparity == 0, 11 matched and kept, 12 matched and removed by the median cut."""
import numpy as np
from scipy import ndimage

f32 = np.float32


def orb_levels(scale_factor, n_levels):
    """mvScaleFactor / mvInvScaleFactor as ORBextractor builds them: cumulative float products, inverse by one division."""
    scale = np.ones(n_levels, f32)
    for i in range(1, n_levels):
        scale[i] = f32(scale[i - 1] * f32(scale_factor))
    return scale, (f32(1.0) / scale).astype(f32)


def flip_bits(desc, k, first=0):
    """`desc` [8] uint32 with the k bits first .. first+k-1 flipped: Hamming distance exactly k."""
    d = np.array(desc, np.uint32, copy=True)
    for b in range(first, first + k):
        d[(b >> 5) & 7] ^= np.uint32(1) << np.uint32(b & 31)
    return d


class Builder:
    def __init__(self, name, exits, width, height, n_levels, scale_factor=1.2, seed=0, shift=4, noise=3, mb=0.5, mbf=32.0, texture="smooth"):
        self.name, self.exits, self.width, self.height, self.shift = name, tuple(exits), width, height, shift
        self.mb, self.mbf = float(f32(mb)), float(f32(mbf))
        self.rng = np.random.default_rng([0x57E2E0, seed])
        self.scale, self.inv_scale = orb_levels(scale_factor, n_levels)
        self.cols = [int(np.round(width * float(s))) for s in self.inv_scale]
        self.rows = [int(np.round(height * float(s))) for s in self.inv_scale]
        self.left = [self._texture(texture, r, c) for r, c in zip(self.rows, self.cols)]
        self.right = []
        for im in self.left:
            r = np.roll(im, -shift, axis=1).astype(np.int32)
            if noise:
                r = r + self.rng.integers(-noise, noise + 1, r.shape)
            self.right.append(np.clip(r, 0, 255).astype(np.uint8))
        self.l_xy, self.l_oct, self.l_desc, self.r_xy, self.r_oct, self.r_desc = [], [], [], [], [], []
        self.tags, self.pairs = {}, []

    def _texture(self, kind, rows, cols):
        if kind == "smooth":                                       # values 40 .. 200: room for perturbations without clipping
            g = ndimage.gaussian_filter(self.rng.normal(size=(rows, cols)), 1.0)
            return np.round(40.0 + 160.0 * (g - g.min()) / (g.max() - g.min())).astype(np.uint8)
        if kind == "mirror":                                       # T(y, x) = g[y, distance of x to the nearest multiple of 12]:
            g = self.rng.integers(40, 201, (rows, 13))             # symmetric about every column that is a multiple of 12
            x = np.arange(cols) % 24
            return g[:, np.minimum(x, 24 - x)].astype(np.uint8)
        raise ValueError(kind)

    def left_kp(self, u, v, octave, desc=None, tag=None):
        self.l_xy.append((f32(u), f32(v))); self.l_oct.append(octave)
        self.l_desc.append(self.rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32) if desc is None else desc)
        if tag is not None:
            self.tags.setdefault(tag, []).append(len(self.l_oct) - 1)
        return len(self.l_oct) - 1

    def right_kp(self, u, v, octave, desc):
        self.r_xy.append((f32(u), f32(v))); self.r_oct.append(octave); self.r_desc.append(desc)
        return len(self.r_oct) - 1

    def pair(self, level, x0, v, xr=None, dy=0.0, r_level=None, flips=4, tag=None, ul=None, ur=None):
        """Left keypoint on level pixel column x0 at image row v, right keypoint on level column xr (default: where the texture went),
        its octave r_level (default: the same).  ul / ur override the image columns themselves."""
        s = self.scale[level]
        xr = x0 - self.shift if xr is None else xr
        uL = f32(x0) * s if ul is None else f32(ul)
        uR = f32(xr) * s if ur is None else f32(ur)
        iL = self.left_kp(uL, v, level, tag=tag)
        self.right_kp(uR, f32(v) + f32(dy), level if r_level is None else r_level, flip_bits(self.l_desc[iL], flips))
        return iL

    def fill(self, n, levels=None, rows=None, tag="fill", spoil_every=0):
        """n pairs that match: random places at least 5 px (and the search window) inside their level; `rows`: image rows to use."""
        levels = list(range(len(self.scale))) if levels is None else levels
        for i in range(n):
            l = levels[i % len(levels)]
            x0 = int(self.rng.integers(self.shift + 10, self.cols[l] - 11))
            if rows is None:
                v = f32(int(self.rng.integers(5, self.rows[l] - 5))) * self.scale[l]
            else:
                v = f32(rows[i % len(rows)])
            self.pair(l, x0, v, dy=float(self.rng.uniform(-0.8, 0.8)), r_level=int(np.clip(l + self.rng.integers(-1, 2), 0, len(self.scale) - 1)), tag=tag)
            if spoil_every and i % spoil_every == spoil_every - 1:
                self.spoil(l, x0, v, 12)

    def spoil(self, level, x0, v, amp):
        """Noise of +-amp on the right level where the pair's patch lands: a SAD distance several times the usual one."""
        y0 = int(np.round(float(f32(v) * self.inv_scale[level]))); xr = x0 - self.shift
        R = self.right[level]
        ys, xs = slice(max(y0 - 5, 0), y0 + 6), slice(max(xr - 5, 0), xr + 6)
        R[ys, xs] = np.clip(R[ys, xs].astype(np.int32) + self.rng.integers(-amp, amp + 1, R[ys, xs].shape), 0, 255).astype(np.uint8)

    def bump(self, level, x0, y0, amount):
        """One pixel of the pair's best right patch (not its centre) raised by `amount`: with a noise-free right level the pair's SAD is `amount`."""
        R = self.right[level]
        assert int(R[y0 - 3, x0 - self.shift - 3]) + amount <= 255
        R[y0 - 3, x0 - self.shift - 3] += np.uint8(amount)

    def scene(self, n_left=None):
        A = lambda a, t, shape: np.ascontiguousarray(np.array(a, t).reshape(shape))
        sc = dict(name=self.name, exits=self.exits, width=self.width, height=self.height, scale=self.scale, inv_scale=self.inv_scale,
                  left=self.left, right=self.right, mb=self.mb, mbf=self.mbf, tags=self.tags, pairs=self.pairs,
                  l_xy=A(self.l_xy, f32, (-1, 2)), l_oct=A(self.l_oct, np.int32, (-1,)), l_desc=A(self.l_desc, np.uint32, (-1, 8)),
                  r_xy=A(self.r_xy, f32, (-1, 2)), r_oct=A(self.r_oct, np.int32, (-1,)), r_desc=A(self.r_desc, np.uint32, (-1, 8)))
        if n_left is not None:
            for k in ("l_xy", "l_oct", "l_desc"):
                sc[k] = np.ascontiguousarray(sc[k][:n_left])
        return sc


# ---------------------------------------------------------------------------------------------------------------- the scenes
def tall():
    """160 x 720, 8 levels: taller than the 512 row buckets of the host route's stage 1.  Left rows 0 .. 719, every row 500 .. 525;
    right keypoints of every octave below row 512, some with their 2 * scale band across rows 511 / 512."""
    b = Builder("tall", (11,), 160, 720, 8, seed=1)
    b.fill(91, rows=np.r_[np.arange(0, 720, 8), 719])
    b.fill(104, rows=np.repeat(np.arange(500, 526), 4))
    for o in range(8):                                             # the right keypoint just below row 512, the left one above it, inside the band
        for k, x0 in enumerate((16, 22, 28)):
            b.pair(o, x0, f32(511.5 - k), dy=float(f32(512.25) - f32(511.5 - k)), tag="across")
    return b.scene()


def levels_1():
    """One level: a row table of one octave, the level gate [-1, 1] clamped to it."""
    b = Builder("levels_1", (11,), 200, 120, 1, seed=2)
    b.fill(60)
    return b.scene()


def levels_3():
    """Three levels, right keypoints of the top octave: the +-1 gate at the table's end (left octave 1 and 2 pass, 0 does not)."""
    b = Builder("levels_3", (4, 11), 200, 120, 3, seed=3)
    b.fill(45)
    for l in (0, 1, 2):
        for i in range(8):
            x0 = 30 + 14 * i
            b.pair(l, x0, f32(10 + 4 * l + 9 * i), r_level=2, tag="top_%d" % l)
    return b.scene()


def levels_16():
    """Sixteen levels at scale 1.1, 200 x 540: 511 buckets per octave, so rows from 511 on share one bucket."""
    b = Builder("levels_16", (11,), 200, 540, 16, scale_factor=1.1, seed=4)
    b.fill(96, rows=np.arange(6, 540, 11))
    b.fill(160, rows=np.repeat(np.arange(500, 540), 4))
    return b.scene()


def patch_limits():
    """200 x 120, 4 levels, shift 7.  At every level one pair a pixel inside and one a pixel outside each limit of the refinement:
    xr - 10 >= 0, endu = xr + 11 < cols, x0 + 5 < cols, y0 - 5 >= 0, y0 + 5 < rows.  `pairs` lists (what, level, inside, outside).
    x0 - 5 >= 0 cannot be met on its own: stage 1 admits only uR <= uL, rounding keeps the order, so xr <= x0 and xr - 10 < 0 leaves first;
    the x0 = 4 and x0 = 5 keypoints are there (tag `x0_low`) and both leave at exit 7.  Level 0 also holds keypoints on x.5 and y.5, where
    round-half-away and round-half-even part, two of them on a limit (v = 4.5 -> y0 = 5 inside; uL = cols - 5.5 -> x0 = cols - 5 outside)."""
    b = Builder("patch_limits", (6, 7, 11), 200, 120, 4, seed=5, shift=7)
    for l in range(4):
        C, Rw, s = b.cols[l], b.rows[l], b.scale[l]
        y = lambda k: f32(8 + 7 * k) * s                           # a row of its own for every keypoint of the level
        b.pairs.append(("xr", l, b.pair(l, 17, y(0), tag="in"), b.pair(l, 16, y(1), tag="out")))
        b.pairs.append(("endu", l, b.pair(l, C - 8, y(2), xr=C - 12, tag="in"), b.pair(l, C - 8, y(3), xr=C - 11, tag="out")))
        b.pairs.append(("x0_high", l, b.pair(l, C - 6, y(4), tag="in"), b.pair(l, C - 5, y(5), tag="out")))
        b.pairs.append(("y0_low", l, b.pair(l, 40, f32(5) * s, tag="in"), b.pair(l, 60, f32(4) * s, tag="out")))
        b.pairs.append(("y0_high", l, b.pair(l, 40, f32(Rw - 6) * s, tag="in"), b.pair(l, 60, f32(Rw - 5) * s, tag="out")))
        b.pair(l, 5, y(6), xr=5, tag="x0_low"); b.pair(l, 4, y(7), xr=4, tag="x0_low")
    for k, (ul, v, ur) in enumerate(((60.5, 30.0, 52.5), (62.5, 40.5, 56.0), (80.0, 50.5, 72.5), (100.5, 60.5, 92.5), (120.5, 70.0, 114.0))):
        b.pair(0, 0, f32(v), ul=ul, ur=ur, tag="half")
    b.pair(0, 0, f32(4.5), ul=90.0, ur=83.0, tag="half")
    b.pair(0, 0, f32(90.0), ul=b.cols[0] - 5.5, ur=b.cols[0] - 13.0, tag="half")
    b.fill(24)
    return b.scene()


def shifts():
    """The right keypoint e = -6 .. 6 columns off the column the texture moved to: bestincR = -e takes every value, +-5 included
    (exit 8; at |e| = 6 the minimum lies outside the window).  Pairs at Hamming distance 74 and 75 around thOrbDist, and some
    spoiled right patches for the median cut."""
    b = Builder("shifts", (5, 8, 11, 12), 240, 140, 3, seed=6, shift=8)
    k = 0
    for l in range(3):
        for e in range(-6, 7):
            for rep in range(2):
                x0 = 30 + (k * 37) % (b.cols[l] - 60); v = f32(6 + (k * 5) % (b.rows[l] - 12)) * b.scale[l]; k += 1
                b.pair(l, x0, v, xr=x0 - 8 + e, tag="e%+d" % e)
    for i in range(6):
        b.pair(0, 40 + 25 * i, f32(20 + 15 * i), flips=74, tag="d74")
        b.pair(0, 50 + 25 * i, f32(25 + 15 * i), flips=75, tag="d75")
    b.fill(40, spoil_every=5, tag="fill")
    return b.scene()


def zero_disparity():
    """Both images equal.  The top of level 0 and 1 is column-symmetric about every 12th column, so a pair on such a column has
    dist1 == dist3 and a disparity of exactly 0 (exit 10: u_right = uL - 0.01, depth = mbf / 0.01f).  Below, noise on the right
    level makes the parabola lean either way: slightly negative disparities (exit 9) and slightly positive ones, whose SAD
    distances keep the median above 0."""
    b = Builder("zero_disparity", (9, 10, 11), 200, 120, 2, seed=7, shift=0, noise=0, texture="mirror")
    for l in (0, 1):
        half = b.rows[l] // 3
        low = Builder("_", (), b.cols[l], b.rows[l] - half, 1, seed=70 + l, shift=0, noise=4)
        b.left[l][half:] = low.left[0]; b.right[l][half:] = low.right[0]
        for i in range(10):
            x0 = 24 + 12 * i
            b.pair(l, x0, f32(6 + (i * 3) % (half - 12)) * b.scale[l], tag="zero")
        for i in range(50):
            x0 = int(b.rng.integers(12, b.cols[l] - 12))
            b.pair(l, x0, f32(int(b.rng.integers(half + 6, b.rows[l] - 6))) * b.scale[l], tag="lean")
    return b.scene()


def max_disparity():
    """mb = 0.5, mbf = 4: maxD = 8.  Level 0 moved by 8 px, so refined disparities 8 - deltaR land on both sides of maxD (exit 9 / 11);
    right keypoints at uL - maxD exactly, one ulp inside and one ulp outside stage 1's inclusive u gate (exit 4)."""
    b = Builder("max_disparity", (4, 9, 11), 200, 120, 2, seed=8, shift=8, mbf=4.0)
    for i in range(36):
        x0 = 20 + (i * 29) % 160; v = f32(6 + 3 * i)
        ur = f32(x0 - 8)
        ur = [ur, np.nextafter(ur, f32(1e9)), np.nextafter(ur, f32(-1e9))][i % 3]
        b.pair(0, x0, v, ur=ur, tag=("at", "above", "below")[i % 3])
    b.shift = 6                                                    # level 1: 6 px there are 7.2 px in the image
    b.right[1] = np.clip(np.roll(b.left[1], -6, axis=1).astype(np.int32) + b.rng.integers(-3, 4, b.left[1].shape), 0, 255).astype(np.uint8)
    b.fill(20, levels=[1])
    return b.scene()


def saturated():
    """SAD distances in the upper half of their range (ceiling 121 * 510 = 61710), the median included.  Left level: 255 with a 0 on every
    keypoint; right level: 0, the keypoint's row 255, and next to the best column a few 255 whose number falls off with the distance,
    so that SAD(incR) = 58650 - 255 * (255s under the patch) has its minimum inside the window, between 40000 and 58000."""
    b = Builder("saturated", (11,), 200, 120, 2, seed=9, shift=6, noise=0)
    for l in (0, 1):
        b.left[l][:] = 255; b.right[l][:] = 0
        k = 0
        for y0 in range(8, b.rows[l] - 8, 12):
            b.right[l][y0, :] = 255
            for x0 in range(30, b.cols[l] - 20, 40):
                b.left[l][y0, x0] = 0
                e = (k % 7) - 3; peak = 4 + (k * 3) % 7; k += 1    # right keypoint e columns off the best column; 255s in a column: peak, peak - 2, ..
                c = x0 - 6
                for dx in range(-4, 5):
                    m = max(peak - 2 * abs(dx), 0)
                    b.right[l][y0 - 5:y0 - 5 + min(m, 5), c + dx] = 255
                    b.right[l][y0 + 1:y0 + 1 + max(m - 5, 0), c + dx] = 255
                b.pair(l, x0, f32(y0) * b.scale[l], xr=c + e, tag="sat")
    return b.scene()


def _median(name, sads, exits, extra=()):
    """Noise-free levels, one matching pair per entry of `sads` with exactly that SAD distance; `extra` pairs leave before the refinement."""
    b = Builder(name, exits, 200, 120, 2, seed=10 + len(sads) + sum(sads), noise=0)
    for i, s in enumerate(sads):
        l = i % 2; x0, y0 = 30 + 16 * (i % 8), 10 + 13 * (i // 8) + 6 * (i % 2)
        b.pair(l, x0, f32(y0) * b.scale[l], tag="m")
        if s:
            b.bump(l, x0, y0, s)
    for i in range(6):                                             # company that never reaches vDistIdx: too far in Hamming distance
        b.pair(0, 40 + 20 * i, f32(100 + 3 * i), flips=90, tag="far")
    return b.scene()


def median_1(): return _median("median_1", [30], (5,))
def median_2(): return _median("median_2", [20, 50], (5,))              # size / 2 = 1: the median is 50, both stay; (size - 1) / 2 would cut the 50
def median_3(): return _median("median_3", [20, 30, 70], (5,))          # median 30, thDist 63: the 70 goes
def median_equal(): return _median("median_equal", [25] * 24, (5, 11))  # all equal and non-zero: nothing goes
def median_zero(): return _median("median_zero", [0] * 24, (5, 12))     # median 0, thDist 0: everything goes, n_matches == 0


def row_outside():
    """Left keypoints whose row (long long)vL is not a row of level 0 - vL >= rows[0] and vL <= -1 - next to right keypoints of the same
    octave and descriptor whose band reaches across the border: no candidate row, best_r = -1 (exit 1).  vL in (-1, 0) truncates to row 0
    and is searched (its patch then leaves the image, exit 7).  Also left keypoints on rows without any right keypoint (exit 2) and left
    of the image (uL < 0, exit 3)."""
    b = Builder("row_outside", (1, 2, 3, 7), 200, 120, 3, seed=11)
    for i, v in enumerate((120.0, 120.5, 121.0, 121.75, 122.0, 125.0, 1000.0, 70000.0)):
        b.pair(i % 3, 30 + 12 * i, f32(v), dy=float(f32(119.0) - f32(v)), tag="below")
    for i, v in enumerate((-1.0, -1.5, -1.25, -1.75, -1.999, -40.0)):
        b.pair(i % 3, 30 + 12 * i, f32(v), dy=float(f32(1.0) - f32(v)), tag="above")
    for i, v in enumerate((-0.25, -0.5, -0.75, -0.999)):
        b.pair(i % 3, 30 + 12 * i, f32(v), dy=float(f32(1.5) - f32(v)), tag="row0")
    b.fill(30, rows=np.arange(8, 56, 3), levels=[0, 1])
    for i in range(5):
        b.left_kp(f32(40 + 20 * i), f32(80 + 4 * i), i % 3, tag="empty_row")
    for i, u in enumerate((-0.5, -1e-3, -3.0, -100.0)):
        iL = b.left_kp(f32(u), f32(20 + 6 * i), 0, tag="left_of_image")
        b.right_kp(f32(0.0), f32(20 + 6 * i), 0, flip_bits(b.l_desc[iL], 3))
    return b.scene()


GROUP_SIZES = (1, 15, 16, 17, 255, 257)


def groups(n_left):
    """One scene cut to n_left left keypoints: the refinement gives 16 lanes to a keypoint and 16 keypoints to a block."""
    b = Builder("groups_%d" % n_left, (11,) if n_left >= 15 else (), 300, 200, 3, seed=12)
    b.fill(257, spoil_every=9)
    return b.scene(n_left)


SCENES = dict(tall=tall, levels_1=levels_1, levels_3=levels_3, levels_16=levels_16, patch_limits=patch_limits, shifts=shifts,
              zero_disparity=zero_disparity, max_disparity=max_disparity, saturated=saturated, median_1=median_1, median_2=median_2,
              median_3=median_3, median_equal=median_equal, median_zero=median_zero, row_outside=row_outside,
              **{"groups_%d" % n: (lambda n=n: groups(n)) for n in GROUP_SIZES})


def frames(sc):
    """The scene's keypoints as the library's Frame records (left, right)."""
    from lld_slam_amd.orb_search import Frame
    sigma2 = (sc["scale"] * sc["scale"]).astype(f32)
    def one(xy, octave, desc):
        n = octave.shape[0]
        return Frame(desc=desc.copy(), xy=xy.copy(), octave=octave.copy(), uright=np.full(n, -1, f32), angle=np.zeros(n, f32), min_x=0.0, min_y=0.0,
                     max_x=float(sc["width"]), max_y=float(sc["height"]), scale=sc["scale"].copy(), sigma2=sigma2, inv_sigma2=(f32(1.0) / sigma2).astype(f32)).normalise()
    return one(sc["l_xy"], sc["l_oct"], sc["l_desc"]), one(sc["r_xy"], sc["r_oct"], sc["r_desc"])
