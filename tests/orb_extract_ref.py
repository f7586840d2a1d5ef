"""CPU restatement of ORBextractor::operator() (src/ORBextractor.cc:1043-1105) as include/lld_amd.h defines it: the checker of
lld_orb_extract.  numpy for the image passes, plain loops for DistributeOctTree.  Imports nothing from lld_slam_amd, so it shares no
code with what it checks; cosf / sinf come from the host's libm through ctypes."""
from __future__ import annotations

import ctypes
import ctypes.util
import math

import numpy as np

EDGE_THRESHOLD = 19
PATCH_SIZE = 31
HALF_PATCH_SIZE = 15
MIN_BORDER = EDGE_THRESHOLD - 3
f32 = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.cosf.argtypes = [ctypes.c_float]; _libm.cosf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]; _libm.sinf.restype = ctypes.c_float


def cv_round(x):
    """cvRound: round half to even."""
    return int(np.rint(x))


# ------------------------------------------------------------------------------------------ level tables (:411-470)
def level_tables(nfeatures, scale_factor, nlevels):
    sf = f32(scale_factor)
    scale = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        scale[i] = f32(scale[i - 1] * sf)
    sigma2 = (scale * scale).astype(f32)
    inv_scale = (f32(1) / scale).astype(f32)
    inv_sigma2 = (f32(1) / sigma2).astype(f32)
    factor = f32(f32(1) / sf)
    nd = f32(f32(f32(nfeatures) * f32(f32(1) - factor)) / f32(f32(1) - f32(math.pow(float(factor), float(nlevels)))))
    per = np.zeros(nlevels, np.int32)
    s = 0
    for l in range(nlevels - 1):
        per[l] = cv_round(nd); s += int(per[l]); nd = f32(nd * factor)
    per[nlevels - 1] = max(nfeatures - s, 0)
    vmax = int(math.floor(HALF_PATCH_SIZE * float(f32(math.sqrt(2.0))) / 2 + 1))
    vmin = int(math.ceil(HALF_PATCH_SIZE * float(f32(math.sqrt(2.0))) / 2))
    umax = [0] * (HALF_PATCH_SIZE + 1)
    for v in range(vmax + 1):
        umax[v] = cv_round(f32(math.sqrt(HALF_PATCH_SIZE * HALF_PATCH_SIZE - v * v)))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0; v0 += 1
    return dict(scale=scale, inv_scale=inv_scale, sigma2=sigma2, inv_sigma2=inv_sigma2, per_level=per, umax=np.array(umax, np.int32))


# ------------------------------------------------------------------------------------------ pyramid
def _lin_coef(ssize, dsize):
    scale = 1.0 / (float(dsize) / float(ssize))
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(f32)).astype(f32)
    lo = s < 0
    s[lo] = 0; f[lo] = 0
    hi = s >= ssize - 1
    s[hi] = ssize - 1; f[hi] = 0
    c1 = np.rint(f * f32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, ssize - 1), 2048 - c1, c1


def resize_linear(src, dcols, drows):
    sr, sc = src.shape
    sx0, sx1, a0, a1 = _lin_coef(sc, dcols)
    sy0, sy1, b0, b1 = _lin_coef(sr, drows)
    S = src.astype(np.int64)
    H = S[:, sx0] * a0[None, :] + S[:, sx1] * a1[None, :]
    V = H[sy0, :] * b0[:, None] + H[sy1, :] * b1[:, None]
    return ((V + (1 << 21)) >> 22).astype(np.uint8)


def level_size(cols, rows, inv):
    return cv_round(f32(f32(cols) * inv)), cv_round(f32(f32(rows) * inv))


def pyramid(image, tables):
    levels = [np.ascontiguousarray(image, np.uint8)]
    for l in range(1, len(tables["scale"])):
        c, r = level_size(image.shape[1], image.shape[0], tables["inv_scale"][l])
        levels.append(resize_linear(levels[-1], c, r))
    return levels


# ------------------------------------------------------------------------------------------ FAST
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3)]


def fast_score_patch(p7):
    """Score of the centre of a 7x7 patch: (largest m with 9 contiguous circle pixels all >= p+m or all <= p-m) - 1."""
    p7 = np.asarray(p7, np.int64)
    c = p7[3, 3]
    d = [int(p7[3 + dy, 3 + dx]) - int(c) for dx, dy in CIRCLE]
    best = -1000
    for s in range(16):
        arc = [d[(s + k) & 15] for k in range(9)]
        best = max(best, min(arc), min(-v for v in arc))
    return best - 1


def fast_score_map(img):
    """Score map of a level (pixels whose circle leaves the image score 0; scores below 1 are clamped to 0)."""
    I = img.astype(np.int16)
    R, Cc = I.shape
    out = np.zeros((R, Cc), np.int16)
    if R < 7 or Cc < 7:
        return out
    p = I[3:R - 3, 3:Cc - 3]
    d = np.stack([I[3 + dy:R - 3 + dy, 3 + dx:Cc - 3 + dx] - p for dx, dy in CIRCLE])
    best = np.full(p.shape, -1000, np.int16)
    for s in range(16):
        idx = [(s + k) & 15 for k in range(9)]
        arc = d[idx]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    out[3:R - 3, 3:Cc - 3] = np.maximum(best - 1, 0)
    return out


def level_grid(cols, rows):
    max_bx, max_by = cols - EDGE_THRESHOLD + 3, rows - EDGE_THRESHOLD + 3
    width, height = f32(max_bx - MIN_BORDER), f32(max_by - MIN_BORDER)
    n_cols, n_rows = int(width / f32(30)), int(height / f32(30))
    w_cell = int(math.ceil(f32(width / f32(n_cols)))) if n_cols else 0
    h_cell = int(math.ceil(f32(height / f32(n_rows)))) if n_rows else 0
    return max_bx, max_by, n_cols, n_rows, w_cell, h_cell


def n_ini(cols, rows):
    """DistributeOctTree's initial node count for a level: std::round((maxX - minX) / (maxY - minY)), halves away from zero."""
    max_bx, max_by = cols - EDGE_THRESHOLD + 3, rows - EDGE_THRESHOLD + 3
    return int(math.floor(float(f32(max_bx - MIN_BORDER) / f32(max_by - MIN_BORDER)) + 0.5))


def level_ok(cols, rows):
    """False where the reference divides by zero: no FAST cell (nCols or nRows = 0) or no initial octree node (round(w/h) = 0)."""
    _, _, n_cols, n_rows, _, _ = level_grid(cols, rows)
    return n_cols >= 1 and n_rows >= 1 and n_ini(cols, rows) >= 1


def image_ok(cols, rows, tables):
    """Every level of a cols x rows image passes level_ok: what extract() accepts."""
    return all(level_ok(*(level_size(cols, rows, inv) if l else (cols, rows))) for l, inv in enumerate(tables["inv_scale"]))


def cell_keypoints(score, max_bx, max_by, n_cols, n_rows, w_cell, h_cell, ini_th, min_th, stats):
    """ComputeKeyPointsOctTree's cell loop (:786-832): candidates (x, y relative to minBorder, score) in reference order."""
    out = []
    for i in range(n_rows):
        iniY = f32(MIN_BORDER + i * h_cell)
        maxY = f32(iniY + f32(h_cell) + f32(6))
        if iniY >= max_by - 3:
            continue
        if maxY > max_by:
            maxY = f32(max_by)
        for j in range(n_cols):
            iniX = f32(MIN_BORDER + j * w_cell)
            maxX = f32(iniX + f32(w_cell) + f32(6))
            if iniX >= max_bx - 6:
                continue
            if maxX > max_bx:
                maxX = f32(max_bx)
            y0, x0 = int(iniY), int(iniX)
            sub = score[y0:int(maxY), x0:int(maxX)].astype(np.int32)
            h, w = sub.shape
            found = []
            for pas, th in enumerate((ini_th, min_th)):
                interior = np.zeros((h, w), bool)
                interior[3:h - 3, 3:w - 3] = True
                eff = np.where(interior & (sub >= th), sub, 0)
                pad = np.zeros((h + 2, w + 2), np.int32); pad[1:-1, 1:-1] = eff
                keep = interior & (sub >= th)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if dx or dy:
                            keep &= sub > pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                ys, xs = np.nonzero(keep)                 # row-major
                found = [(x0 + int(x) - MIN_BORDER, y0 + int(y) - MIN_BORDER, int(sub[y, x])) for y, x in zip(ys, xs)]
                if found:
                    break
                stats["cells_min_th" if pas == 0 else "cells_empty"] += 1
            out.extend(found)
    return out


# ------------------------------------------------------------------------------------------ DistributeOctTree (:539-763)
class Node:
    __slots__ = ("x0", "y0", "x1", "y1", "keys", "no_more")

    def __init__(self, x0, y0, x1, y1, keys):
        self.x0, self.y0, self.x1, self.y1, self.keys = x0, y0, x1, y1, keys
        self.no_more = False

    def divide(self, X, Y):
        """DivideNode (:480-537): children n1..n4 with their keys in the parent's order."""
        hx = int(math.ceil(f32(self.x1 - self.x0) / f32(2)))
        hy = int(math.ceil(f32(self.y1 - self.y0) / f32(2)))
        xm, ym = self.x0 + hx, self.y0 + hy
        k = self.keys
        left, top = X[k] < xm, Y[k] < ym
        ch = [Node(self.x0, self.y0, xm, ym, k[left & top]), Node(xm, self.y0, self.x1, ym, k[~left & top]),
              Node(self.x0, ym, xm, self.y1, k[left & ~top]), Node(xm, ym, self.x1, self.y1, k[~left & ~top])]
        for c in ch:
            if len(c.keys) == 1:
                c.no_more = True
        return ch


def distribute_oct_tree(cands, min_x, max_x, min_y, max_y, N, stats):
    """cands: list of (x, y, score) relative to minBorder, in candidate order.  Returns the retained candidates in lNodes order.
    Tie rule (the reference orders equal sizes by heap address): a node created later counts as the larger."""
    X = np.array([c[0] for c in cands], np.int64); Y = np.array([c[1] for c in cands], np.int64)
    Sc = np.array([c[2] for c in cands], np.int64)
    n_ini = int(math.floor(float(f32(max_x - min_x) / f32(max_y - min_y)) + 0.5))     # std::round: halves away from zero
    hX = f32(f32(max_x - min_x) / f32(n_ini))
    ini = [Node(int(f32(hX * f32(i))), 0, int(f32(hX * f32(i + 1))), max_y - min_y, None) for i in range(n_ini)]
    owner = np.array([int(f32(f32(x) / hX)) for x in X], np.int64)
    for i, nd in enumerate(ini):
        nd.keys = np.nonzero(owner == i)[0]
    lst = []
    for nd in ini:
        if len(nd.keys) == 1:
            nd.no_more = True
        if len(nd.keys):
            lst.append(nd)
    created = {}                          # id(node) -> creation counter (stands for the heap address)
    counter = [0]

    def push_children(parent, front, vsize):
        for c in parent.divide(X, Y):
            if len(c.keys) > 0:
                front.append(c)           # push_front: reversed below
                created[id(c)] = counter[0]; counter[0] += 1
                if len(c.keys) > 1:
                    vsize.append(c)

    iteration = sorted_rounds = 0
    finish_unchanged = 0
    vsize = []
    while True:
        iteration += 1
        prev = len(lst)
        vsize = []
        front, rest = [], []
        for nd in lst:
            if nd.no_more:
                rest.append(nd)
            else:
                push_children(nd, front, vsize)
        lst = front[::-1] + rest
        if len(lst) >= N or len(lst) == prev:
            finish_unchanged = int(len(lst) < N)
            break
        if len(lst) + 3 * len(vsize) > N:
            done = False
            while not done:
                sorted_rounds += 1
                prev = len(lst)
                vprev = sorted(vsize, key=lambda n: (len(n.keys), created[id(n)]))
                vsize = []
                front = []
                split = set()
                for nd in reversed(vprev):
                    push_children(nd, front, vsize)
                    split.add(id(nd))
                    if len(lst) - len(split) + len(front) >= N:
                        break
                lst = front[::-1] + [nd for nd in lst if id(nd) not in split]
                if len(lst) >= N or len(lst) == prev:
                    finish_unchanged = int(len(lst) < N)
                    done = True
            break
    stats["iterations"] = iteration; stats["sorted_rounds"] = sorted_rounds; stats["finish_unchanged"] = finish_unchanged
    out = []
    for nd in lst:
        k = nd.keys
        best = k[int(np.argmax(Sc[k]))]                  # argmax: the first of the greatest
        out.append((int(X[best]), int(Y[best]), int(Sc[best])))
    return out


# ------------------------------------------------------------------------------------------ orientation, blur, descriptor
_P = [f32(0.9997878412794807), f32(-0.3258083974640975), f32(0.1555786518463281), f32(-0.04432655554792128)]
_K = f32(180.0 / math.pi)
ATAN_P = [f32(p * _K) for p in _P]


def fast_atan2(y, x):
    """OpenCV's fastAtan2, float polynomial in degrees; y, x float32 arrays."""
    y = np.asarray(y, f32); x = np.asarray(x, f32)
    ax, ay = np.abs(x), np.abs(y)
    eps = f32(np.finfo(np.float64).eps)
    ge = ax >= ay
    c = np.where(ge, ay / (ax + eps), ax / (ay + eps)).astype(f32)
    c2 = (c * c).astype(f32)
    p1, p3, p5, p7 = ATAN_P
    a = ((((((p7 * c2).astype(f32) + p5).astype(f32) * c2).astype(f32) + p3).astype(f32) * c2).astype(f32) + p1).astype(f32)
    a = (a * c).astype(f32)
    a = np.where(ge, a, f32(90) - a).astype(f32)
    a = np.where(x < 0, f32(180) - a, a).astype(f32)
    a = np.where(y < 0, f32(360) - a, a).astype(f32)
    return a


def ic_angle(img, x, y, umax):
    m01 = m10 = 0
    I = img.astype(np.int64)
    for u in range(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1):
        m10 += u * int(I[y, x + u])
    for v in range(1, HALF_PATCH_SIZE + 1):
        d = int(umax[v])
        us = np.arange(-d, d + 1)
        vp, vm = I[y + v, x + us], I[y - v, x + us]
        m10 += int((us * (vp + vm)).sum())
        m01 += v * int((vp - vm).sum())
    return m01, m10


GAUSS_Q8 = np.array([18, 34, 49, 54, 49, 34, 18], np.int64)


def blur(img):
    """The documented integer 7x7 Gaussian (include/lld_amd.h): separable Q8 taps, reflect-101, one rounding at the end."""
    I = img.astype(np.int64)
    R, Cc = I.shape
    xi = np.arange(Cc)[:, None] + np.arange(-3, 4)[None, :]
    xi = np.where(xi < 0, -xi, np.where(xi >= Cc, 2 * Cc - 2 - xi, xi))
    yi = np.arange(R)[:, None] + np.arange(-3, 4)[None, :]
    yi = np.where(yi < 0, -yi, np.where(yi >= R, 2 * R - 2 - yi, yi))
    H = (I[:, xi] * GAUSS_Q8[None, None, :]).sum(axis=2)
    V = (H[yi, :] * GAUSS_Q8[None, :, None]).sum(axis=1)
    return ((V + 32768) >> 16).astype(np.uint8)


FACTOR_PI = f32(math.pi / 180.0)


def descriptors(bimg, pts, angles, pattern):
    """computeOrbDescriptor (:108-148) for keypoints `pts` (level pixels) on the blurred level; returns [n][8] u32."""
    pat = np.asarray(pattern, np.int32).reshape(512, 2).astype(f32)
    out = np.zeros((len(pts), 8), np.uint32)
    step = bimg.shape[1]
    flat = bimg.reshape(-1).astype(np.int32)
    for i, ((x, y), ang) in enumerate(zip(pts, angles)):
        ar = float(f32(f32(ang) * FACTOR_PI))
        a, b = f32(_libm.cosf(ar)), f32(_libm.sinf(ar))
        px, py = pat[:, 0], pat[:, 1]
        ry = np.rint(((px * b).astype(f32) + (py * a).astype(f32)).astype(f32)).astype(np.int64)
        rx = np.rint(((px * a).astype(f32) - (py * b).astype(f32)).astype(f32)).astype(np.int64)
        v = flat[(y + ry) * step + (x + rx)]
        bits = (v[0::2] < v[1::2]).astype(np.uint64)
        words = (bits.reshape(8, 32) << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1)
        out[i] = words.astype(np.uint32)
    return out


# ------------------------------------------------------------------------------------------ the whole operator()
def extract(image, nfeatures, scale_factor, nlevels, ini_th, min_th, pattern):
    """Returns dict(xy, octave, angle, response, size, desc, stats [nlevels][8], levels (pyramid), candidates per level)."""
    T = level_tables(nfeatures, scale_factor, nlevels)
    levels = pyramid(image, T)
    xy, octv, ang, resp, size, desc, stats, cands_all = [], [], [], [], [], [], [], []
    for l, img in enumerate(levels):
        st = dict(n_candidates=0, cells_min_th=0, cells_empty=0, iterations=0, sorted_rounds=0, finish_unchanged=0, n_keypoints=0,
                  features_wanted=int(T["per_level"][l]))
        rows, cols = img.shape
        max_bx, max_by, n_cols, n_rows, w_cell, h_cell = level_grid(cols, rows)
        if not level_ok(cols, rows):
            raise ValueError(f"level {l} ({cols}x{rows}): no FAST cell or no initial octree node (the reference divides by zero)")
        sc = fast_score_map(img)
        cands = cell_keypoints(sc, max_bx, max_by, n_cols, n_rows, w_cell, h_cell, ini_th, min_th, st)
        st["n_candidates"] = len(cands)
        cands_all.append(cands)
        kps = distribute_oct_tree(cands, MIN_BORDER, max_bx, MIN_BORDER, max_by, int(T["per_level"][l]), st)
        st["n_keypoints"] = len(kps)
        pts = [(x + MIN_BORDER, y + MIN_BORDER) for x, y, _ in kps]
        angles = []
        for x, y in pts:
            m01, m10 = ic_angle(img, x, y, T["umax"])
            angles.append(fast_atan2(f32(m01), f32(m10))[()])
        angles = np.array(angles, f32)
        d = descriptors(blur(img), pts, angles, pattern) if pts else np.zeros((0, 8), np.uint32)
        s = T["scale"][l]
        for (x, y), a, (_, _, r), dd in zip(pts, angles, kps, d):
            xy.append((f32(f32(x) * s), f32(f32(y) * s)) if l else (f32(x), f32(y)))
            octv.append(l); ang.append(a); resp.append(f32(r)); size.append(f32(int(f32(f32(PATCH_SIZE) * s))))
            desc.append(dd)
        stats.append([st[k] for k in ("n_candidates", "cells_min_th", "cells_empty", "iterations", "sorted_rounds", "finish_unchanged",
                                      "n_keypoints", "features_wanted")])
    n = len(xy)
    return dict(xy=np.array(xy, f32).reshape(n, 2), octave=np.array(octv, np.int32), angle=np.array(ang, f32),
                response=np.array(resp, f32), size=np.array(size, f32), desc=np.array(desc, np.uint32).reshape(n, 8),
                stats=np.array(stats, np.int32), levels=levels, candidates=cands_all, tables=T)


def seeded_pattern(seed=0):
    """A stand-in for ORBextractor::pattern: 256 point pairs with coordinates in [-13, 12] (the published pattern's range)."""
    return np.random.default_rng(seed).integers(-13, 13, size=(256, 4)).astype(np.int32)
