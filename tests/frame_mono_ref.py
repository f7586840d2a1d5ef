"""An independent numpy restatement of what lld_frame_build_mono* computes (include/lld_amd.h): Frame::UndistortKeyPoints
(src/Frame.cc:468-498) on the restated cv::undistortPoints, Frame::ComputeStereoFromRGBD (:707-728) on the depth image GrabImageRGBD
receives (src/Tracking.cc:252-253), Frame::ComputeImageBounds (:500-528) and Frame::PosInGrid (:446-456), plus the crafted scenes of the
tests.  It is NOT the reference and not OpenCV: it states, in numpy, the arithmetic the header states, and the device is held to it bit
for bit.  numpy rounds every float64 / float32 operation separately, which is what the header asks of the kernel.  It does not import
lld_slam_amd.
"""
import numpy as np

f32, f64 = np.float32, np.float64
DEPTH_F32, DEPTH_U16 = 0, 1
GRID_COLS, GRID_ROWS = 64, 48

# the camera of the tests: a 416x240 image with TUM1-like coefficients scaled to it
W, H = 416, 240
CAM = (336.25, 335.7, 207.1, 127.6)
DIST5 = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
MBF = 40.0


def _cam64(cam, dist):
    fx, fy, cx, cy = [f64(f32(c)) for c in cam[:4]]
    d = [f64(f32(c)) for c in dist]
    k1, k2, p1, p2 = d[:4]
    k3 = d[4] if len(d) == 5 else f64(0.0)
    return fx, fy, cx, cy, k1, k2, p1, p2, k3


def undistort(xy, cam, dist):
    """mvKeysUn[i].pt from mvKeys[i].pt: [n,2] float32 -> [n,2] float32."""
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 2)
    assert len(dist) in (4, 5)
    if f32(dist[0]) == f32(0.0):                    # mDistCoef.at<float>(0)==0.0, whatever the rest holds
        return xy.copy()
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = _cam64(cam, dist)
    with np.errstate(all="ignore"):
        ifx, ify = f64(1.0) / fx, f64(1.0) / fy
        x0 = (xy[:, 0].astype(f64) - cx) * ifx
        y0 = (xy[:, 1].astype(f64) - cy) * ify
        x, y = x0.copy(), y0.copy()
        for _ in range(5):
            r2 = x * x + y * y
            icdist = f64(1.0) / (f64(1.0) + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = ((f64(2.0) * p1) * x) * y + p2 * (r2 + (f64(2.0) * x) * x)
            dy = p1 * (r2 + (f64(2.0) * y) * y) + ((f64(2.0) * p2) * x) * y
            x = (x0 - dx) * icdist
            y = (y0 - dy) * icdist
        return np.stack([(fx * x + cx).astype(f32), (fy * y + cy).astype(f32)], 1)


def distort(xy_un, cam, dist):
    """The forward model (cv::projectPoints' distortion) in float64: undistorted pixels -> distorted pixels.  Used only to judge the
    undistortion's residual; nothing on the device computes it."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = _cam64(cam, dist)
    a = np.asarray(xy_un, f64).reshape(-1, 2)
    x, y = (a[:, 0] - cx) / fx, (a[:, 1] - cy) / fy
    r2 = x * x + y * y
    cd = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * cd + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * cd + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], 1)


def image_bounds(cols, rows, cam, dist):
    """mnMinX, mnMaxX, mnMinY, mnMaxY as float32."""
    if f32(dist[0]) == f32(0.0):
        return np.array([0.0, cols, 0.0, rows], f32)
    c = undistort(np.array([[0, 0], [cols, 0], [0, rows], [cols, rows]], f32), cam, dist)
    return np.array([min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0]), min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1])], f32)


def grid_inv(bounds):
    """mfGridElementWidthInv, mfGridElementHeightInv (Frame.cc:199-200)."""
    b = np.asarray(bounds, f32)
    return f32(GRID_COLS) / (b[1] - b[0]), f32(GRID_ROWS) / (b[3] - b[2])


def _round_away(v):
    """C's round() on a float: halves away from zero."""
    v = np.asarray(v, f32)
    return (np.sign(v) * np.floor(np.abs(v) + f32(0.5))).astype(np.int64)


def grid_cell(xy_un, bounds):
    """Frame::PosInGrid: (posX, posY, inside)."""
    b = np.asarray(bounds, f32); wi, hi = grid_inv(b)
    a = np.asarray(xy_un, f32).reshape(-1, 2)
    px = _round_away((a[:, 0] - b[0]) * wi); py = _round_away((a[:, 1] - b[2]) * hi)
    return px, py, (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)


def sample_depth(xy, depth, factor):
    """imDepth.at<float>(v,u) after GrabImageRGBD's convertTo, at the DISTORTED keypoints; (d [n] float32, readable [n] bool).  A
    keypoint that is not finite or lies outside (-1, cols) x (-1, rows) reads nothing."""
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 2)
    depth = np.asarray(depth); rows, cols = depth.shape
    factor = f32(factor)
    u, v = xy[:, 0], xy[:, 1]
    with np.errstate(invalid="ignore"):
        ok = (u > f32(-1.0)) & (u < f32(cols)) & (v > f32(-1.0)) & (v < f32(rows))
    col = np.where(ok, np.trunc(np.where(ok, u, 0)), 0).astype(np.int64); row = np.where(ok, np.trunc(np.where(ok, v, 0)), 0).astype(np.int64)
    raw = depth[row, col]
    with np.errstate(all="ignore"):
        if depth.dtype == np.uint16:
            d = raw.astype(f32) * factor
        else:
            assert depth.dtype == f32
            d = raw * factor if np.abs(factor - f32(1.0)) > f32(1e-5) else raw.copy()
    return d.astype(f32), ok


def build(xy, cam, dist, mbf, depth=None, factor=1.0):
    """What the build leaves in the frame: dict(xy_un [n,2], u_right [n], depth [n]) float32."""
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 2)
    n = xy.shape[0]
    un = undistort(xy, cam, dist)
    ur, dep = np.full(n, -1, f32), np.full(n, -1, f32)
    if depth is not None and n:
        d, ok = sample_depth(xy, depth, factor)
        with np.errstate(all="ignore"):
            has = ok & (d > f32(0.0))
            ur[has] = (un[has, 0] - f32(mbf) / d[has]).astype(f32)
        dep[has] = d[has]
    return dict(xy_un=un, u_right=ur, depth=dep)


# ---------------------------------------------------------------------------------------------- scenes
OUT_OF_GRID = np.array([[415.5, 128.0], [414.0, 100.0], [200.0, 239.5]], f32)      # grid column 64, column 64, row 48 on CAM / DIST5


def crafted_keypoints(seed=3, n=300, w=W, h=H, n_levels=8):
    """n keypoints inside a w x h image - the three OUT_OF_GRID ones first, then corners and borders, then a quarter-pixel lattice of
    random positions - with octaves, angles and descriptors."""
    rng = np.random.default_rng(seed)
    xy = np.empty((n, 2), f32)
    fixed = np.concatenate([OUT_OF_GRID, np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [w - 0.25, h - 0.25], [10.99, 7.999],
                                                   [207.1, 127.6], [0.5, 120.0], [208.0, 0.25]], f32)])
    k = min(len(fixed), n)
    xy[:k] = fixed[:k]
    xy[k:, 0] = rng.integers(0, 4 * w, n - k) / 4.0
    xy[k:, 1] = rng.integers(0, 4 * h, n - k) / 4.0
    return dict(xy=xy, octave=rng.integers(0, n_levels, n).astype(np.int32), angle=(rng.random(n) * 360.0).astype(f32),
                desc=rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32))


def depth_image(kind, seed=5, w=W, h=H):
    """Depth images that hold zeros, negative values, NaN and +inf next to plausible depths.  kind: 'f32' (metres, 0.5 .. 8) or 'u16'
    (raw 0 .. 40000; a u16 image has no negatives, NaN or inf - it holds zeros and the extremes 1 and 65535)."""
    rng = np.random.default_rng(seed)
    if kind == "u16":
        d = rng.integers(2500, 40000, (h, w)).astype(np.uint16)
        m = rng.random((h, w))
        d[m < 0.15] = 0; d[(m >= 0.15) & (m < 0.18)] = 1; d[(m >= 0.18) & (m < 0.21)] = 65535
        return d
    d = (0.5 + 7.5 * rng.random((h, w))).astype(f32)
    m = rng.random((h, w))
    d[m < 0.1] = 0.0; d[(m >= 0.1) & (m < 0.13)] = -0.0; d[(m >= 0.13) & (m < 0.2)] = -1.5
    d[(m >= 0.2) & (m < 0.27)] = np.nan; d[(m >= 0.27) & (m < 0.34)] = np.inf; d[(m >= 0.34) & (m < 0.37)] = -np.inf
    return d


def depth_ramp(w=W, h=H):
    """A depth that changes from pixel to pixel, so that a look-up at the undistorted instead of the distorted position reads another value."""
    yy, xx = np.mgrid[0:h, 0:w]
    return (1.0 + xx * 0.01 + yy * 0.013).astype(f32)
