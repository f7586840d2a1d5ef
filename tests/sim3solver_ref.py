"""Independent restatement of ORB-SLAM2's Sim3Solver (src/Sim3Solver.cc) with the two deviations of include/lld_amd.h: one glibc
TYPE_3 rand() stream per solver, and the numerics OpenCV would decide (products summed in double in index order, cv::eigen as a
cyclic Jacobi with canonical signs, cv::Rodrigues written out).  Imports nothing from lld_slam_amd; the stream, the Jacobi and
the sign rule come from tests/pnp_ref.py.

Horn's method is written in Python scalars on purpose: a float value is held in a Python float, a float operation is the double
operation rounded to float once (exact for + - * / of floats), and every double operation is one IEEE operation in the order
the kernels of lld_sim3solver.hip use (they are compiled without FMA contraction).  CheckInliers runs over all correspondences
with numpy float32 / float64 element-wise arithmetic in the same order.

Also: a seeded scene generator for a loop pair (two keyframes whose camera points are related by a known Sim3 with a non-trivial
rotation, octaves 0-7, sub-pixel noise, outliers) and its variants."""
from __future__ import annotations

import math

import numpy as np

from pnp_ref import GlibcRand, canonical, draw_set, jacobi_eig

F32 = np.float32
DBL_EPSILON = 2.220446049250313e-16
DEFAULT_PARAMS = (0.99, 20, 300)      # SetRansacParameters as LoopClosing::ComputeSim3 calls it (LoopClosing.cc:277)
LEVEL_SIGMA2 = np.array([np.float32(np.float32(1.44) ** np.float32(l)) for l in range(8)], np.float32)


def f32(x: float) -> float:
    """The float nearest to x, as a Python float."""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(x))


def _div(a: float, b: float) -> float:
    """a / b with IEEE semantics (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def dot3f(a, b) -> float:
    """A float 3-product: the exact double products summed in index order from the first, rounded to float once."""
    s = a[0] * b[0]
    s += a[1] * b[1]
    s += a[2] * b[2]
    return f32(s)


def max_error(sigma2) -> np.ndarray:
    """mvnMaxError: 9.210*sigmaSquare in double pushed into a std::vector<size_t> (truncated), compared as float."""
    return np.array([float(int(9.210 * float(s))) for s in np.asarray(sigma2, F32)], F32)


def camera_points(R, t, xyz) -> np.ndarray:
    """Rcw*X + tcw per point (float): each row a dot3f, then the float + t."""
    R = np.asarray(R, F32).reshape(3, 3).astype(np.float64)
    t = np.asarray(t, F32).reshape(3)
    X = np.asarray(xyz, F32).reshape(-1, 3).astype(np.float64)
    out = np.empty(X.shape, F32)
    for r in range(3):
        s = R[r, 0] * X[:, 0]
        s = s + R[r, 1] * X[:, 1]
        s = s + R[r, 2] * X[:, 2]
        out[:, r] = s.astype(F32) + t[r]
    return out


def to_image(Xc, k) -> np.ndarray:
    """FromCameraToImage (:403-421) in float: invz = 1/z, x = X*invz, u = fx*x + cx."""
    Xc = np.asarray(Xc, F32)
    fx, fy, cx, cy = (F32(v) for v in k)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F32(1.0) / Xc[:, 2]
        x = Xc[:, 0] * invz
        y = Xc[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], 1).astype(F32)


def project(T, Xc, k) -> np.ndarray:
    """Project (:380-400) with T = [R | t] (3x4 float): P3Dc = R*X + t, then as FromCameraToImage."""
    T = np.asarray(T, F32).reshape(3, 4)
    return to_image(camera_points(T[:, :3], T[:, 3], Xc), k)


def check_inliers(T12, T21, X1, X2, P1im1, P2im2, err1, err2, k1, k2):
    """CheckInliers (:340-364): (mask, count).  err = dist.dot(dist) summed in double, as float; both below their thresholds."""
    with np.errstate(invalid="ignore", over="ignore"):
        p21 = project(T12, X2, k1)
        p12 = project(T21, X1, k2)
        d1 = (P1im1 - p21).astype(np.float64)
        d2 = (p12 - P2im2).astype(np.float64)
        e1 = (d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]).astype(F32)
        e2 = (d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]).astype(F32)
    mask = (e1 < err1) & (e2 < err2)
    return mask, int(mask.sum()), e1, e2


def compute_sim3(P1, P2, fix_scale):
    """ComputeSim3 (:226-337) on 3 points each (P1[i] = point i's float xyz).  Returns dict(R, t, s, T12, T21) of floats."""
    P1 = [[float(v) for v in p] for p in P1]
    P2 = [[float(v) for v in p] for p in P2]
    O1 = [f32(f32(f32(P1[0][r] + P1[1][r]) + P1[2][r]) / 3.0) for r in range(3)]
    O2 = [f32(f32(f32(P2[0][r] + P2[1][r]) + P2[2][r]) / 3.0) for r in range(3)]
    Pr1 = [[f32(P1[i][r] - O1[r]) for i in range(3)] for r in range(3)]          # Pr1[r][i]: coordinate r of point i
    Pr2 = [[f32(P2[i][r] - O2[r]) for i in range(3)] for r in range(3)]
    M = [[dot3f(Pr2[i], Pr1[j]) for j in range(3)] for i in range(3)]            # Pr2 * Pr1^T
    N11 = f32(f32(M[0][0] + M[1][1]) + M[2][2])
    N12 = f32(M[1][2] - M[2][1])
    N13 = f32(M[2][0] - M[0][2])
    N14 = f32(M[0][1] - M[1][0])
    N22 = f32(f32(M[0][0] - M[1][1]) - M[2][2])
    N23 = f32(M[0][1] + M[1][0])
    N24 = f32(M[2][0] + M[0][2])
    N33 = f32(f32(-M[0][0] + M[1][1]) - M[2][2])
    N34 = f32(M[1][2] + M[2][1])
    N44 = f32(f32(-M[0][0] - M[1][1]) + M[2][2])
    A = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    lam, V = jacobi_eig(A, 4)                                                    # cv::eigen: largest eigenvalue, lowest index on a tie
    e = 0
    for k in range(1, 4):
        if lam[k] > lam[e]:
            e = k
    q = [f32(x) for x in canonical([V[k][e] for k in range(4)])]
    nv = q[1] * q[1]
    nv += q[2] * q[2]
    nv += q[3] * q[3]
    nv = math.sqrt(nv)
    ang = math.atan2(nv, q[0])
    alpha = _div(2.0 * ang, nv)
    vec = [f32(q[k + 1] * alpha) for k in range(3)]
    th = vec[0] * vec[0]
    th += vec[1] * vec[1]
    th += vec[2] * vec[2]
    th = math.sqrt(th)
    if th < DBL_EPSILON:                                                         # cv::Rodrigues
        R = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    else:
        r = [vec[0] / th, vec[1] / th, vec[2] / th]
        if math.isfinite(th):
            c, sn = math.cos(th), math.sin(th)
        else:
            c = sn = math.nan
        c1 = 1.0 - c
        K = [[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]]
        R = [[f32((c * (1.0 if i == j else 0.0) + c1 * (r[i] * r[j])) + sn * K[i][j]) for j in range(3)] for i in range(3)]
    P3 = [[dot3f(R[i], [Pr2[0][j], Pr2[1][j], Pr2[2][j]]) for j in range(3)] for i in range(3)]
    if fix_scale:
        s = 1.0
    else:
        nom = Pr1[0][0] * P3[0][0]
        den = f32(P3[0][0] * P3[0][0])
        for q9 in range(1, 9):
            i, j = divmod(q9, 3)
            nom += Pr1[i][j] * P3[i][j]
            den += f32(P3[i][j] * P3[i][j])
        s = f32(_div(nom, den))
    sR = [[f32(s * R[i][j]) for j in range(3)] for i in range(3)]
    t = [f32(O1[i] - dot3f(sR[i], O2)) for i in range(3)]
    inv = _div(1.0, s)
    sRi = [[f32(inv * R[j][i]) for j in range(3)] for i in range(3)]
    ti = [-dot3f(sRi[i], t) for i in range(3)]
    T12 = np.array([sR[i] + [t[i]] for i in range(3)], F32)
    T21 = np.array([sRi[i] + [ti[i]] for i in range(3)], F32)
    return dict(R=np.array(R, F32), t=np.array(t, F32), s=F32(s), T12=T12, T21=T21)


def ransac_constants(N, probability=0.99, min_inliers=20, max_iterations=300):
    """SetRansacParameters (:114-138): mRansacMaxIts."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        eps = F32(min_inliers) / F32(N)                                          # (float)minInliers/N
        if min_inliers == N:
            n_it = 1
        else:
            q = np.log(np.float64(1 - probability)) / np.log(np.float64(1 - math.pow(float(eps), 3)))
            # N < minInliers makes epsilon > 1 and the quotient NaN; the (int) of it is INT_MIN on x86-64, so the budget is 1
            n_it = math.ceil(q) if np.isfinite(q) else -(1 << 31)
    return max(1, min(n_it, max_iterations))


class Sim3SolverRef:
    """Sim3Solver with its state across iterate() calls.  `hyps` collects every hypothesis of the last call."""

    def __init__(self, xyz1, xyz2, sigma2_1, sigma2_2, index1, n1, Rcw1, tcw1, Rcw2, tcw2, K1, K2, fix_scale, seed,
                 params=DEFAULT_PARAMS):
        self.X1 = camera_points(Rcw1, tcw1, xyz1)                               # mvX3Dc1
        self.X2 = camera_points(Rcw2, tcw2, xyz2)
        self.K1 = tuple(float(F32(v)) for v in K1)
        self.K2 = tuple(float(F32(v)) for v in K2)
        self.P1im1 = to_image(self.X1, self.K1)
        self.P2im2 = to_image(self.X2, self.K2)
        self.err1 = max_error(sigma2_1)
        self.err2 = max_error(sigma2_2)
        self.index1 = np.ascontiguousarray(index1, np.int64)
        self.n1 = int(n1)
        self.fix_scale = bool(fix_scale)
        self.N = len(self.X1)
        self.rng = GlibcRand(seed)
        self.n_iterations = 0
        self.best_inliers = 0
        self.best = None                                                        # dict(R, t, s, T12) of mBest*
        self.set_ransac_parameters(*params)

    def set_ransac_parameters(self, probability=0.99, min_inliers=20, max_iterations=300):
        self.min_inliers = min_inliers
        self.max_its = ransac_constants(self.N, probability, min_inliers, max_iterations)
        self.n_iterations = 0

    def check(self, h):
        return check_inliers(h["T12"], h["T21"], self.X1, self.X2, self.P1im1, self.P2im2, self.err1, self.err2, self.K1, self.K2)

    def sample(self):
        return draw_set(self.rng, self.N, 3)

    def hypothesis(self, idx):
        return compute_sim3(self.X1[idx], self.X2[idx], self.fix_scale)

    def iterate(self, n):
        """Returns dict(T12 (3x4 float32) or None, no_more, inliers (uint8[n1]), n_inliers)."""
        self.hyps = []
        out = dict(T12=None, no_more=False, inliers=np.zeros(self.n1, np.uint8), n_inliers=0)
        if self.N < self.min_inliers:
            out["no_more"] = True
            return out
        cur = 0
        while self.n_iterations < self.max_its and cur < n:
            cur += 1
            self.n_iterations += 1
            idx = self.sample()
            h = self.hypothesis(idx)
            mask, cnt, _, _ = self.check(h)
            h.update(idx=idx, n_inliers=cnt, record=cnt >= self.best_inliers)
            self.hyps.append(h)
            if cnt >= self.best_inliers:
                self.best_inliers = cnt
                self.best = h
                if cnt > self.min_inliers:
                    out["T12"] = h["T12"].copy()
                    out["n_inliers"] = cnt
                    out["inliers"][self.index1[mask]] = 1
                    return out
        if self.n_iterations >= self.max_its:
            out["no_more"] = True
        return out

    def find(self):
        return self.iterate(self.max_its)

    # GetEstimatedRotation / Translation / Scale: the best hypothesis
    def GetEstimatedRotation(self):
        return None if self.best is None else self.best["R"].copy()

    def GetEstimatedTranslation(self):
        return None if self.best is None else self.best["t"].copy()

    def GetEstimatedScale(self):
        return None if self.best is None else self.best["s"]


def loop_rounds(solvers, active=None, n=5, max_rounds=1000):
    """LoopClosing::ComputeSim3's RANSAC loop (LoopClosing.cc:289-342) without the steps after a pose: iterate(5) on every
    candidate not yet discarded; a candidate with no_more is discarded.  A candidate with a pose stays in play, as it does in the
    reference when its OptimizeSim3 keeps fewer than 20 inliers.  Returns the per-round outputs (list of lists, None = skipped)."""
    live = [True] * len(solvers) if active is None else list(active)
    rounds = []
    for _ in range(max_rounds):
        if not any(live):
            break
        row = []
        for i, s in enumerate(solvers):
            if not live[i]:
                row.append(None)
                continue
            o = s.iterate(n)
            row.append(o)
            if o["no_more"]:
                live[i] = False
        rounds.append(row)
    return rounds


# ------------------------------------------------------------------ scenes
KITTI = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, w=1241, h=376)
KITTI2 = dict(fx=707.0912, fy=707.0912, cx=601.8873, cy=183.1104, w=1241, h=376)


def rotation(rng, scale):
    w = rng.normal(0, scale, 3)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def make_scene(seed, n, inlier_ratio=0.7, noise=0.3, fix_scale=False, variant=None, n1=None):
    """One loop pair: N matched MapPoints of KF1 and KF2.  The true S12 maps KF2's camera frame into KF1's (X1c = s R X2c + t);
    inliers carry lateral noise of `noise` pixels times the octave's sigma; outliers' KF2 points are uniform in KF2's frustum.
    Variants: 'exact' (no noise, no outliers), 'collinear' (every point on one 3D line), 'duplicate' (a third of the
    correspondences repeat earlier ones), 'behind' (a quarter of KF1's points behind the camera), 'identity' (KF2 = KF1: every
    sample's rotation is exactly the identity, the NaN path)."""
    rng = np.random.default_rng(seed)
    cam1, cam2 = KITTI, KITTI2
    R12 = rotation(rng, 0.25)
    s12 = 1.0 if fix_scale else float(rng.uniform(0.6, 1.6))
    t12 = rng.normal(0, 0.5, 3)
    depth = rng.uniform(4.0, 30.0, n)
    u0 = rng.uniform(0, cam1["w"], n); v0 = rng.uniform(0, cam1["h"], n)
    X1c = np.stack([(u0 - cam1["cx"]) / cam1["fx"] * depth, (v0 - cam1["cy"]) / cam1["fy"] * depth, depth], 1)
    if variant == "collinear":
        a = X1c[0]; b = X1c[1]
        X1c = a + rng.uniform(-1, 2, n)[:, None] * (b - a)
    if variant == "behind":
        X1c[: n // 4, 2] *= -1.0
    X2c = ((X1c - t12) @ R12) / s12                                           # X2c = S21 X1c
    level1 = rng.integers(0, 8, n)
    level2 = rng.integers(0, 8, n)
    out = np.zeros(n, bool)
    if variant not in ("exact", "identity"):
        sig = noise * np.sqrt(LEVEL_SIGMA2[level2].astype(np.float64))
        X2c[:, 0] += rng.normal(0, 1, n) * sig * X2c[:, 2] / cam2["fx"]
        X2c[:, 1] += rng.normal(0, 1, n) * sig * X2c[:, 2] / cam2["fy"]
        out = rng.random(n) >= inlier_ratio
        d2 = rng.uniform(4.0, 30.0, out.sum())
        X2c[out] = np.stack([rng.uniform(-0.8, 0.8, out.sum()) * d2, rng.uniform(-0.25, 0.25, out.sum()) * d2, d2], 1)
    if variant == "duplicate":
        k = n // 3
        src = rng.integers(0, n - k, k)
        X1c[n - k:] = X1c[src]; X2c[n - k:] = X2c[src]
    R1 = rotation(rng, 0.5); t1 = rng.normal(0, 3.0, 3)
    R2 = rotation(rng, 0.5); t2 = rng.normal(0, 3.0, 3)
    if variant == "identity":
        R2, t2, X2c = R1, t1, X1c.copy()
        level2 = level1
    Xw1 = (X1c - t1) @ R1                                                     # Xc = R Xw + t
    Xw2 = (X2c - t2) @ R2
    n1 = n1 if n1 is not None else min(n + n // 2, 8192)
    idx1 = np.sort(rng.choice(n1, n, replace=False)).astype(np.int32)
    sc = dict(xyz1=Xw1.astype(F32), xyz2=Xw2.astype(F32), sigma2_1=LEVEL_SIGMA2[level1], sigma2_2=LEVEL_SIGMA2[level2],
              index1=idx1, n1=n1, Rcw1=R1.astype(F32), tcw1=t1.astype(F32), Rcw2=R2.astype(F32), tcw2=t2.astype(F32),
              K1=(cam1["fx"], cam1["fy"], cam1["cx"], cam1["cy"]), K2=(cam2["fx"], cam2["fy"], cam2["cx"], cam2["cy"]),
              fix_scale=bool(fix_scale), seed=int(rng.integers(0, 1 << 32)), R12=R12, t12=t12, s12=s12, outlier=out)
    if variant == "identity":
        sc["xyz2"] = sc["xyz1"].copy()
    return sc


def solver_from_scene(sc, params=DEFAULT_PARAMS):
    return Sim3SolverRef(sc["xyz1"], sc["xyz2"], sc["sigma2_1"], sc["sigma2_2"], sc["index1"], sc["n1"], sc["Rcw1"], sc["tcw1"],
                         sc["Rcw2"], sc["tcw2"], sc["K1"], sc["K2"], sc["fix_scale"], sc["seed"], params)
