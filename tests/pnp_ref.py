"""Independent fp64 restatement of ORB-SLAM2's PnPsolver (src/PnPsolver.cc) with the two deviations of include/lld_amd.h:
one glibc TYPE_3 rand() stream per solver, and the null-space basis of a minimal set from a Householder QR of M^T (cyclic Jacobi
eigendecompositions everywhere the reference calls cvSVD on a symmetric or 3x3 matrix).  Imports nothing from lld_slam_amd.

The core is written in Python scalars on purpose: every sum runs in ascending index order and every product / quotient is one
IEEE double operation, in the order the kernels of lld_pnp.hip use (they are compiled without FMA contraction).  CheckInliers
keeps the reference's float / double mix with numpy float32 / float64 element-wise arithmetic.  Sums over correspondences use
np.cumsum, which accumulates sequentially.

Also: a seeded scene generator (KITTI-like camera, octaves 0-7, inliers with sub-pixel noise, outliers uniform in the image,
coplanar / behind-the-camera / duplicated-point variants)."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
RAND_MAX = 2147483647
JACOBI_SWEEPS = 40          # most sweeps of the cyclic Jacobi (LLD_PNP_JACOBI_SWEEPS)
JACOBI_TOL = 1e-36          # stop when sum of squared off-diagonals <= JACOBI_TOL * sum of squared diagonals
PINV_CUT = 1e-14            # eigenvalue of A^T A kept when > PINV_CUT * the largest (singular value > 1e-7 * the largest)


# ------------------------------------------------------------------ glibc rand() (TYPE_3 additive feedback generator)
class GlibcRand:
    """rand() after srand(seed): r[0] = seed (0 -> 1), r[i] = 16807 r[i-1] mod (2^31 - 1) for i < 31 (Schrage's method on int32),
    r[31..33] = r[0..2], then r[i] = r[i-3] + r[i-31] mod 2^32; outputs r[i] >> 1 from i = 344 (310 warm-up values discarded)."""

    def __init__(self, seed: int):
        seed &= 0xFFFFFFFF
        if seed == 0:
            seed = 1
        word = seed - (1 << 32) if seed >= 1 << 31 else seed      # int32_t word = seed
        r = [word]
        for _ in range(1, 31):
            hi = int(word / 127773)                                   # C division truncates toward zero
            lo = word - hi * 127773
            word = 16807 * lo - 2836 * hi
            if word < 0:
                word += 2147483647
            r.append(word)
        r = [x & 0xFFFFFFFF for x in r]
        r += r[0:3]
        self.ring = r[3:34]                                           # r[i-31 .. i-1] for i = 34
        self.head = 0                                                 # ring[head] = r[i-31]
        for _ in range(310):
            self._next()

    def _next(self) -> int:
        h = self.head
        x = (self.ring[h] + self.ring[(h + 28) % 31]) & 0xFFFFFFFF
        self.ring[h] = x
        self.head = (h + 1) % 31
        return x

    def rand(self) -> int:
        return self._next() >> 1

    def random_int(self, lo: int, hi: int) -> int:
        """DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50)."""
        d = hi - lo + 1
        return int((float(self.rand()) / (float(RAND_MAX) + 1.0)) * d) + lo


def draw_set(rng: GlibcRand, N: int, K: int) -> list[int]:
    """One minimal set: vAvailableIndices = mvAllIndices, then K x (RandomInt over the remaining, take, move the back into its
    place, pop_back)."""
    avail = list(range(N))
    idx = []
    for _ in range(K):
        r = rng.random_int(0, len(avail) - 1)
        idx.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return idx


def glibc_rand_sequence(seed: int, n: int) -> list[int]:
    g = GlibcRand(seed)
    return [g.rand() for _ in range(n)]


# ------------------------------------------------------------------ small dense linear algebra (row-major Python lists)
def jacobi_eig(A: list[list[float]], n: int):
    """Cyclic Jacobi on a symmetric n x n matrix (modified in place).  Returns (eigenvalues, V) with V's columns the eigenvectors."""
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for _ in range(JACOBI_SWEEPS):
        off = 0.0
        dg = 0.0
        for p in range(n):
            dg += A[p][p] * A[p][p]
            for q in range(p + 1, n):
                off += A[p][q] * A[p][q]
        if off <= JACOBI_TOL * dg:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    akp = A[k][p]; akq = A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(n):
                    apk = A[p][k]; aqk = A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                A[p][q] = 0.0
                A[q][p] = 0.0
                for k in range(n):
                    vkp = V[k][p]; vkq = V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return [A[i][i] for i in range(n)], V


def order_by_abs(lam: list[float], n: int) -> list[int]:
    """Selection sort of the indices by ascending |lambda| (a strictly smaller value moves; the same swaps as the kernel)."""
    o = list(range(n))
    for i in range(n):
        m = i
        for j in range(i + 1, n):
            if abs(lam[o[j]]) < abs(lam[o[m]]):
                m = j
        o[i], o[m] = o[m], o[i]
    return o


def canonical(v: list[float]) -> list[float]:
    """Sign of an eigenvector fixed: its first largest-magnitude component positive."""
    m = 0
    for k in range(1, len(v)):
        if abs(v[k]) > abs(v[m]):
            m = k
    return [-x for x in v] if v[m] < 0.0 else list(v)


def ata(A: list[list[float]], m: int, n: int) -> list[list[float]]:
    B = [[0.0] * n for _ in range(n)]
    for a in range(n):
        for b in range(a, n):
            s = 0.0
            for i in range(m):
                s += A[i][a] * A[i][b]
            B[a][b] = s
            B[b][a] = s
    return B


def pinv_eig(A: list[list[float]], m: int, n: int):
    """Jacobi eigendecomposition of A^T A and the reciprocal eigenvalues kept by the PINV_CUT cutoff (the others 0)."""
    lam, V = jacobi_eig(ata(A, m, n), n)
    lmax = 0.0
    for k in range(n):
        if abs(lam[k]) > lmax:
            lmax = abs(lam[k])
    w = [(1.0 / lam[k]) if lam[k] > PINV_CUT * lmax else 0.0 for k in range(n)]
    return V, w


def pinv_solve(V, w, n: int, atb: list[float]) -> list[float]:
    """(A^T A)^+ atb = sum_k V[:, k] (w_k (V[:, k] . atb))."""
    y = [0.0] * n
    for k in range(n):
        s = 0.0
        for c in range(n):
            s += V[c][k] * atb[c]
        y[k] = w[k] * s
    x = [0.0] * n
    for a in range(n):
        s = 0.0
        for k in range(n):
            s += V[a][k] * y[k]
        x[a] = s
    return x


def lstsq(A: list[list[float]], m: int, n: int, b: list[float]) -> list[float]:
    """cvSolve(A, b, x, CV_SVD) restated as x = A^+ b = (A^T A)^+ A^T b."""
    V, w = pinv_eig(A, m, n)
    atb = [0.0] * n
    for c in range(n):
        s = 0.0
        for i in range(m):
            s += A[i][c] * b[i]
        atb[c] = s
    return pinv_solve(V, w, n, atb)


def inv3(CC: list[list[float]]) -> list[list[float]]:
    """cvInvert(CC, CV_SVD) restated as the pseudo-inverse (A^T A)^+ A^T; its column b is (A^T A)^+ applied to row b of A."""
    V, w = pinv_eig(CC, 3, 3)
    P = [[0.0] * 3 for _ in range(3)]
    for b in range(3):
        col = pinv_solve(V, w, 3, [CC[b][0], CC[b][1], CC[b][2]])
        for a in range(3):
            P[a][b] = col[a]
    return P


def _div(a: float, b: float) -> float:
    """a / b as IEEE (and the kernel) divide: x / 0 is +-inf or NaN instead of Python's ZeroDivisionError."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def rotation_from_abt(abt: list[list[float]]):
    """cvSVD(ABt) -> U, V and R = U V^T (PnPsolver.cc:600-604): V from the Jacobi eigendecomposition of ABt^T ABt sorted by
    descending |lambda|, u_k = ABt v_k / s_k; a third column whose singular value is cut is completed by u0 x u1."""
    lam, V = jacobi_eig(ata(abt, 3, 3), 3)
    o = order_by_abs(lam, 3)
    o = [o[2], o[1], o[0]]
    lmax = abs(lam[o[0]])
    vs, us = [], []
    for k in range(3):
        v = canonical([V[0][o[k]], V[1][o[k]], V[2][o[k]]])
        lk = lam[o[k]]
        if lk > PINV_CUT * lmax:
            s = math.sqrt(lk)
            u = [(abt[i][0] * v[0] + abt[i][1] * v[1] + abt[i][2] * v[2]) / s for i in range(3)]
        elif k == 2 and len(us) == 2 and us[1] is not None:
            a, b = us[0], us[1]
            u = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        else:
            u = None
        vs.append(v)
        us.append(u)
    R = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                uik = us[k][i] if us[k] is not None else 0.0
                s += uik * vs[k][j]
            R[i][j] = s
    return R


# ------------------------------------------------------------------ EPnP (PnPsolver.cc:375-952)
def _cumsum_last(x: np.ndarray) -> np.ndarray:
    """Sequential sum over axis 0 (ascending index), as the reference's loops and the kernels accumulate."""
    return np.cumsum(np.concatenate([np.zeros((1,) + x.shape[1:]), x]), axis=0)[-1]


def _fill_L(v):
    dv = []
    for i in range(4):
        a, b = 0, 1
        rows = []
        for _ in range(6):
            rows.append([v[i][3 * a + k] - v[i][3 * b + k] for k in range(3)])
            b += 1
            if b > 3:
                a += 1
                b = a + 1
        dv.append(rows)
    L = []
    for i in range(6):
        L.append([dot3(dv[0][i], dv[0][i]), 2.0 * dot3(dv[0][i], dv[1][i]), dot3(dv[1][i], dv[1][i]),
                  2.0 * dot3(dv[0][i], dv[2][i]), 2.0 * dot3(dv[1][i], dv[2][i]), dot3(dv[2][i], dv[2][i]),
                  2.0 * dot3(dv[0][i], dv[3][i]), 2.0 * dot3(dv[1][i], dv[3][i]), 2.0 * dot3(dv[2][i], dv[3][i]),
                  dot3(dv[3][i], dv[3][i])])
    return L


def _dist2(p, q):
    return (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2])


def _qr_solve(A, b):
    """PnPsolver::qr_solve (:840-952), literally: Householder with eta scaling, A 6 x 4.  Returns None where the reference
    returns early (eta == 0) without writing X."""
    nr, nc = 6, 4
    A = [row[:] for row in A]
    b = b[:]
    A1 = [0.0] * nc
    A2 = [0.0] * nc
    for k in range(nc):
        eta = abs(A[k][k])
        for i in range(k + 1, nr):
            elt = abs(A[i][k])
            if eta < elt:
                eta = elt
        if eta == 0:
            return None
        s = 0.0
        inv_eta = _div(1.0, eta)
        for i in range(k, nr):
            A[i][k] *= inv_eta
            s += A[i][k] * A[i][k]
        sigma = math.sqrt(s)
        if A[k][k] < 0:
            sigma = -sigma
        A[k][k] += sigma
        A1[k] = sigma * A[k][k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s += A[i][k] * A[i][j]
            tau = _div(s, A1[k])
            for i in range(k, nr):
                A[i][j] -= tau * A[i][k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i][j] * b[i]
        tau = _div(tau, A1[j])
        for i in range(j, nr):
            b[i] -= tau * A[i][j]
    x = [0.0] * nc
    x[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s += A[i][j] * x[j]
        x[i] = _div(b[i] - s, A2[i])
    return x


def _gauss_newton(L, rho, betas):
    x = [0.0] * 4                      # the reference's x[4] is left unwritten when qr_solve returns early; here it starts at 0
    for _ in range(5):
        A, bb = [], []
        for i in range(6):
            r = L[i]
            A.append([2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3],
                      r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3],
                      r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3],
                      r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3]])
            bb.append(rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] +
                                r[3] * betas[0] * betas[2] + r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] +
                                r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] + r[8] * betas[2] * betas[3] +
                                r[9] * betas[3] * betas[3]))
        xx = _qr_solve(A, bb)
        if xx is not None:
            x = xx
        for i in range(4):
            betas[i] += x[i]
    return betas


def _betas(L, rho):
    out = []
    b4 = lstsq([[r[0], r[1], r[3], r[6]] for r in L], 6, 4, rho)
    if b4[0] < 0:
        b0 = math.sqrt(-b4[0]); bet = [b0, _div(-b4[1], b0), _div(-b4[2], b0), _div(-b4[3], b0)]
    else:
        b0 = math.sqrt(b4[0]); bet = [b0, _div(b4[1], b0), _div(b4[2], b0), _div(b4[3], b0)]
    out.append(_gauss_newton(L, rho, bet))
    b3 = lstsq([[r[0], r[1], r[2]] for r in L], 6, 3, rho)
    if b3[0] < 0:
        bet = [math.sqrt(-b3[0]), math.sqrt(-b3[2]) if b3[2] < 0 else 0.0, 0.0, 0.0]
    else:
        bet = [math.sqrt(b3[0]), math.sqrt(b3[2]) if b3[2] > 0 else 0.0, 0.0, 0.0]
    if b3[1] < 0:
        bet[0] = -bet[0]
    out.append(_gauss_newton(L, rho, bet))
    b5 = lstsq([[r[0], r[1], r[2], r[3], r[4]] for r in L], 6, 5, rho)
    if b5[0] < 0:
        bet = [math.sqrt(-b5[0]), math.sqrt(-b5[2]) if b5[2] < 0 else 0.0, 0.0, 0.0]
    else:
        bet = [math.sqrt(b5[0]), math.sqrt(b5[2]) if b5[2] > 0 else 0.0, 0.0, 0.0]
    if b5[1] < 0:
        bet[0] = -bet[0]
    bet[2] = _div(b5[3], bet[0])
    out.append(_gauss_newton(L, rho, bet))
    return out


def householder_null4(Mt: list[list[float]]):
    """Columns 9..12 of Q of the Householder QR of M^T (12 x 8): the null space of a minimal set's M, in that order."""
    A = [row[:] for row in Mt]
    hb = [0.0] * 8
    for k in range(8):
        s = 0.0
        for i in range(k, 12):
            s += A[i][k] * A[i][k]
        sigma = math.sqrt(s)
        if A[k][k] < 0.0:
            sigma = -sigma
        v0 = A[k][k] + sigma
        hb[k] = sigma * v0
        A[k][k] = v0
        if hb[k] == 0.0:
            continue
        for j in range(k + 1, 8):
            d = 0.0
            for i in range(k, 12):
                d += A[i][k] * A[i][j]
            tau = d / hb[k]
            for i in range(k, 12):
                A[i][j] = A[i][j] - tau * A[i][k]
    basis = []
    for c in range(4):
        y = [0.0] * 12
        y[8 + c] = 1.0
        for k in range(7, -1, -1):
            if hb[k] == 0.0:
                continue
            d = 0.0
            for i in range(k, 12):
                d += A[i][k] * y[i]
            tau = d / hb[k]
            for i in range(k, 12):
                y[i] = y[i] - tau * A[i][k]
        basis.append(canonical(y))
    return basis


def compute_pose(pws: np.ndarray, us: np.ndarray, fu: float, fv: float, uc: float, vc: float):
    """PnPsolver::compute_pose (:477-525) on n correspondences (pws n x 3, us n x 2, float64).  Returns (R 3x3, t 3, rep_error)."""
    n = len(pws)
    pws = np.asarray(pws, np.float64)
    us = np.asarray(us, np.float64)
    # choose_control_points (:375-409)
    c0 = list(_cumsum_last(pws) / n)
    PW0 = pws - np.array(c0)
    pp = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            pp[a][b] = pp[b][a] = float(_cumsum_last(PW0[:, a] * PW0[:, b]))
    lam, V = jacobi_eig(pp, 3)
    o = order_by_abs(lam, 3)
    cws = [c0]
    for i in range(1, 4):
        e = o[3 - i]                                        # descending |lambda|, as cvSVD orders dc
        u = canonical([V[0][e], V[1][e], V[2][e]])
        k = math.sqrt(abs(lam[e]) / n)
        cws.append([c0[j] + k * u[j] for j in range(3)])
    # compute_barycentric_coordinates (:411-434)
    CC = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
    ci = inv3(CC)
    d = pws - np.array(cws[0])
    al = np.empty((n, 4))
    for j in range(3):
        al[:, 1 + j] = ci[j][0] * d[:, 0] + ci[j][1] * d[:, 1] + ci[j][2] * d[:, 2]
    al[:, 0] = 1.0 - al[:, 1] - al[:, 2] - al[:, 3]
    # fill_M (:436-452) and the null space
    M = np.zeros((2 * n, 12))
    for i in range(4):
        M[0::2, 3 * i] = al[:, i] * fu
        M[0::2, 3 * i + 2] = al[:, i] * (uc - us[:, 0])
        M[1::2, 3 * i + 1] = al[:, i] * fv
        M[1::2, 3 * i + 2] = al[:, i] * (vc - us[:, 1])
    if n == 4:
        v = householder_null4([[float(M[r][a]) for r in range(8)] for a in range(12)])
    else:
        P = M[:, :, None] * M[:, None, :]
        mtm = _cumsum_last(P)
        lam, V = jacobi_eig([[float(mtm[a][b]) for b in range(12)] for a in range(12)], 12)
        o = order_by_abs(lam, 12)
        v = [canonical([V[k][o[i]] for k in range(12)]) for i in range(4)]
    L = _fill_L(v)
    rho = [_dist2(cws[0], cws[1]), _dist2(cws[0], cws[2]), _dist2(cws[0], cws[3]),
           _dist2(cws[1], cws[2]), _dist2(cws[1], cws[3]), _dist2(cws[2], cws[3])]
    best = None
    for betas in _betas(L, rho):
        # compute_R_and_t (:636-665)
        ccs = [[0.0] * 3 for _ in range(4)]
        for i in range(4):
            for j in range(4):
                for k in range(3):
                    ccs[j][k] += betas[i] * v[i][3 * j + k]
        pc0z = al[0, 0] * ccs[0][2] + al[0, 1] * ccs[1][2] + al[0, 2] * ccs[2][2] + al[0, 3] * ccs[3][2]
        if pc0z < 0.0:                                       # solve_for_sign: the first point's z only
            ccs = [[-x for x in r] for r in ccs]
        pcs = np.empty((n, 3))
        for j in range(3):
            pcs[:, j] = al[:, 0] * ccs[0][j] + al[:, 1] * ccs[1][j] + al[:, 2] * ccs[2][j] + al[:, 3] * ccs[3][j]
        # estimate_R_and_t (:569-627)
        pc0 = list(_cumsum_last(pcs) / n)
        pw0 = c0
        A = pcs - np.array(pc0)
        B = pws - np.array(pw0)
        abt = [[float(_cumsum_last(A[:, j] * B[:, c])) for c in range(3)] for j in range(3)]
        R = rotation_from_abt(abt)
        det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
               R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
        if det < 0:
            R[2] = [-x for x in R[2]]
        t = [pc0[i] - dot3(R[i], pw0) for i in range(3)]
        # reprojection_error (:546-567)
        Xc = R[0][0] * pws[:, 0] + R[0][1] * pws[:, 1] + R[0][2] * pws[:, 2] + t[0]
        Yc = R[1][0] * pws[:, 0] + R[1][1] * pws[:, 1] + R[1][2] * pws[:, 2] + t[1]
        with np.errstate(divide="ignore", invalid="ignore"):
            iz = 1.0 / (R[2][0] * pws[:, 0] + R[2][1] * pws[:, 1] + R[2][2] * pws[:, 2] + t[2])
            ue = uc + fu * Xc * iz
            ve = vc + fv * Yc * iz
            term = np.sqrt((us[:, 0] - ue) * (us[:, 0] - ue) + (us[:, 1] - ve) * (us[:, 1] - ve))
        err = float(_cumsum_last(term)) / n
        if best is None or err < best[2]:                    # rep_errors[k] < rep_errors[N]: ties keep the lower index
            best = (R, t, err)
    return np.array(best[0]), np.array(best[1]), best[2]


def check_inliers(R, t, xyz, uv, max_error, fu, fv, uc, vc):
    """PnPsolver::CheckInliers (:308-340) with its float / double mix: Xc, Yc, invZc float; ue, ve double; distX, distY, error2
    float; error2 < mvMaxError[i] (float).  Returns (mask, count, error2 as float64 of the float)."""
    R = np.asarray(R, np.float64)
    x = xyz[:, 0].astype(np.float64); y = xyz[:, 1].astype(np.float64); z = xyz[:, 2].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Xc = (R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + t[0]).astype(F32)
        Yc = (R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + t[1]).astype(F32)
        invZc = (1.0 / (R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + t[2])).astype(F32)
        ue = uc + fu * Xc.astype(np.float64) * invZc.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * invZc.astype(np.float64)
        dX = (uv[:, 0].astype(np.float64) - ue).astype(F32)
        dY = (uv[:, 1].astype(np.float64) - ve).astype(F32)
        e2 = dX * dX + dY * dY
    mask = e2 < max_error
    return mask, int(mask.sum()), e2


def tcw_float(R, t) -> np.ndarray:
    """Rcw / tcw convertTo(CV_32F) into a 3x4 (row-major) float pose."""
    T = np.empty((3, 4), F32)
    T[:, :3] = np.asarray(R, np.float64).astype(F32)
    T[:, 3] = np.asarray(t, np.float64).astype(F32)
    return T


# ------------------------------------------------------------------ PnPsolver
def ransac_constants(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5):
    """SetRansacParameters (:121-157): (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon)."""
    eps = F32(epsilon)
    n_min = int(F32(N) * eps)                                # int nMinInliers = N*mRansacEpsilon (float product, truncated)
    if n_min < min_inliers:
        n_min = min_inliers
    if n_min < min_set:
        n_min = min_set
    if N > 0 and eps < F32(n_min) / F32(N):
        eps = F32(n_min) / F32(N)
    if n_min == N:
        n_it = 1
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.log(np.float64(1 - probability)) / np.log(np.float64(1 - math.pow(float(eps), 3)))
        # N < minInliers makes epsilon > 1 and the quotient NaN; the (int) of it is INT_MIN on x86-64, so the budget is 1 (and
        # iterate() never draws for such a solver anyway)
        n_it = math.ceil(q) if np.isfinite(q) else -(1 << 31)
    return n_min, max(1, min(n_it, max_iterations)), eps


class PnPsolverRef:
    """PnPsolver with its state across iterate() calls.  `hyps` collects (count, R, t) of every hypothesis of the last call."""

    def __init__(self, xyz, uv, sigma2, kp_index, n_keypoints, fx, fy, cx, cy, seed, params=(0.99, 10, 300, 4, 0.5, 5.991)):
        self.xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
        self.uv = np.ascontiguousarray(uv, F32).reshape(-1, 2)
        self.sigma2 = np.ascontiguousarray(sigma2, F32)
        self.kp = np.ascontiguousarray(kp_index, np.int64)
        self.n_kp = int(n_keypoints)
        self.fu, self.fv, self.uc, self.vc = (float(F32(a)) for a in (fx, fy, cx, cy))
        self.N = len(self.xyz)
        self.rng = GlibcRand(seed)
        self.n_iterations = 0
        self.best_inliers = 0
        self.best_mask = None
        self.best_Tcw = None
        self.refine_sizes = []                                   # size of every Refine's set, over all calls
        self.set_ransac_parameters(*params)

    def set_ransac_parameters(self, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991):
        assert min_set == 4
        self.min_inliers, self.max_its, self.eps = ransac_constants(self.N, probability, min_inliers, max_iterations, min_set, epsilon)
        self.max_error = self.sigma2 * F32(th2)

    def _check(self, R, t):
        return check_inliers(R, t, self.xyz, self.uv, self.max_error, self.fu, self.fv, self.uc, self.vc)

    def sample(self):
        return draw_set(self.rng, self.N, 4)

    def hypothesis(self, idx):
        return compute_pose(self.xyz[idx].astype(np.float64), self.uv[idx].astype(np.float64), self.fu, self.fv, self.uc, self.vc)

    def refine(self):
        sel = np.flatnonzero(self.best_mask)
        self.refine_sizes.append(len(sel))
        R, t, _ = compute_pose(self.xyz[sel].astype(np.float64), self.uv[sel].astype(np.float64), self.fu, self.fv, self.uc, self.vc)
        mask, cnt, _ = self._check(R, t)
        self.refined = (R, t, mask, cnt)
        return cnt > self.min_inliers

    def _flags(self, mask):
        f = np.zeros(self.n_kp, np.uint8)
        f[self.kp[mask]] = 1
        return f

    def iterate(self, n):
        """Returns dict(Tcw (3x4 float32) or None, no_more, inliers (uint8[n_keypoints]), n_inliers)."""
        self.hyps = []
        self.refines = []
        out = dict(Tcw=None, no_more=False, inliers=np.zeros(self.n_kp, np.uint8), n_inliers=0)
        if self.N < self.min_inliers:
            out["no_more"] = True
            return out
        cur = 0
        while self.n_iterations < self.max_its or cur < n:
            cur += 1
            self.n_iterations += 1
            R, t, _ = self.hypothesis(self.sample())
            mask, cnt, _ = self._check(R, t)
            self.hyps.append((cnt, R, t))
            if cnt >= self.min_inliers:
                if cnt > self.best_inliers:
                    self.best_mask = mask
                    self.best_inliers = cnt
                    self.best_Tcw = tcw_float(R, t)
                ok = self.refine()
                self.refines.append(ok)
                if ok:
                    R2, t2, m2, c2 = self.refined
                    out.update(Tcw=tcw_float(R2, t2), n_inliers=c2, inliers=self._flags(m2))
                    return out
        if self.n_iterations >= self.max_its:
            out["no_more"] = True
            if self.best_inliers >= self.min_inliers:
                out.update(Tcw=self.best_Tcw.copy(), n_inliers=self.best_inliers, inliers=self._flags(self.best_mask))
        return out

    def find(self):
        return self.iterate(self.max_its)


def relocalization_rounds(solvers, active=None, n=5, max_rounds=1000):
    """Tracking::Relocalization's loop (Tracking.cc:1894-1916) without the PoseOptimization part: iterate(5) on every candidate
    not yet discarded; a candidate with no_more is discarded.  Returns the per-round outputs (list of lists, None = skipped)."""
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


def _rot(rng, scale):
    w = rng.normal(0, scale, 3)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def make_scene(seed, n, inlier_ratio=0.6, noise=0.5, variant=None, n_keypoints=None, cam=KITTI):
    """One relocalisation candidate: N correspondences of a KITTI-like stereo frame.  Inliers project the true pose with
    Gaussian pixel noise (sigma `noise` times the octave scale); outliers are uniform in the image.  Variants: 'coplanar' (world
    points on one plane), 'behind' (a quarter of the points behind the camera), 'duplicate' (a third of the points repeated),
    'exact' (no noise, no outliers), 'collapsed' (every world point the same: the EPnP quantities turn to NaN)."""
    rng = np.random.default_rng(seed)
    R = _rot(rng, 0.3)
    t = rng.normal(0, 2.0, 3)
    depth = rng.uniform(4.0, 40.0, n)
    u0 = rng.uniform(0, cam["w"], n); v0 = rng.uniform(0, cam["h"], n)
    Xc = np.stack([(u0 - cam["cx"]) / cam["fx"] * depth, (v0 - cam["cy"]) / cam["fy"] * depth, depth], 1)
    if variant == "coplanar":
        nrm = np.array([0.1, -0.2, 1.0]); nrm /= np.linalg.norm(nrm)
        d0 = 15.0
        dirs = Xc / depth[:, None]
        s = d0 / (dirs @ nrm)
        Xc = dirs * s[:, None]
    if variant == "behind":
        k = n // 4
        Xc[:k, 2] *= -1.0
    Xw = (Xc - t) @ R                                            # Xc = R Xw + t
    if variant == "collapsed":
        Xw[:] = Xw[0]
    if variant == "duplicate":
        k = n // 3
        src = rng.integers(0, n - k, k)
        Xw[n - k:] = Xw[src]
    level = rng.integers(0, 8, n)
    sigma2 = np.array([np.float32(np.float32(1.44) ** np.float32(l)) for l in level], F32)
    Xc2 = Xw @ R.T + t
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([cam["fx"] * Xc2[:, 0] / Xc2[:, 2] + cam["cx"], cam["fy"] * Xc2[:, 1] / Xc2[:, 2] + cam["cy"]], 1)
    if variant != "exact":
        uv += rng.normal(0, noise, (n, 2)) * np.sqrt(sigma2)[:, None]
        out = rng.random(n) >= inlier_ratio
        uv[out] = np.stack([rng.uniform(0, cam["w"], out.sum()), rng.uniform(0, cam["h"], out.sum())], 1)
    else:
        out = np.zeros(n, bool)
    bad = ~np.isfinite(uv).all(1)
    uv[bad] = 0.0
    nk = n_keypoints if n_keypoints is not None else min(n + n // 2, 8192)
    kp = np.sort(rng.choice(nk, n, replace=False)).astype(np.int32)
    return dict(xyz=Xw.astype(F32), uv=uv.astype(F32), sigma2=sigma2, kp_index=kp, n_keypoints=nk,
                fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], seed=int(rng.integers(0, 1 << 32)), R=R, t=t,
                outlier=out)


def solver_from_scene(sc, params=(0.99, 10, 300, 4, 0.5, 5.991)):
    return PnPsolverRef(sc["xyz"], sc["uv"], sc["sigma2"], sc["kp_index"], sc["n_keypoints"], sc["fx"], sc["fy"], sc["cx"], sc["cy"],
                        sc["seed"], params)
