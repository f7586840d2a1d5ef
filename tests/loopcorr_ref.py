"""A numpy restatement of the three loops in which the loop-closing thread moves the map, written from src/LoopClosing.cc:440-518 and
:678-739, src/Optimizer.cc:1601-1653, src/KeyFrame.cc:78-92, src/Converter.cc:55-108 and Thirdparty/g2o/g2o/types/sim3.h, with the
numerics include/lld_amd.h states.  It does not import lld_slam_amd.

Everything is SEQUENTIAL, in the reference's loop order: correct_loop_literal interleaves SetPose with the point corrections as
:474-518 does, global_ba_literal is the queue walk of :679-702.  correct_loop_batched is the rule the device follows (owner = the
smallest rank, the camera centre chosen by rank); the tests hold it to the literal loop.

Doubles are Python floats combined one operation at a time (no `@`, no dot: BLAS may fuse); floats are np.float32 scalars, one
rounding per operation.  UpdateNormalAndDepth is tests/landmark_ref.py's."""
import numpy as np

import landmark_ref as LR

f32 = np.float32
MOVED, NORMAL_DEPTH = 1, 2


# ------------------------------------------------------------------ float cv::Mat forms (a pose is 12 float32: the rows of [R|t])
def centre_of(T):
    """Ow = -Rwc*tcw with Rwc = Rcw.t() (KeyFrame.cc:84-85): one product, double accumulation in index order, one rounding."""
    ow = np.zeros(3, f32)
    for i in range(3):
        s = float(T[i]) * float(T[3])
        s += float(T[4 + i]) * float(T[7])
        s += float(T[8 + i]) * float(T[11])
        ow[i] = -f32(s)
    return ow


def inverse_of(T):
    """Twc = [Rcw^T | Ow] (KeyFrame.cc:87-89)."""
    ow = centre_of(T)
    out = np.zeros(12, f32)
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = T[4 * j + i]
        out[4 * i + 3] = ow[i]
    return out


def mul44(A, B):
    """Two 4x4 float matrices with bottom rows (0, 0, 0, 1): every entry the four-term double sum in index order, rounded once."""
    C = np.zeros(12, f32)
    for i in range(3):
        for j in range(4):
            s = float(A[4 * i]) * float(B[j])
            s += float(A[4 * i + 1]) * float(B[4 + j])
            s += float(A[4 * i + 2]) * float(B[8 + j])
            s += float(A[4 * i + 3]) * (1.0 if j == 3 else 0.0)
            C[4 * i + j] = f32(s)
    return C


# ------------------------------------------------------------------ Eigen quaternions and g2o::Sim3, scalar by scalar.  Sim3 = (q[4] xyzw, t[3], s)
def quat_from_R(R):
    """Eigen's Quaterniond(Matrix3d): the trace branch, else the largest diagonal (ties keep the lower index)."""
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return [(R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t, w]
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = np.sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0)
    q = [0.0, 0.0, 0.0, 0.0]
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (R[k][j] - R[j][k]) * t
    q[j] = (R[j][i] + R[i][j]) * t
    q[k] = (R[k][i] + R[i][k]) * t
    return q


def quat_to_R(q):
    """Eigen's toRotationMatrix, applied to q as it is."""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def quat_rotate(q, v):
    """Eigen's q * v: v + w*(2 q.vec x v) + q.vec x (2 q.vec x v)."""
    qv = q[:3]
    uv = cross(qv, v)
    uv = [u + u for u in uv]
    c = cross(qv, uv)
    return [(v[i] + q[3] * uv[i]) + c[i] for i in range(3)]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def sim3_map(S, x):
    q, t, s = S
    r = quat_rotate(q, x)
    return [s * r[i] + t[i] for i in range(3)]                 # s*(r*xyz) + t (sim3.h:133-135)


def sim3_mul(a, b):
    """Sim3::operator* (sim3.h:264-272)."""
    r = quat_rotate(a[0], b[1])
    return (quat_mul(a[0], b[0]), [a[2] * r[i] + a[1][i] for i in range(3)], a[2] * b[2])


def sim3_inverse(S):
    """Sim3::inverse (sim3.h:222-224): Sim3(r.conjugate(), r.conjugate()*((-1./s)*t), 1./s)."""
    q, t, s = S
    c = [-q[0], -q[1], -q[2], q[3]]
    m = -1. / s
    return (c, quat_rotate(c, [m * t[i] for i in range(3)]), 1. / s)


def sim3_of_pose(T):
    """Sim3(toMatrix3d(R), toVector3d(t), 1.0) of a float pose."""
    R = [[float(T[4 * i + j]) for j in range(3)] for i in range(3)]
    return (quat_from_R(R), [float(T[3]), float(T[7]), float(T[11])], 1.0)


def se3_of_sim3(S):
    """toCvSE3(R(q), t*(1./s)): a reciprocal, then a product (LoopClosing.cc:506-512)."""
    q, t, s = S
    R = quat_to_R(q)
    inv = 1. / s
    T = np.zeros(12, f32)
    for i in range(3):
        for j in range(3):
            T[4 * i + j] = f32(R[i][j])
        T[4 * i + 3] = f32(t[i] * inv)
    return T


def cvmat_of_sim3(S):
    """Converter::toCvMat(Sim3) = toCvSE3(s*R, t) (Converter.cc:55-61)."""
    q, t, s = S
    R = quat_to_R(q)
    T = np.zeros(12, f32)
    for i in range(3):
        for j in range(3):
            T[4 * i + j] = f32(s * R[i][j])
        T[4 * i + 3] = f32(t[i])
    return T


def sim3_flat(S):
    return np.array(list(S[0]) + list(S[1]) + [S[2]], np.float64)


def sim3_unflat(a):
    return ([float(x) for x in a[:4]], [float(x) for x in a[4:7]], float(a[7]))


def correct_point(Siw, Swi, P):
    """Swi.map(Siw.map(P)) of a float point, rounded to float once (LoopClosing.cc:494-499)."""
    Q = sim3_map(Swi, sim3_map(Siw, [float(P[0]), float(P[1]), float(P[2])]))
    return np.array([f32(Q[0]), f32(Q[1]), f32(Q[2])], f32)


def _nd_scene(sc, pos, ow):
    return dict(obs_start=sc["obs_start"], obs_kf=sc["obs_kf"], kf_ow=ow, pos=pos, bad=sc["bad"], ref_kf=sc["ref_kf"],
                ref_level=sc["ref_level"], level_scale=sc["level_scale"], n_levels=len(sc["level_scale"]))


def _point_outputs(sc):
    n = len(sc["bad"])
    return dict(pos=np.array(sc["pos"], f32), normal=np.array(sc["normal"], f32), min_distance=np.array(sc["min_distance"], f32),
                max_distance=np.array(sc["max_distance"], f32), updated=np.zeros(n, np.uint8))


# ------------------------------------------------------------------ loop 1: LoopClosing::CorrectLoop :440-518
def loop_poses(sc):
    """:440-471 and the pose half of :506-514 per connected keyframe, in conn order."""
    conn, cur = sc["conn"], sc["cur"]
    Scw = sim3_unflat(sc["scw"])
    Twc = inverse_of(sc["kf_tcw"][conn[cur]])                  # :442
    corrected, non = [], []
    for r, k in enumerate(conn):
        Tiw = sc["kf_tcw"][k]
        if r != cur:
            Tic = mul44(Tiw, Twc)                              # :457
            corrected.append(sim3_mul(sim3_of_pose(Tic), Scw))  # :460-463
        else:
            corrected.append(Scw)                              # :441
        non.append(sim3_of_pose(Tiw))                          # :466-470
    tiw = np.array([se3_of_sim3(S) for S in corrected], f32).reshape(-1, 12)
    return dict(corrected=corrected, non=non, corrected_sim3=np.array([sim3_flat(S) for S in corrected]),
                non_corrected_sim3=np.array([sim3_flat(S) for S in non]), tiw_corrected=tiw,
                ow_corrected=np.array([centre_of(T) for T in tiw], f32).reshape(-1, 3),
                scw_f32=np.array([cvmat_of_sim3(S) for S in corrected], f32).reshape(-1, 12))


def correct_loop_literal(sc):
    """The loop of :474-518 as written: per connected keyframe its points, then its SetPose."""
    K = loop_poses(sc)
    out = _point_outputs(sc)
    n = len(sc["bad"])
    out["corrected_by"] = np.full(n, -1, np.int32)
    ow = np.array([centre_of(T) for T in sc["kf_tcw"]], f32).reshape(-1, 3)      # GetCameraCenter() of every keyframe on entry
    already = np.array(sc["already"], bool)
    for r, k in enumerate(sc["conn"]):
        Swi = sim3_inverse(K["corrected"][r])                  # :478
        for e in range(sc["kf_start"][r], sc["kf_start"][r + 1]):
            p = sc["kf_point"][e]
            if sc["bad"][p] or already[p]:                     # :488-491
                continue
            out["pos"][p] = correct_point(K["non"][r], Swi, out["pos"][p])
            already[p] = True                                  # mnCorrectedByKF = mpCurrentKF->mnId
            out["corrected_by"][p] = r
            out["updated"][p] |= MOVED
            nd = LR.normal_depth(_nd_scene(sc, out["pos"], ow), p)               # :502, with the centres as they are NOW
            if nd is not None:
                out["normal"][p], out["min_distance"][p], out["max_distance"][p] = nd
                out["updated"][p] |= NORMAL_DEPTH
        ow[k] = K["ow_corrected"][r]                           # SetPose :514
    out.update({q: K[q] for q in ("corrected_sim3", "non_corrected_sim3", "tiw_corrected", "ow_corrected", "scw_f32")})
    return out


def owners(sc):
    """The first rank whose list holds the point, bad and already-corrected points skipped; -1 for none."""
    own = np.full(len(sc["bad"]), -1, np.int32)
    for r in range(len(sc["conn"]) - 1, -1, -1):
        for e in range(sc["kf_start"][r], sc["kf_start"][r + 1]):
            p = sc["kf_point"][e]
            if not sc["bad"][p] and not sc["already"][p]:
                own[p] = r
    return own


def loop_normals(sc, own, pos, ow_corrected):
    """UpdateNormalAndDepth by the rank rule on GIVEN positions and corrected centres: a point owned by rank k reads the corrected
    centre of a keyframe whose rank is strictly below k, the centre on entry otherwise.  -> (normal, min, max, did)."""
    n = len(sc["bad"])
    normal = np.array(sc["normal"], f32); mn = np.array(sc["min_distance"], f32); mx = np.array(sc["max_distance"], f32)
    did = np.zeros(n, bool)
    ow_old = np.array([centre_of(T) for T in sc["kf_tcw"]], f32).reshape(-1, 3)
    cache = {}
    for p in range(n):
        k = int(own[p])
        if k < 0:
            continue
        if k not in cache:
            ow = ow_old.copy()
            for r in range(k):
                ow[sc["conn"][r]] = ow_corrected[r]
            cache[k] = ow
        nd = LR.normal_depth(_nd_scene(sc, pos, cache[k]), p)
        if nd is not None:
            normal[p], mn[p], mx[p] = nd
            did[p] = True
    return normal, mn, mx, did


def correct_loop_batched(sc):
    """The device's rule: the poses, then the owners, then every position, then every normal by rank."""
    K = loop_poses(sc)
    out = _point_outputs(sc)
    own = owners(sc)
    for p in np.flatnonzero(own >= 0):
        r = own[p]
        out["pos"][p] = correct_point(K["non"][r], sim3_inverse(K["corrected"][r]), sc["pos"][p])
        out["updated"][p] |= MOVED
    out["normal"], out["min_distance"], out["max_distance"], did = loop_normals(sc, own, out["pos"], K["ow_corrected"])
    out["updated"][did] |= NORMAL_DEPTH
    out["corrected_by"] = own
    out.update({q: K[q] for q in ("corrected_sim3", "non_corrected_sim3", "tiw_corrected", "ow_corrected", "scw_f32")})
    return out


# ------------------------------------------------------------------ loop 2: Optimizer.cc:1601-1653
def graph_normals(sc, pos, ow):
    """UpdateNormalAndDepth of every point that is not bad on GIVEN positions and centres (all new, :1652)."""
    n = len(sc["bad"])
    normal = np.array(sc["normal"], f32); mn = np.array(sc["min_distance"], f32); mx = np.array(sc["max_distance"], f32)
    did = np.zeros(n, bool)
    S = _nd_scene(sc, pos, ow)
    for p in range(n):
        nd = LR.normal_depth(S, p)                             # returns None for a bad point or one without observations
        if nd is not None:
            normal[p], mn[p], mx[p] = nd
            did[p] = True
    return normal, mn, mx, did


def essential_graph_literal(sc):
    n_kf = len(sc["sim3_after"])
    after = [sim3_unflat(a) for a in sc["sim3_after"]]
    swc = [sim3_inverse(S) for S in after]                     # vCorrectedSwc (:1610)
    tiw = np.array([se3_of_sim3(S) for S in after], f32).reshape(n_kf, 12)       # :1611-1617
    ow = np.array([centre_of(T) for T in tiw], f32).reshape(n_kf, 3)             # SetPose :1619
    out = _point_outputs(sc)
    for p in range(len(sc["bad"])):
        if sc["bad"][p]:
            continue
        r = sc["corr_kf"][p]
        out["pos"][p] = correct_point(sim3_unflat(sc["sim3_before"][r]), swc[r], out["pos"][p])   # :1642-1650
        out["updated"][p] |= MOVED
        nd = LR.normal_depth(_nd_scene(sc, out["pos"], ow), p)                   # :1652
        if nd is not None:
            out["normal"][p], out["min_distance"][p], out["max_distance"][p] = nd
            out["updated"][p] |= NORMAL_DEPTH
    out.update(tiw=tiw, ow=ow)
    return out


# ------------------------------------------------------------------ loop 3: LoopClosing.cc:678-739
def gba_point(Tb, Tn, ow_new, P):
    """Xc = Rcw_before*P + tcw_before (the product rounded, then the float sum); P' = Rwc_new*Xc + Ow_new (:728-737)."""
    Xc = np.zeros(3, f32)
    for i in range(3):
        s = float(Tb[4 * i]) * float(P[0])
        s += float(Tb[4 * i + 1]) * float(P[1])
        s += float(Tb[4 * i + 2]) * float(P[2])
        Xc[i] = f32(s) + Tb[4 * i + 3]
    out = np.zeros(3, f32)
    for i in range(3):
        s = float(Tn[i]) * float(Xc[0])
        s += float(Tn[4 + i]) * float(Xc[1])
        s += float(Tn[8 + i]) * float(Xc[2])
        out[i] = f32(s) + ow_new[i]
    return out


def global_ba_literal(sc):
    """The queue walk of :679-702 on mutable keyframe state, then the point loop of :705-739."""
    n_kf = len(sc["parent"])
    tcw = np.array(sc["kf_tcw"], f32).reshape(n_kf, 12)        # Tcw, updated by SetPose
    twc = np.array([inverse_of(T) for T in tcw], f32)          # Twc, updated by SetPose
    gba = np.array(sc["kf_tcw_gba"], f32).reshape(n_kf, 12)    # mTcwGBA
    in_gba = np.array(sc["kf_in_gba"], bool)                   # mnBAGlobalForKF == nLoopKF
    before = np.array(tcw)                                     # mTcwBefGBA, meaningful where visited
    visited = np.zeros(n_kf, np.uint8)
    childs = [[c for c in range(n_kf) if sc["parent"][c] == k] for k in range(n_kf)]     # std::set<KeyFrame*>: pointer order
    queue = list(sc["origins"])
    while queue:
        k = queue[0]
        Twc = twc[k].copy()                                    # :685
        for c in childs[k]:
            if not in_gba[c]:
                Tchildc = mul44(tcw[c], Twc)                   # :691
                gba[c] = mul44(Tchildc, gba[k])                # :692
                in_gba[c] = True
            queue.append(c)
        before[k] = tcw[k]                                     # :699
        tcw[k] = gba[k]                                        # SetPose :700
        twc[k] = inverse_of(tcw[k])
        visited[k] = 1
        queue.pop(0)
    n = len(sc["bad"])
    pos = np.array(sc["pos"], f32).reshape(n, 3)
    moved = np.zeros(n, np.uint8)
    for p in range(n):
        if sc["bad"][p]:
            continue
        if sc["in_gba"][p]:
            pos[p] = sc["pos_gba"][p]                          # :717
            moved[p] = 1
            continue
        r = sc["ref_kf"][p]
        if not in_gba[r]:                                      # :724-725
            continue
        pos[p] = gba_point(before[r], tcw[r], twc[r][[3, 7, 11]], pos[p])
        moved[p] = 2
    ow_new = np.array([twc[k][[3, 7, 11]] for k in range(n_kf)], f32)
    return dict(visited=visited, tcw_new=tcw, tcw_before=before, ow_new=ow_new, pos=pos, moved=moved)


# ------------------------------------------------------------------ comparisons
def ulp_steps(a, b):
    """How many representable floats apart two float32 arrays are, element by element (finite values)."""
    def key(x):
        i = np.ascontiguousarray(x, f32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def bits_equal(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
