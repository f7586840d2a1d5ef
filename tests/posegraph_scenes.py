"""Essential graphs shaped like Optimizer::OptimizeEssentialGraph builds them (src/Optimizer.cc:1391-1585), for the pose-graph tests.

synth.make_essential_graph is a band: a chain, covisibility a few keyframes back and one loop edge onto keyframe 0, the only fixed
vertex, so its loop edge adds nothing off the diagonal and the tile Cholesky of the system has no fill.  The reference's graphs are
not bands: pLoopKF (the only fixed vertex) sits in the middle of the id range, LoopConnections join every keyframe around the
current one to every keyframe around pLoopKF (both ends free), loop edges of earlier closures and covisibility across earlier loops
join free keyframes far apart, and a re-parented spanning-tree edge can point to a newer keyframe (edge_i < edge_j).

Conventions are synth's: Sji = Sjw * Swi; normal edges are measured on the NonCorrected poses, LoopConnections on the Corrected ones;
meta carries the ground truth.  `tile_pattern` / `symbolic_cholesky` are the witness: a tile-level symbolic factorisation written from
the definition (eliminating tile column k joins every pair of its non-zero rows), independent of the host's elimination-tree merge."""
import dataclasses

import numpy as np
from scipy.spatial.transform import Rotation

from lld_slam_amd.host import EssentialGraph


def _rodrigues(w):
    return Rotation.from_rotvec(w).as_matrix()


def _mat(S):
    M = np.eye(4); M[:3, :3] = S[7] * Rotation.from_quat(S[:4]).as_matrix(); M[:3, 3] = S[4:7]; return M


def _from_mat(M):
    s = np.cbrt(np.linalg.det(M[:3, :3]))
    return np.concatenate([Rotation.from_matrix(M[:3, :3] / s).as_quat(), M[:3, 3], [s]])


def _to_sim3(T):
    return np.concatenate([Rotation.from_matrix(T[:3, :3]).as_quat(), T[:3, 3], [1.0]])


def make_loop_scene(seed=0, n_kf=120, laps=1, loop_kf=None, cur_conn=6, loop_conn=6, extra_fixed=(), earlier_loops=0, long_covis=0,
                    reparent_frac=0.0, covis=3, drift=(0.002, 0.03), n_corrected=None):
    """A trajectory of `laps` laps of a circle (one loop closure per lap after the first is what `earlier_loops` stands for), odometry
    that drifts, and the graph of the current closure: the current keyframe is the last one, pLoopKF = `loop_kf` is fixed (plus
    `extra_fixed`).  ComputeSim3 found the current keyframe's pose relative to pLoopKF's (drifted) pose: that is its Corrected pose,
    and the last `n_corrected` keyframes get the same correction (CorrectLoop).  Edges, in the reference's order:
      LoopConnections: the last `cur_conn` keyframes x the `loop_conn` keyframes around pLoopKF, on the Corrected poses;
      spanning tree k -> k-1 (a fraction `reparent_frac` written the other way round, as after SetBadFlag re-parents a child);
      `earlier_loops` loop edges of earlier closures between keyframes far apart (measured on the ground truth: those loops were
      closed); covisibility k -> k-2 .. k-covis and `long_covis` covisibility edges across the map, on the NonCorrected poses."""
    rng = np.random.default_rng(0x9E5C0000 + seed)
    loop_kf = n_kf // 3 if loop_kf is None else loop_kf
    n_corrected = max(cur_conn, 6) if n_corrected is None else n_corrected
    ang = np.linspace(0, 2 * np.pi * laps, n_kf, endpoint=False)
    lift = 0.5 * np.arange(n_kf) / max(n_kf, 1)                                   # the laps do not coincide
    Rw = [Rotation.from_euler("y", -a).as_matrix() for a in ang]
    tw = np.stack([40 * np.cos(ang), 0.3 * np.sin(3 * ang) + lift, 40 * np.sin(ang)], 1)
    Tgt = [np.block([[Rw[k].T, (-Rw[k].T @ tw[k])[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]) for k in range(n_kf)]   # Tiw
    Td = [Tgt[0]]
    for k in range(1, n_kf):
        rel = Tgt[k] @ np.linalg.inv(Tgt[k - 1])
        N = np.eye(4); N[:3, :3] = _rodrigues(rng.normal(0, drift[0], 3)); N[:3, 3] = rng.normal(0, drift[1], 3)
        Td.append(N @ rel @ Td[k - 1])
    non_corr = np.stack([_to_sim3(T) for T in Td])
    verts = non_corr.copy()
    cur = n_kf - 1
    corrected_cur = Tgt[cur] @ np.linalg.inv(Tgt[loop_kf]) @ Td[loop_kf]     # Scw = Scm * Smw, found against pLoopKF's own estimate
    for k in range(n_kf - n_corrected, n_kf):
        verts[k] = _from_mat(_mat(non_corr[k]) @ np.linalg.inv(_mat(non_corr[cur])) @ corrected_cur)
    ei, ej, meas = [], [], []

    def add(i, j, Si, Sj):                                                        # Sji = Sjw * Swi
        ei.append(i); ej.append(j); meas.append(_from_mat(_mat(Sj) @ np.linalg.inv(_mat(Si))))
    lo = max(0, loop_kf - loop_conn // 2)
    loop_side = [k for k in range(lo, min(n_kf - n_corrected, lo + loop_conn))]
    for i in range(n_kf - cur_conn, n_kf):                                        # LoopConnections
        for j in loop_side:
            add(i, j, verts[i], verts[j])
    far = []
    while len(far) < earlier_loops + long_covis:
        a, b = sorted(int(v) for v in rng.integers(0, n_kf - n_corrected, 2))
        if b - a > n_kf // 4 and (b, a) not in far: far.append((b, a))
    gt = np.stack([_to_sim3(T) for T in Tgt])
    for i in range(1, n_kf):
        if rng.random() < reparent_frac: add(i - 1, i, non_corr[i - 1], non_corr[i])   # re-parented: the parent is the newer one
        else: add(i, i - 1, non_corr[i], non_corr[i - 1])
        for (a, b) in far[:earlier_loops]:
            if a == i: add(a, b, gt[a], gt[b])                                    # old loop edge
        for d in range(2, covis + 1):
            if i - d >= 0: add(i, i - d, non_corr[i], non_corr[i - d])
        for (a, b) in far[earlier_loops:]:
            if a == i: add(a, b, non_corr[a], non_corr[b])                        # covisibility across an earlier loop
    fixed = np.zeros(n_kf, np.uint8); fixed[loop_kf] = 1
    for v in extra_fixed: fixed[v] = 1
    return EssentialGraph(sim3=verts, fixed=fixed, edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32), edge_sji=np.stack(meas),
                          meta=dict(gt=gt, drifted=non_corr, loop_kf=loop_kf, n_corrected=n_corrected))


# Named scenes, each aimed at one path of the tile Cholesky / the assembly (the witness tests check that each reaches it).
# (kwargs of make_loop_scene, bFixScale); every one <= 160 keyframes, so the oracle's dense LDL^T stays a few seconds.
SCENES = {
    # pLoopKF in the middle, a 6 x 6 LoopConnections block: fill tiles, rows with dozens of K tiles (second k0 pass of
    # pg_chol_col, every wavefront and every q), multi-workgroup back substitution
    "mid_loop": (dict(seed=1, n_kf=120, loop_kf=40), True),
    # the shape the reference builds after a long run: pLoopKF near the start, 8 x 9 LoopConnections, two earlier loop edges
    "many_to_many": (dict(seed=2, n_kf=150, loop_kf=24, cur_conn=8, loop_conn=9, earlier_loops=2), True),
    # three laps: earlier closures and covisibility across them, free scale
    "three_laps": (dict(seed=3, n_kf=150, laps=3, loop_kf=60, earlier_loops=4, long_covis=6), False),
    # a third of the spanning tree re-parented to the newer keyframe: edges with edge_i < edge_j
    "reparented": (dict(seed=4, n_kf=120, loop_kf=60, reparent_frac=0.35, long_covis=3), True),
    # several fixed vertices: keyframe 0, keyframe 17 (the 16 unknowns before it end on the tile boundary 112), one late one
    "fixed_many": (dict(seed=5, n_kf=120, loop_kf=50, extra_fixed=(0, 17, 90)), True),
    # a short loop onto a fixed vertex near the end and a free keyframe 0: small, free scale
    "short_free": (dict(seed=6, n_kf=48, loop_kf=30, cur_conn=3, loop_conn=4, earlier_loops=1, covis=2), False),
}


def scene(name):
    kw, fix = SCENES[name]
    return make_loop_scene(**kw), fix


def make_padding_graph(nu, seed=0):
    """nu free keyframes plus a fixed first one: a chain with covisibility, a loop edge between the first and the last free
    keyframe (nu >= 3), and the last one Corrected.  7 nu mod 16 runs through all 16 residues for nu = 1..16."""
    n = nu + 1
    gr = make_loop_scene(seed=1000 + nu, n_kf=n, loop_kf=0, cur_conn=1, loop_conn=1, covis=min(3, n - 1), n_corrected=1)
    if nu >= 3:                                                   # a loop edge between free vertices, on the ground truth
        gt = gr.meta["gt"]
        gr = dataclasses.replace(gr, edge_i=np.append(gr.edge_i, np.int32(nu)), edge_j=np.append(gr.edge_j, np.int32(1)),
                                 edge_sji=np.vstack([gr.edge_sji, _from_mat(_mat(gt[1]) @ np.linalg.inv(_mat(gt[nu])))]))
    return gr


PADDING_SIZES = list(range(1, 18)) + [32]


def reverse_edges(gr, seed=0, frac=0.5):
    """The same graph with a random `frac` of its edges written the other way round: (i, j, Sji) -> (j, i, Sji^-1)."""
    rng = np.random.default_rng(seed)
    flip = rng.random(len(gr.edge_i)) < frac
    ei = np.where(flip, gr.edge_j, gr.edge_i).astype(np.int32); ej = np.where(flip, gr.edge_i, gr.edge_j).astype(np.int32)
    sji = np.array([_from_mat(np.linalg.inv(_mat(s))) if f else s for s, f in zip(gr.edge_sji, flip)])
    return dataclasses.replace(gr, edge_i=ei, edge_j=ej, edge_sji=sji), flip


def relative_error(sim3, gt, ref):
    """Per keyframe: distance between the camera centre of keyframe k expressed in keyframe `ref`'s frame and the ground truth's
    (the gauge is pinned at the fixed pLoopKF; scale divided out)."""
    def centres(S):
        Ms = [_mat(s) for s in S]
        Mr = Ms[ref]
        return np.array([(Mr @ np.linalg.inv(M))[:3, 3] / np.cbrt(np.linalg.det((Mr @ np.linalg.inv(M))[:3, :3])) for M in Ms])
    return np.linalg.norm(centres(sim3) - centres(gt), axis=1)


# ---------------------------------------------------------------- the witness: tile pattern of H and of its Cholesky factor

def unknown_index(gr):
    fixed = np.asarray(gr.fixed).astype(bool)
    hidx = np.full(len(fixed), -1); hidx[~fixed] = np.arange(int((~fixed).sum()))
    return hidx


def tile_pattern(gr, ts=16):
    """Boolean lower-triangular NT x NT pattern of H (7 x 7 blocks of the unknowns on 16 x 16 tiles): every diagonal block and
    the off-diagonal block of every edge between two different unknowns."""
    hidx = unknown_index(gr); nu = int((hidx >= 0).sum())
    NT = (7 * nu + ts - 1) // ts
    P = np.zeros((NT, NT), bool)

    def mark(a, b):
        ra = np.arange(7 * a, 7 * a + 7) // ts; rb = np.arange(7 * b, 7 * b + 7) // ts
        for r in np.unique(ra):
            for c in np.unique(rb):
                P[max(r, c), min(r, c)] = True
    for u in range(nu): mark(u, u)
    for i, j in zip(gr.edge_i, gr.edge_j):
        a, b = hidx[i], hidx[j]
        if a >= 0 and b >= 0 and a != b: mark(a, b)
    return P


def symbolic_cholesky(P):
    """Tile pattern of L for A with lower pattern P: eliminating column k makes L_rk L_sk^T non-zero for every pair of non-zero
    rows r, s > k of column k (the definition; no elimination tree)."""
    L = np.tril(P).copy()
    for k in range(L.shape[0]):
        rows = np.nonzero(L[k + 1:, k])[0] + k + 1
        if rows.size > 1:
            L[np.ix_(rows, rows)] |= np.tril(np.ones((rows.size, rows.size), bool))
    return L


def witness(gr):
    """What the dense path of lld_optimize_essential_graph meets on this graph."""
    P = tile_pattern(gr); L = symbolic_cholesky(P)
    off = np.tril(L, -1)
    k_per_row = off.sum(1)                                         # nK of pg_chol_col / pg_chol_back for tile row J
    hidx = unknown_index(gr); fixed = np.nonzero(np.asarray(gr.fixed))[0]
    return dict(NT=P.shape[0], fill=int((L & ~P).sum()), max_k=int(k_per_row.max()) if k_per_row.size else 0,
                rows_k4=int((k_per_row >= 4).sum()), rows_k17=int((k_per_row >= 17).sum()),
                back_groups=int(((1 + k_per_row + 3) // 4).max()) if k_per_row.size else 0,
                i_lt_j=int((np.asarray(gr.edge_i) < np.asarray(gr.edge_j)).sum()),
                fixed=fixed.tolist(), free_edges=int(sum(hidx[i] >= 0 and hidx[j] >= 0 for i, j in zip(gr.edge_i, gr.edge_j))))
