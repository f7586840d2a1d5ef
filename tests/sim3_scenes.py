"""Deterministic candidates for Optimizer::OptimizeSim3 whose survivor counts are exact whatever the rounding.

Inliers are projections of the float-rounded points through the generating S12 with at most `noise` px of uniform noise per
coordinate (inverse sigma^2 = 1), so their chi2 stays <= 2 noise^2, far below any th2 used; outliers are moved 100-200 px in obs1
only (e12 fails), obs2 only (e21 fails) or both, so their chi2 is far above it.  g2oS12 starts at the generating transform: round 1
starts at the answer and which correspondences it drops is known in advance."""
import numpy as np
from scipy.spatial.transform import Rotation

from lld_slam_amd.host import Sim3Pair
from lld_slam_amd.synth import KITTI_CAM


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def make_exact_pair(seed=0, n=100, out12=0, out21=0, out_both=0, noise=0.45, scale=1.0, behind=0):
    """`out12` / `out21` / `out_both`: how many correspondences fail e12 only, e21 only, both (at random positions, listed in
    meta); `behind`: how many points lie at a finite negative depth (behind both cameras; consistent observations: inliers)."""
    rng = np.random.default_rng(0x5E3E0000 + seed)
    fx, fy, cx, cy, _ = [float(v) for v in KITTI_CAM]
    R = Rotation.from_rotvec(rng.normal(0, 0.15, 3)).as_matrix(); t = rng.normal(0, 0.6, 3); s = float(scale)
    X2 = np.stack([rng.uniform(-10, 10, n), rng.uniform(-3, 3, n), rng.uniform(8, 40, n)], 1)
    order = rng.permutation(n)
    back = order[:behind]
    X2[back, 2] = -X2[back, 2]
    p2c = _f32(X2)
    p1c = _f32(s * p2c @ R.T + t)

    def proj(X): return np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
    obs1 = proj(s * p2c @ R.T + t) + rng.uniform(-noise, noise, (n, 2))          # e12 = obs1 - proj(S12 X2)
    obs2 = proj((p1c - t) @ R / s) + rng.uniform(-noise, noise, (n, 2))           # e21 = obs2 - proj(S12^-1 X1)
    rest = order[behind:]
    k12, k21, kb = rest[:out12], rest[out12:out12 + out21], rest[out12 + out21:out12 + out21 + out_both]
    assert len(kb) == out_both, "more outliers than correspondences"

    def push(k):
        a = rng.uniform(0, 2 * np.pi, len(k)); r = rng.uniform(100, 200, len(k))
        return np.stack([r * np.cos(a), r * np.sin(a)], 1)
    obs1[np.concatenate([k12, kb])] += push(np.concatenate([k12, kb]))
    obs2[np.concatenate([k21, kb])] += push(np.concatenate([k21, kb]))
    bad = np.zeros(n, bool); bad[k12] = bad[k21] = bad[kb] = True
    K = (np.float32(fx), np.float32(fy), np.float32(cx), np.float32(cy))
    return Sim3Pair(K1=K, K2=K, s12_q=Rotation.from_matrix(R).as_quat(), s12_t=t.copy(), s12_s=s, p1c=p1c, p2c=p2c,
                    obs1=_f32(obs1), obs2=_f32(obs2), inv_sigma2_1=np.ones(n), inv_sigma2_2=np.ones(n),
                    meta=dict(bad=bad, out12=np.sort(k12), out21=np.sort(k21), out_both=np.sort(kb), behind=np.sort(back)))
