"""TEST INFRASTRUCTURE ONLY: scenes for Tracking::TrackReferenceKeyFrame on the device-resident chain (lld_frame_track_reference_keyframe).

A scene is a synth.make_tracking_scene world (frame, camera, local map, lines) plus a small seeded vocabulary (bow_ref.make_vocab) and a
reference keyframe: a share of its keypoints are bit-flipped copies of frame descriptors whose MapPoint sits at the scene's world position
of that keypoint (ids = the local map's, so TrackLocalMap meets the points the discard marked), the rest are unrelated.  The keyframe's
FeatureVector is bow_ref's transform of its descriptors.  Shapes are the smallest at which the matcher can still go wrong: a few hundred
keypoints over 16, 2 or 1 vocabulary nodes (in-node occupancy, nodes of more than 64 features, nothing in common, nothing valid, nothing at all)."""
from __future__ import annotations

import functools

import numpy as np

import bow_ref
from lld_slam_amd import orb_search, synth

NAMES = ("main", "chunks", "deep_levelsup", "disjoint_nodes", "kf_all_null", "kf_empty", "duplicates", "rotation_outliers", "failure_exit", "weak_pose")


def flip_bits(rng, desc, n_bits):
    """Every row of [n, 8] u32 with exactly n_bits distinct random bits flipped."""
    out = np.array(desc, np.uint32, copy=True).reshape(-1, 8)
    for r in range(out.shape[0]):
        for b in rng.choice(256, n_bits, replace=False):
            out[r, b // 32] ^= np.uint32(1 << int(b % 32))
    return out


def make_keyframe(sc, rng, n_kf, related_frac, null_frac=0.1, rot_outlier_frac=0.0, flips=(2, 9), no_obs_frac=0.1):
    """mpReferenceKF against the scene's frame: `related_frac` of its keypoints copy the descriptor of the keypoint a local MapPoint came from
    (distinct keypoints), rotated by ten degrees; the others are random descriptors with a MapPoint somewhere else.  null_frac of all have no
    (or a bad) MapPoint."""
    F = sc["frame"]; mp = sc["map_points"]
    n_rel = int(round(n_kf * related_frac))
    src_all = np.asarray(mp["src"])
    _, first = np.unique(src_all, return_index=True)                       # one MapPoint per frame keypoint
    pick = np.sort(rng.permutation(first)[:n_rel])
    n_rel = len(pick)
    src = src_all[pick]
    desc = np.empty((n_kf, 8), np.uint32)
    for i in range(n_rel):
        desc[i] = flip_bits(rng, F.desc[src[i]][None], int(rng.integers(flips[0], flips[1])))[0]
    desc[n_rel:] = rng.integers(0, 1 << 32, (n_kf - n_rel, 8), dtype=np.uint64).astype(np.uint32)
    angle = rng.uniform(0, 360, n_kf).astype(np.float32)
    angle[:n_rel] = np.mod(F.angle[src] + 10.0 + rng.normal(0, 3.0, n_rel), 360.0).astype(np.float32)
    out_rot = np.nonzero(rng.random(n_rel) < rot_outlier_frac)[0]
    angle[out_rot] = np.mod(F.angle[src[out_rot]] + rng.uniform(60, 300, len(out_rot)), 360.0).astype(np.float32)
    point_id = np.empty(n_kf, np.int32); world = np.empty((n_kf, 3), np.float32); obs = np.ones(n_kf, np.uint8)
    point_id[:n_rel] = np.asarray(sc["map_ids"])[pick]; world[:n_rel] = np.asarray(mp["world_pos"], np.float32)[pick]
    obs[:n_rel] = np.asarray(mp["has_obs"], np.uint8)[pick]
    point_id[n_rel:] = len(sc["map_ids"]) + np.arange(n_kf - n_rel); world[n_rel:] = rng.normal(0, 20.0, (n_kf - n_rel, 3)).astype(np.float32)
    obs[rng.random(n_kf) < no_obs_frac] = 0
    order = rng.permutation(n_kf)                                           # related and unrelated keypoints interleaved
    kf = dict(desc=desc[order], angle=angle[order], point_id=point_id[order], world_pos=world[order], has_obs=obs[order])
    kf["point_id"][rng.random(n_kf) < null_frac] = -1
    kf["src"] = np.concatenate([src, np.full(n_kf - n_rel, -1)])[order].astype(np.int32)   # the frame keypoint each was copied from (scene bookkeeping)
    return kf


def keyframe_frame(kf) -> orb_search.Frame:
    """The keyframe as the oracle's Frame (SearchByBoW reads descriptors and angles only)."""
    n = len(kf["angle"])
    return orb_search.Frame(desc=np.asarray(kf["desc"], np.uint32).reshape(-1, 8), xy=np.zeros((n, 2), np.float32), octave=np.zeros(n, np.int32),
                            uright=np.full(n, -1.0, np.float32), angle=np.asarray(kf["angle"], np.float32)).normalise()


def add_feature_vector(kf, tree, levelsup):
    fv = bow_ref.transform(tree, np.asarray(kf["desc"], np.uint32).reshape(-1, 8), levelsup)
    kf.update(node=fv["node"], node_start=fv["node_start"], feature=fv["feature"])
    return kf


@functools.lru_cache(maxsize=None)
def make_scene(name: str) -> dict:
    """dict(sc, vocab, levelsup, kf, Tcw_last, [contest]).  Cached: treat as read-only."""
    assert name in NAMES, name
    # deep_levelsup is the main scene's world, keyframe and vocabulary with nothing but levelsup changed: only the node structure differs
    seed = 300 + NAMES.index("main" if name == "deep_levelsup" else name)
    rng = np.random.default_rng(0xB0F + seed)
    k, L, levelsup = 4, 3, 1
    n_kf, related, kw = 300, 0.6, {}
    if name == "chunks": k, L = 2, 2
    if name == "deep_levelsup": levelsup = 3
    if name == "rotation_outliers": kw["rot_outlier_frac"] = 0.3
    if name == "failure_exit": n_kf, related = 60, 0.2
    if name == "weak_pose": kw["no_obs_frac"] = 0.97
    if name == "kf_empty": n_kf = 0
    sc = synth.make_tracking_scene(seed, n_kp=300, n_map=420, n_last=60, n_lines=40, n_map_lines=40, n_last_lines=16)
    F = sc["frame"]
    contest = None
    if name == "duplicates":
        # keypoints b = a with three bits flipped, for a few a: near-duplicates that fall under one node
        a_all = rng.permutation(F.n)[:12]; b_all = np.setdiff1d(np.arange(F.n), a_all)[:12]
        for a, b in zip(a_all, b_all):
            F.desc[b] = flip_bits(rng, F.desc[a][None], 3)[0]
    V = bow_ref.make_vocab(seed, k=k, L=L)
    tree = bow_ref.Tree(V)
    kf = make_keyframe(sc, rng, n_kf, related, **kw)
    if name == "duplicates":
        # two keyframe keypoints per pair, in index order: the first equals a (distance 0 to a, 3 to b: takes a), the second is one bit from a
        # (1 to a, 4 to b): it would take a too, finds it occupied and takes b
        mp = sc["map_points"]
        contest = []
        for j, (a, b) in enumerate(zip(a_all, b_all)):
            k1, k2 = 2 * j, 2 * j + 1
            d2 = np.array(F.desc[a], np.uint32, copy=True)
            free = [bit for bit in range(256) if not ((int(F.desc[a][bit // 32]) ^ int(F.desc[b][bit // 32])) >> (bit % 32)) & 1]
            bit = int(rng.choice(free)); d2[bit // 32] ^= np.uint32(1 << (bit % 32))
            kf["desc"][k1] = F.desc[a]; kf["desc"][k2] = d2
            for kk, t in ((k1, a), (k2, b)):
                kf["angle"][kk] = np.float32(np.mod(F.angle[t] + 10.0, 360.0)); kf["point_id"][kk] = 100000 + kk; kf["has_obs"][kk] = 1
                kf["world_pos"][kk] = np.asarray(mp["world_pos"], np.float32)[kk]; kf["src"][kk] = t
            contest.append((int(a), int(b), k1, k2))
    if name == "kf_all_null": kf["point_id"][:] = -1
    add_feature_vector(kf, tree, levelsup)
    if name == "disjoint_nodes":                                             # the keyframe's nodes: ids no frame feature can have
        kf["node"] = (kf["node"] + len(V["parent"])).astype(np.int32)
    return dict(name=name, sc=sc, vocab=V, tree=tree, levelsup=levelsup, kf=kf, Tcw_last=np.asarray(sc["Tcw_guess"], np.float32), contest=contest)
