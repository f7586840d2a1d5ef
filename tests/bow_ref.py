"""Independent numpy restatement of DBoW2's vocabulary as ORB-SLAM2 uses it (Thirdparty/DBoW2/DBoW2/ of the reference).  It shares no
code with lld_slam_amd: the text loader, the single-descriptor descent, both vector transforms, the L1 normalisation and the L1
score, each written from the lines cited in include/lld_amd.h.  Also: a seeded synthetic-vocabulary generator and a writer of
DBoW2's text format (the repository carries no vocabulary).

A vocabulary here is a dict: k, L, scoring, weighting, parent [n] (parent[0] = -1), is_leaf [n] u8 (the file flag), desc [n][8] u32
(byte order of the text), weight [n] f64."""
from __future__ import annotations

import numpy as np

POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


class Refused(ValueError):
    """loadFromTextFile returns false (or the file is one this restatement does not define)."""


# ------------------------------------------------------------------------------------------------------------------ loader

def parse_text(text: str) -> dict:
    """loadFromTextFile (TemplatedVocabulary.h:1338-1424) on the file's text.  Blank lines add no node (the documented deviation
    from the reference's `while(!f.eof())`, which parses a trailing empty line into one more child of the root)."""
    lines = text.split("\n")
    head = lines[0].split()
    if len(head) < 4:
        raise Refused("short header")
    try:
        k, L, n1, n2 = (int(x) for x in head[:4])
    except ValueError:
        raise Refused("header is not four ints")
    if k < 0 or k > 20 or L < 1 or L > 10 or n1 < 0 or n1 > 5 or n2 < 0 or n2 > 3:            # :1358
        raise Refused("header out of range")
    parent, is_leaf, desc, weight = [-1], [0], [bytes(32)], [0.0]
    for ln in lines[1:]:
        t = ln.split()
        if not t:
            continue
        if len(t) < 35:
            raise Refused("short node line")
        try:
            pid, leaf = int(t[0]), int(t[1])
            b = bytes(int(x) & 0xFF for x in t[2:34])                                             # (unsigned char)n, FORB.cpp:131
            w = float(t[34])
        except ValueError:
            raise Refused("malformed node line")
        if not (0 <= pid < len(parent)):
            raise Refused("parent is not an earlier node")
        parent.append(pid); is_leaf.append(1 if leaf > 0 else 0); desc.append(b); weight.append(w)
    return dict(k=k, L=L, scoring=n1, weighting=n2, parent=np.array(parent, np.int32), is_leaf=np.array(is_leaf, np.uint8),
                desc=np.frombuffer(b"".join(desc), "<u4").reshape(-1, 8).copy(), weight=np.array(weight, np.float64))


def read_text(path) -> dict:
    with open(path, "r") as f:
        return parse_text(f.read())


def write_text(V: dict, path, trailing_newline=True, blank_every=0):
    """DBoW2's text format: `k L scoring weighting`, then one line per node 1..n-1: `parent isLeaf d0 .. d31 weight`.  Weights
    are written with 17 significant digits so they read back exactly.  blank_every > 0 inserts an empty line after every
    blank_every nodes."""
    b = V["desc"].astype("<u4").view(np.uint8).reshape(-1, 32)
    out = [f"{V['k']} {V['L']} {V['scoring']} {V['weighting']}"]
    for i in range(1, len(V["parent"])):
        out.append(f"{V['parent'][i]} {int(V['is_leaf'][i])} " + " ".join(map(str, b[i].tolist())) + f" {float(V['weight'][i])!r}")
        if blank_every and i % blank_every == 0:
            out.append("")
    with open(path, "w") as f:
        f.write("\n".join(out) + ("\n" if trailing_newline else ""))


# ------------------------------------------------------------------------------------------------------------------ tree

def children(V: dict):
    """m_nodes[i].children: the child lines of i in file order (ascending id), :1384."""
    ch = [[] for _ in range(len(V["parent"]))]
    for i in range(1, len(V["parent"])):
        ch[int(V["parent"][i])].append(i)
    return ch


def word_ids(V: dict):
    """word_id per node: the lines with isLeaf > 0 numbered in file order (:1402-1409), -1 elsewhere."""
    w = np.full(len(V["parent"]), -1, np.int64)
    leaf = np.nonzero(V["is_leaf"] > 0)[0]
    w[leaf] = np.arange(len(leaf))
    return w


def distance(a, b):
    """FORB::distance (FORB.cpp:81-101): the 256-bit Hamming distance of [..., 8] u32 arrays."""
    x = np.bitwise_xor(a, b).astype("<u4").view(np.uint8)
    return POPCOUNT8[x].sum(axis=-1)


class Tree:
    """The children of every node as a padded matrix, for a vectorised descent."""

    def __init__(self, V: dict):
        ch = children(V)
        self.V = V
        self.nch = np.array([len(c) for c in ch], np.int64)
        kmax = max(1, int(self.nch.max()))
        self.ch = np.full((len(ch), kmax), -1, np.int64)
        for i, c in enumerate(ch):
            self.ch[i, :len(c)] = c
        self.word = word_ids(V)


def descend(T: Tree, desc, levelsup):
    """transform(feature, word_id, weight, &nid, levelsup) (:1218-1256) for every row of desc: returns (leaf node, word id, weight,
    nid).  Strict `<` over the children in order = the first minimum.  nid: the node at level m_L - levelsup, the root when that
    is <= 0, the leaf itself when the descent stops above it (the documented deviation)."""
    V = T.V
    desc = np.asarray(desc, np.uint32).reshape(-1, 8)
    n = len(desc)
    nid_level = V["L"] - levelsup
    cur = np.zeros(n, np.int64)
    nid = np.where(nid_level <= 0, 0, -1) * np.ones(n, np.int64)
    active = T.nch[cur] > 0
    level = 0
    while active.any():
        level += 1
        a = np.nonzero(active)[0]
        ch = T.ch[cur[a]]                                          # [m, kmax], -1 padded
        d = distance(desc[a][:, None, :], V["desc"][np.maximum(ch, 0)])
        d = np.where(ch >= 0, d, 1 << 20)
        best = ch[np.arange(len(a)), np.argmin(d, axis=1)]        # argmin: the first of equal minima
        cur[a] = best
        if level == nid_level:
            nid[a] = best
        active[a] = T.nch[best] > 0
    nid = np.where(nid < 0, cur, nid)
    return cur, T.word[cur], V["weight"][cur], nid


def transform(T: Tree, desc, levelsup=4):
    """transform(features, BowVector, FeatureVector, levelsup) (:1127-1194) followed by normalize(L1) (BowVector.cpp:62-84).
    Returns dict(word, value, node, node_start, feature, feature_word, feature_nid)."""
    V = T.V
    leaf, wid, w, nid = descend(T, desc, levelsup)
    bow, fv = {}, {}
    tf = V["weighting"] in (0, 1)
    for i in range(len(wid)):
        wi = float(w[i])
        if wi > 0:
            key = int(wid[i])
            if key in bow:
                if tf:
                    bow[key] = bow[key] + wi                       # BowVector::addWeight, :34-46
            else:
                bow[key] = wi                                      # first hit; addIfNotExist keeps it (:50-58)
            fv.setdefault(int(nid[i]), []).append(i)               # FeatureVector::addFeature
    words = sorted(bow)
    norm = 0.0
    for k_ in words:
        norm += abs(bow[k_])
    values = [bow[k_] / norm if norm > 0.0 else bow[k_] for k_ in words]
    nodes = sorted(fv)
    start, feat = [0], []
    for nd in nodes:
        feat.extend(fv[nd]); start.append(len(feat))
    fword = np.where(w > 0, wid, -1)
    return dict(word=np.array(words, np.int32), value=np.array(values, np.float64), node=np.array(nodes, np.int32),
                node_start=np.array(start, np.int32), feature=np.array(feat, np.int32), feature_word=fword.astype(np.int32),
                feature_nid=nid.astype(np.int32))


def score(v1, v2):
    """L1Scoring::score (ScoringObject.cpp:23-66) on (word, value) pairs with ascending words."""
    a = dict(zip(np.asarray(v1[0]).tolist(), np.asarray(v1[1]).tolist()))
    b = dict(zip(np.asarray(v2[0]).tolist(), np.asarray(v2[1]).tolist()))
    s = 0.0
    for wd in sorted(set(a) & set(b)):
        vi, wi = a[wd], b[wd]
        s += abs(vi - wi) - abs(vi) - abs(wi)
    return -s / 2.0


# ------------------------------------------------------------------------------------------------------------------ known answers

W_REPEAT = 7.8250594041967245            # 7 repeated additions of it differ from 7*w in the last bit
W_OTHER = 0.3


def bits(*idx):
    """A descriptor ([8] u32) with the given bits set (bit b = byte b//8, bit b%8 of mDescriptors.data)."""
    b = np.zeros(32, np.uint8)
    for i in idx:
        b[i // 8] |= 1 << (i % 8)
    return b.view("<u4").copy()


def hand_tree():
    """Root 0 -> A=1, B=2, C=3 (C is a leaf at depth 1, above the nid level of L=6, levelsup=4).  A -> 4, 5, 6 (6 is a stop word),
    B -> 7, 8, 9.  Header L = 6 puts nid at level 2, so only the leaves 4..9 are reached there.  File order = id order."""
    desc = np.zeros((10, 8), np.uint32)
    desc[1] = bits(0, 1, 2, 3)            # A
    desc[2] = bits(4, 5, 6, 7)            # B
    desc[3] = bits(100, 101, 102, 103, 104, 105, 106, 107, 108, 109)       # C, far from everything else
    desc[4] = bits(0, 1, 2, 3, 10)
    desc[5] = bits(0, 1, 2, 3, 11)
    desc[6] = bits(0, 1, 2, 3, 12)
    desc[7] = bits(4, 5, 6, 7, 20)
    desc[8] = bits(4, 5, 6, 7, 21)
    desc[9] = bits(4, 5, 6, 7, 22)
    parent = np.array([-1, 0, 0, 0, 1, 1, 1, 2, 2, 2], np.int32)
    is_leaf = np.array([0, 0, 0, 1, 1, 1, 1, 1, 1, 1], np.uint8)
    weight = np.array([0, 0, 0, 2.0, W_REPEAT, W_OTHER, 0.0, 1.5, 0.25, 4.0])
    return dict(k=3, L=6, scoring=0, weighting=0, parent=parent, is_leaf=is_leaf, desc=desc, weight=weight)


def hand_queries():
    """[tie A/B] [near 4 x7] [near 5] [near 6: stop] [near C]"""
    q = [bits(0, 1, 4, 5)]                                       # 2 bits from A and from B: the first child (A) wins
    q += [bits(0, 1, 2, 3, 10)] * 7                              # word of node 4, seven hits
    q += [bits(0, 1, 2, 3, 11), bits(0, 1, 2, 3, 12), bits(100, 101, 102, 103, 104, 105, 106, 107, 108)]
    return np.array(q, np.uint32)


# ------------------------------------------------------------------------------------------------------------------ generator

def make_vocab(seed, k=10, L=6, p_full=0.99, p_early_leaf=0.0, p_stop=0.0, flips=(24, 16, 10, 6, 4, 3, 2, 2, 2, 2), order="bfs",
               scoring=0, weighting=0):
    """A seeded hierarchical vocabulary.  Every internal node has k children with probability p_full, otherwise 2..k; below the
    root a node becomes a leaf early with probability p_early_leaf; nodes at depth L are leaves.  A child is its parent's
    descriptor with flips[depth-1] random bits flipped, so descriptors drawn near a leaf descend to it.  A fraction p_stop of the
    words gets weight 0 (stop words); the others a positive weight.  order: "bfs" (siblings on consecutive lines) or "dfs"
    (preorder: siblings separated by their subtrees)."""
    rng = np.random.default_rng(seed)
    parent = [np.array([-1], np.int64)]
    desc = [rng.integers(0, 1 << 32, (1, 8), dtype=np.uint64).astype(np.uint32)]
    depth_nodes = [np.array([0], np.int64)]
    n = 1
    for depth in range(L):
        par = depth_nodes[-1]
        pd = desc[-1] if depth == 0 else desc_level
        m = len(par)
        nch = np.where(rng.random(m) < p_full, k, rng.integers(2, k + 1, m))
        if depth > 0:
            nch = np.where(rng.random(m) < p_early_leaf, 0, nch)
        kids_par = np.repeat(np.arange(m), nch)
        cnt = len(kids_par)
        ids = np.arange(n, n + cnt)
        f = flips[min(depth, len(flips) - 1)]
        mask = np.zeros((cnt, 32), np.uint8)
        pos = rng.integers(0, 256, (cnt, f))
        np.bitwise_xor.at(mask, (np.repeat(np.arange(cnt), f), (pos // 8).ravel()), (1 << (pos % 8)).astype(np.uint8).ravel())
        desc_level = pd[kids_par] ^ mask.view("<u4").reshape(cnt, 8)
        parent.append(par[kids_par]); desc.append(desc_level); depth_nodes.append(ids)
        n += cnt
    parent = np.concatenate(parent)
    desc = np.concatenate(desc).astype(np.uint32)
    desc[0] = 0                                       # the root has no line in the text format; loaders leave it zero
    nchild = np.bincount(parent[1:], minlength=n)
    is_leaf = (nchild == 0).astype(np.uint8)
    is_leaf[0] = 0
    weight = np.zeros(n)
    leaves = np.nonzero(is_leaf)[0]
    weight[leaves] = rng.uniform(0.05, 12.0, len(leaves))
    weight[leaves[rng.random(len(leaves)) < p_stop]] = 0.0
    V = dict(k=k, L=L, scoring=scoring, weighting=weighting, parent=parent.astype(np.int32), is_leaf=is_leaf, desc=desc, weight=weight)
    return renumber_dfs(V) if order == "dfs" else V


def renumber_dfs(V: dict):
    """The same tree with node ids in preorder (children visited in ascending old id)."""
    ch = children(V)
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        stack.extend(reversed(ch[i]))
    order = np.array(order, np.int64)
    new = np.empty(len(order), np.int64); new[order] = np.arange(len(order))
    par = np.where(V["parent"][order] < 0, -1, new[np.maximum(V["parent"][order], 0)])
    return dict(V, parent=par.astype(np.int32), is_leaf=V["is_leaf"][order], desc=V["desc"][order], weight=V["weight"][order])


def near_leaves(V: dict, seed, n, max_flips=3):
    """n descriptors drawn near random words (0..max_flips bits flipped), and the word nodes they were drawn from."""
    rng = np.random.default_rng(seed)
    leaves = np.nonzero(V["is_leaf"])[0]
    src = leaves[rng.integers(0, len(leaves), n)]
    d = V["desc"][src].copy().view(np.uint8).reshape(n, 32)
    for j in range(max_flips):
        rows = np.nonzero(rng.random(n) < 0.5)[0]
        pos = rng.integers(0, 256, len(rows))
        d[rows, pos // 8] ^= (1 << (pos % 8)).astype(np.uint8)
    return d.view("<u4").reshape(n, 8).copy(), src


def random_desc(seed, n):
    return np.random.default_rng(seed).integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
