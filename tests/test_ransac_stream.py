"""lld_ransac_stream.h on the CPU: the rand() stream, the minimal-set draw, the stream rewind and the iteration budget that the
PnP, Sim3 and Initializer solvers share, against the restatements of pnp_ref / sim3solver_ref.  The header is compiled without
HIP into a stand-alone C++17 program (-Wall -Werror; with gcc's address and undefined-behaviour sanitizers linked statically
when their runtimes are installed) whose output is compared value for value.  CPU only."""
import math
import os
import subprocess

import numpy as np
import pytest

import pnp_ref as P
import sim3solver_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 12345, 2**32 - 1]
KS = [3, 4, 8]
SETS = 20                           # consecutive sets drawn from one stream
WINDOW = 7                          # sets drawn between save and rewind
BUDGET_N = [0, 3, 4, 9, 10, 19, 20, 21, 2000]
PNP_PARAMS = (0.99, 10, 300, 4, 0.5)            # Tracking::Relocalization
SIM3_PARAMS = (0.99, 20, 300)                   # LoopClosing::ComputeSim3


def sizes(K):
    return [K, K + 1, 2 * K - 1, 50]            # N = K and K + 1: every draw after the first hits a swapped-back position


def budget_cases():
    """(probability, epsilon, min_inliers, N, max_iterations, expected mRansacMaxIts) from each restatement's own constants."""
    out = []
    for N in BUDGET_N:
        for mi in (1, 300):
            prob, mn, _, ms, eps = PNP_PARAMS
            n_min, its, e = P.ransac_constants(N, prob, mn, mi, ms, eps)
            out.append((prob, np.float32(e), n_min, N, mi, its))
            prob, mn, _ = SIM3_PARAMS
            with np.errstate(divide="ignore"):
                e = np.float32(mn) / np.float32(N)                                  # sim3solver_ref.ransac_constants' epsilon
            out.append((prob, e, mn, N, mi, S.ransac_constants(N, prob, mn, mi)))
    return out


def c_float(x):
    return "INFINITY" if math.isinf(x) else float(x).hex() + "f"


SOURCE = r"""
#include <cstdio>
#include "%(root)s/lld_slam_amd/csrc/lld_ransac_stream.h"

static const uint32_t kSeeds[] = {%(seeds)s};
struct Budget { double p; float eps; int min_inliers, N, max_iterations; };
static const Budget kBudget[] = {%(budget)s};

template <int K>
static void draws(int N, uint32_t seed) {
  RansacStream s;
  srand_state(seed, s.ring, &s.head);
  for (int k = 0; k < %(sets)d; ++k) {
    int32_t out[K];
    draw_set<K>(s.ring, s.head, N, out);
    for (int i = 0; i < K; ++i) std::printf("%%d ", out[i]);
  }
  std::printf("%%u\n", rng_next(s.ring, s.head) >> 1);
}

template <int K>
static void rewinds(uint32_t seed) {
  const int runs[3] = {0, 1, %(window)d};
  for (int run : runs) {
    RansacStream s;
    srand_state(seed, s.ring, &s.head);
    s.save();
    int32_t out[K];
    for (int k = 0; k < %(window)d; ++k) draw_set<K>(s.ring, s.head, 50, out);
    s.rewind(K * run);
    for (int i = 0; i < 5; ++i) std::printf("%%u ", rng_next(s.ring, s.head) >> 1);
    std::printf("\n");
  }
}

template <int K>
static void all_of(const int (&Ns)[4]) {
  for (uint32_t seed : kSeeds) {
    for (int N : Ns) draws<K>(N, seed);
    rewinds<K>(seed);
  }
}

int main() {
  all_of<3>({%(n3)s});
  all_of<4>({%(n4)s});
  all_of<8>({%(n8)s});
  for (const Budget& b : kBudget) std::printf("%%d\n", ransac_max_iterations(b.p, b.eps, b.min_inliers, b.N, b.max_iterations));
  return 0;
}
"""


def have_static_sanitizers():
    def found(name):
        return os.path.isabs(subprocess.check_output(["g++", "-print-file-name=" + name], text=True).strip())
    return found("libasan.a") and found("libubsan.a")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("ransac_stream")
    cases = budget_cases()
    src = d / "stream.cpp"
    src.write_text(SOURCE % dict(
        root=ROOT, seeds=", ".join("%du" % s for s in SEEDS), sets=SETS, window=WINDOW,
        budget=", ".join("{%r, %s, %d, %d, %d}" % (p, c_float(e), mn, N, mi) for p, e, mn, N, mi, _ in cases),
        n3=", ".join(map(str, sizes(3))), n4=", ".join(map(str, sizes(4))), n8=", ".join(map(str, sizes(8)))))
    exe = d / "stream"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + (san if have_static_sanitizers() else []) +
                          [str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)], text=True).splitlines()


def expected_stream_lines():
    out = []
    for K in KS:
        for seed in SEEDS:
            for N in sizes(K):
                rng = P.GlibcRand(seed)
                idx = [i for _ in range(SETS) for i in P.draw_set(rng, N, K)]
                out.append(idx + [rng.rand()])
            for run in (0, 1, WINDOW):
                rng = P.GlibcRand(seed)
                for _ in range(K * run):
                    rng.rand()
                out.append([rng.rand() for _ in range(5)])
    return out


def test_draws_and_rewind_equal_the_restatement(lines):
    want = expected_stream_lines()
    got = [[int(x) for x in ln.split()] for ln in lines[:len(want)]]
    assert len(got) == len(want) == len(KS) * len(SEEDS) * (4 + 3)
    for g, w in zip(got, want):
        assert g == w


def test_budget_equals_both_restatements(lines):
    cases = budget_cases()
    got = [int(x) for x in lines[-len(cases):]]
    assert len(lines) == len(KS) * len(SEEDS) * 7 + len(cases)
    assert got == [c[5] for c in cases]
    assert any(c[3] < c[2] and c[5] == 1 for c in cases)        # N < min_inliers: budget 1
