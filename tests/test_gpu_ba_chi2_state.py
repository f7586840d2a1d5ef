"""GPU parity of the outlier flags now that no kernel stores e->chi2() per trial: ba_classify_kernel and ba_finalize_kernel compute it from
the state buffer the window's last LM trial evaluated (BAState::ev), and the read-back takes the classification's snapshot for the point
edges round 2 left out.

The reference reads e->chi2() after optimize(): the error of the LAST state an error evaluation ran on - the rejected trial state when
the round ends on a rejected trial (g2o's pop() restores estimates, not errors), and a stale value for an edge the round did not
evaluate.  Every case below is one way of getting the wrong buffer or the wrong edge set; each is held to the CPU oracle with the
suite's own check_ba (identical outlier sets) and asserts from the returned statistics that the case it is named for occurred.  The
seeds were chosen on the CPU, on the oracle alone: its LM trace shows the rejected last trial on them.

Windows: at most 6 free + 2 fixed cameras, 150 points, 30 lines (the long-track case has as many cameras as a track of more than 64
observations needs)."""
import os

import numpy as np
import pytest

from lld_slam_amd import BABatch, Optimizer, synth
from test_gpu_ba import _with_long_tracks, check_ba, oracle_twins

pytestmark = pytest.mark.gpu

SMALL = dict(n_free=6, n_fixed=2, n_points=150, n_lines=30)
# noise-free observations with 30 % gross outliers: the LM converges within a few iterations and then rejects trial after trial; with
# max_trials = 3 a chain of three rejections ends the round (levenberg.cpp:149) ON a rejected trial
REJ = dict(noise=0.0, outlier_frac=0.3)
WID_ROUND1_REJECTED, WID_ROUND2_REJECTED, MAX_TRIALS = 3036, 3003, 3


def _win(wid, **kw):
    a = dict(SMALL); a.update(kw)
    return synth.make_lba_small(wid, **a)


def _same_lm_counts(g, o):
    assert g.stats["lm_trials"] == o.stats["lm_trials"] and g.stats["lm_iterations"] == o.stats["lm_iterations"], (g.stats, o.stats)


@pytest.fixture(scope="module")
def exp_ctx():
    """A context on the experiments build of the library (the LLD_BA_FORCE_BIG knob exists only there)."""
    from lld_slam_amd import Context, abi
    lib = abi.Lib(os.path.join(os.path.dirname(abi.product_library_path()), "liblld_amd_exp.so"), "lld_")
    ctx = Context(0, lib=lib)
    yield ctx
    ctx.close()


def test_round1_ends_on_a_rejected_trial(gpu_ctx, oracle):
    """(a) The classification between the rounds reads the chi2 of the REJECTED trial state (cur ^ 1), not of the state the round keeps."""
    w = _win(WID_ROUND1_REJECTED, **REJ)
    o, trace = oracle.local_ba_traced(w, max_trials=MAX_TRIALS)
    g = Optimizer(gpu_ctx).LocalBundleAdjustment(w, max_trials=MAX_TRIALS)
    _same_lm_counts(g, o)
    t1, i1 = g.stats["lm_trials"][0], g.stats["lm_iterations"][0]
    assert t1 > i1 and trace[t1 - 1, 2] == 0                # trials were rejected in round 1, and its last one was
    assert g.stats["lm_trials"][1] > 0 and g.pt_obs_outlier.any() and g.ln_edge_outlier.any()
    check_ba(g, o, w, twins=oracle_twins(oracle, w, max_trials=MAX_TRIALS))


def test_round2_ends_on_a_rejected_trial_and_excluded_edges_keep_their_stale_chi2(gpu_ctx, oracle):
    """(b) The read-back: edges of round 2 from the rejected trial state, the edges round 2 excluded from the classification's snapshot.
    The excluded edges are those a stop right after round 1 flags (Optimizer.cc:1230: the final classification then runs on the state and
    the errors the classification between the rounds would have seen).  An excluded POINT edge keeps its flag unless its depth test flips
    (its stale chi2 stays beyond the threshold) - none does on these windows; an excluded LINE edge is evaluated again at the final state
    (LineOptimizer.cc:185), so among the excluded edges both flags occur."""
    w = _win(WID_ROUND2_REJECTED, **REJ)
    o, trace = oracle.local_ba_traced(w, max_trials=MAX_TRIALS)
    g = Optimizer(gpu_ctx).LocalBundleAdjustment(w, max_trials=MAX_TRIALS)
    _same_lm_counts(g, o)
    (t1, t2), (_, i2) = g.stats["lm_trials"], g.stats["lm_iterations"]
    assert t2 > i2 and trace[t1 + t2 - 1, 2] == 0           # trials were rejected in round 2, and its last one was
    check_ba(g, o, w, twins=oracle_twins(oracle, w, max_trials=MAX_TRIALS))
    stop = dict(max_trials=MAX_TRIALS, abort_after_trials=t1)
    g1 = Optimizer(gpu_ctx).LocalBundleAdjustment(w, **stop)
    o1 = oracle.local_ba(w, **stop)
    _same_lm_counts(g1, o1)
    assert g1.stats["aborted"] == 1 and g1.stats["lm_trials"][1] == 0
    check_ba(g1, o1, w, twins=oracle_twins(oracle, w, **stop))
    ex_pt, ex_ln = g1.pt_obs_outlier == 1, (g1.ln_edge_outlier == 1) & (g.line_removed[np.repeat(np.arange(w.n_lines), np.diff(w.ln_obs_start))][:, None] == 0)
    assert ex_pt.sum() > 0 and ex_ln.sum() > 0
    assert g.pt_obs_outlier[ex_pt].all()                    # the stale values, still beyond the threshold
    after = np.concatenate([g.pt_obs_outlier[ex_pt], g.ln_edge_outlier[ex_ln]])
    assert (after == 0).any() and (after == 1).any()


@pytest.mark.parametrize("stop", [1, 3, "before_start"])
def test_stop_requests(gpu_ctx, oracle, stop):
    """(c) A stop after the first and after the third LM trial (the read-back classifies from the only round's last trial state), and a
    stop before the first optimize(): nothing classified, nothing written."""
    w = _win(3101, outlier_frac=0.15)
    if stop == "before_start":
        g = Optimizer(gpu_ctx).LocalBundleAdjustment(w, pbStopFlag=True)
        o = oracle.local_ba(w, abort=True)
        assert g.stats["aborted"] == o.stats["aborted"] == 1 and g.stats["lm_trials"] == [0, 0]
        for k in ("cam_qt", "pt_xyz", "line_x0", "line_dir", "pt_obs_outlier", "ln_edge_outlier", "line_removed"):
            np.testing.assert_array_equal(getattr(g, k), getattr(o, k), err_msg=k)
        np.testing.assert_array_equal(g.cam_qt, w.cam_qt); np.testing.assert_array_equal(g.pt_xyz, w.pt_xyz)
        assert not g.pt_obs_outlier.any() and not g.ln_edge_outlier.any() and not g.line_removed.any()
        return
    g = Optimizer(gpu_ctx).LocalBundleAdjustment(w, abort_after_trials=stop)
    o = oracle.local_ba(w, abort_after_trials=stop)
    _same_lm_counts(g, o)
    assert g.stats["aborted"] == 1 and g.stats["lm_trials"] == [stop, 0] and not g.line_removed.any()
    assert g.pt_obs_outlier.any()                           # the final classification still ran
    check_ba(g, o, w, twins=oracle_twins(oracle, w, abort_after_trials=stop))


def test_global_protocol_flags_nothing(gpu_ctx, oracle):
    """(d) Optimizer::BundleAdjustment erases nothing, gross outliers or not."""
    w = _win(3102, outlier_frac=0.3)
    g = Optimizer(gpu_ctx).GlobalBundleAdjustment(w, 4)
    o = oracle.local_ba(w, protocol=1, its_round1=4, robust_points=1)
    _same_lm_counts(g, o)
    assert g.stats["lm_trials"][0] >= 1 and g.stats["lm_trials"][1] == 0
    assert not g.pt_obs_outlier.any() and not g.ln_edge_outlier.any() and not g.line_removed.any()
    check_ba(g, o, w, twins=oracle_twins(oracle, w, protocol=1, its_round1=4, robust_points=1))


def test_window_without_landmarks(gpu_ctx, oracle):
    """(e) Nothing to optimise: straight to the read-back, no trial ever ran."""
    w = _win(3103, n_points=0, n_lines=0)
    g = Optimizer(gpu_ctx).LocalBundleAdjustment(w)
    o = oracle.local_ba(w)
    assert g.stats["lm_trials"] == [0, 0] and g.stats["lm_iterations"] == [0, 0] and g.stats["chi2_final"] == 0.0 and g.stats["aborted"] == o.stats["aborted"]
    np.testing.assert_array_equal(g.cam_qt, w.cam_qt)
    assert g.pt_obs_outlier.size == 0 and g.ln_edge_outlier.size == 0


def test_landmark_with_more_than_64_observations(gpu_ctx, oracle):
    """(f) The single-landmark task path of the point kernels (a track that does not fit one wavefront), both rounds and the classification."""
    w = _with_long_tracks(_win(3104, n_free=70, outlier_frac=0.15), n_long=3)
    assert np.diff(w.pt_obs_start)[:3].max() > 64
    g = Optimizer(gpu_ctx).LocalBundleAdjustment(w, reduced_solver=2)      # (the exact solver for more than 50 free cameras)
    o = oracle.local_ba(w)
    assert g.stats["lm_trials"][1] > 0 and g.pt_obs_outlier.any()
    check_ba(g, o, w, twins=oracle_twins(oracle, w))


def test_observations_that_are_not_widened_floats(gpu_ctx, oracle):
    """(g) The kernels of the as-given observation layout (_f64)."""
    rng = np.random.default_rng(7)
    w = _win(3105, outlier_frac=0.15, mono_frac=0.2)
    uvr = w.pt_obs_uvr.copy(); mono = uvr < 0
    uvr += rng.uniform(-1e-6, 1e-6, uvr.shape); uvr[mono] = w.pt_obs_uvr[mono]
    assert np.any(uvr.astype(np.float32).astype(np.float64) != uvr)
    w.pt_obs_uvr = uvr
    w.ln_obs_left = w.ln_obs_left + rng.uniform(-1e-6, 1e-6, w.ln_obs_left.shape)
    g = Optimizer(gpu_ctx).LocalBundleAdjustment(w)
    o = oracle.local_ba(w)
    assert g.stats["lm_trials"][1] > 0 and g.pt_obs_outlier.any()
    check_ba(g, o, w, twins=oracle_twins(oracle, w))


def test_hbm_accumulator_kernels(exp_ctx, oracle, monkeypatch):
    """(h) The `big` kernels, forced on a small window through the experiments build."""
    monkeypatch.setenv("LLD_BA_FORCE_BIG", "1")
    w = _win(3106, outlier_frac=0.15)
    with pytest.raises(RuntimeError):                       # the path really is taken: it has no bit-reproducible mode
        Optimizer(exp_ctx).LocalBundleAdjustment(w, deterministic=1)
    g = Optimizer(exp_ctx).LocalBundleAdjustment(w)
    o = oracle.local_ba(w)
    assert g.stats["lm_trials"][1] > 0 and g.pt_obs_outlier.any()
    check_ba(g, o, w, tail="shared accumulators")


def test_monocular_observations(gpu_ctx, oracle):
    """(i) Half of the point observations monocular: two residual rows and the other threshold."""
    w = _win(3107, outlier_frac=0.15, mono_frac=0.5)
    mono = w.pt_obs_uvr[:, 2] < 0
    assert 0.3 < mono.mean() < 0.7
    g = Optimizer(gpu_ctx).LocalBundleAdjustment(w)
    o = oracle.local_ba(w)
    assert g.pt_obs_outlier[mono].any() and g.pt_obs_outlier[~mono].any() and not g.pt_obs_outlier[mono].all()
    check_ba(g, o, w, twins=oracle_twins(oracle, w))


def test_mixed_batch_gives_the_same_records_however_it_is_grouped(gpu_ctx, oracle):
    """(j) The cases above in one batch (one parameter set per batch: max_trials = 3; a window that is no float would move the whole batch
    to the other layout and a stop request is per batch, so (c), (g) and (h) stay out), solved as 1, 2 and 4 groups: the fused and the
    separate kernels, queued super-steps.  Bit-identical records, and the oracle's results."""
    ws = [_win(WID_ROUND1_REJECTED, **REJ), _win(WID_ROUND2_REJECTED, **REJ), _win(3103, n_points=0, n_lines=0), _win(3107, outlier_frac=0.15, mono_frac=0.5),
          _with_long_tracks(_win(3104, n_free=70, outlier_frac=0.15), n_long=3), _win(3014, **REJ), _win(3101, outlier_frac=0.15), _win(3108, n_free=3, n_fixed=1, n_points=40, n_lines=7)]
    recs = {}
    with BABatch(gpu_ctx, ws, max_trials=MAX_TRIALS, reduced_solver=2) as b:
        for groups in (1, 2, 4):
            b.set_groups(groups)
            b.solve()
            recs[groups] = [b.download(i) for i in range(len(ws))]
    for groups in (2, 4):
        for a, c in zip(recs[1], recs[groups]):
            for k in ("cam_qt", "pt_xyz", "line_x0", "line_dir", "pt_obs_outlier", "ln_edge_outlier", "line_removed"):
                np.testing.assert_array_equal(getattr(a, k), getattr(c, k), err_msg=k)
            assert a.stats == c.stats
    for i, w in enumerate(ws):
        if w.n_points == 0: continue                        # (e): compared above, nothing for the oracle to solve
        o = oracle.local_ba(w, max_trials=MAX_TRIALS)
        _same_lm_counts(recs[1][i], o)
        check_ba(recs[1][i], o, w, twins=oracle_twins(oracle, w, max_trials=MAX_TRIALS))
    t, it = recs[1][0].stats["lm_trials"], recs[1][0].stats["lm_iterations"]
    assert t[0] > it[0]                                     # the rejection chain of (a), inside the batch
