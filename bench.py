#!/usr/bin/env python3
"""bench.py — throughput of the batched local bundle adjustment (the metric of BASELINE.json) on N MI355X.

  python bench.py --gpus 1 --steps 3 --warmup 1            (the headline alone)
  python bench.py --gpus 1 --steps 3 --warmup 1 --full     (the headline and every other figure below)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one pass of the hot path (Optimizer::LocalBundleAdjustment, both LM rounds, outlier protocol, read-back) over
one batch of synthetic LBA-B windows (50 free + 10 fixed KFs, 10 000 points x 6 stereo observations, 2 000 lines x 5 KFs x
left/right = 80 000 edges) that is ALREADY RESIDENT in HBM; every step restarts from the uploaded initial state.  Windows
are independent, so ranks shard the window list - weak scaling by default (--windows-per-gpu windows on every GPU), --strong
splits the same --windows-per-gpu windows over the ranks - and the only collective is the gather of the fixed-stride result
records to rank 0 (RCCL), inside the timed region (lld_slam_amd/dist.py, the module tests/test_distributed_cpu.py drives over gloo).

Rank 0 prints ONE JSON line.  A plain run does what the headline needs and no more: it generates the windows, uploads them, ramps the
clocks, runs the W warm-up and the K timed steps, writes --dump-outputs and prints `value`, `ms_per_step`, `config` and `lm`.  Everything
else is measured with --full only (each block can be left out of a --full run by its --no-* option); without it these keys are null or absent:
  config.gathered_records_ok  the gathered result records checked against the windows each rank was given (N = 1: one untimed step through
                a one-rank RCCL group after the timed region)
  rccl_overhead N = 1: the K steps again with the asynchronous one-rank RCCL gather behind every solve, against K plain steps
  roofline      the dominant kernel family of the step (by summed HIP-event time on the library's own stream) under two rulers:
                model bytes (SURVEY.md §8d record sizes) against the nominal 8 TB/s, and the bytes the HBM-side
                counters saw (profiles/roofline_traffic.json) against the 6.3 TB/s a streaming kernel reaches on this part; every
                other family under both rulers in `families`
  cpu_baseline  the single-threaded CPU oracle (a port of the reference algorithm, not the reference binary) on a bounded sample;
  parity        the same sample's results against the device's (matched chi2, identical outlier sets)
  e2e           host buffers in -> results out at the C ABI, steady state: three host threads, each create -> solve -> download on its
                own context (NOT `value`, which times resident windows)
  secondary     the other BASELINE.json configs, untimed by `value`: PoseOptimization (4096 frames), ORB + LBD brute force (1024 frame
                pairs), LBA-A (128 windows), one lld_local_ba call, batches of 32 / 64 windows, the bit-reproducible mode - each with its
                own ruler and CPU baseline at N = 1; at N > 1 the PO frames and the frame pairs are split over the ranks (dist.gather_rows)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

METRIC = "local-BA windows/sec (50 KF, 10k pts, 2k lines) at matched chi2; 1/2/4/8 GPU"
HBM_PEAK_GBS = 8000.0               # nominal HBM3E (MI355X_MICROARCH.md)
HBM_ACHIEVABLE_GBS = 6300.0         # what a streaming kernel reaches on this part (same guide)
FP64_FMA_PEAK_T = 39.3              # 256 CU x 4 SIMD x 16 lanes/clk x 2.4 GHz (vector fp64 FMA/s; the fp64 matrix rate is the same)
# 32-bit VALU lane-ops/s for the Hamming kernel's mix of 8 v_xor_b32 + 8 v_bcnt_u32_b32 per descriptor pair, MEASURED on the part
# (tools/microbench/valu_rate.hip: v_xor_b32 55.3 T, v_bcnt_u32_b32 35.0 T, v_fma_f32 44.3 T lane-ops/s with 8 waves per SIMD):
# 16 / (8 / 55.3 + 8 / 35.0).  The 78.6 T of the data sheet (32 lanes/clk/SIMD) is the packed-fp32 rate; no integer instruction reaches it.
VALU32_PEAK_T = 42.9
PHASES = ["ba_linearize", "ba_schur", "ba_solve", "ba_backsub", "ba_control"]


# ================================================================================================== byte / FMA models
def algorithmic_bytes(w, n_trials, n_iters, pcg_iters):
    """Algorithmic HBM bytes of each kernel family for ONE window over a whole solve (SURVEY.md §8(d) record sizes).

    E_in: 44 B per stereo point edge, 36 B mono, 60 B per line edge; W: 144 B / 192 B per edge with a free camera;
    V: 72 B per point, 128 B per line; X: 56 B camera, 24 B point, 40 B line; S: 288 B per 6x6 block.
    """
    import numpy as np
    nf = w.n_free_cams
    mono = int(np.count_nonzero(w.pt_obs_uvr[:, 2] < 0))
    es = w.n_pt_obs - mono
    el = w.n_ln_obs + int(np.count_nonzero(w.ln_obs_right[:, 0] >= 0))
    e_in = 44 * es + 36 * mono + 60 * el
    free_p = int(np.count_nonzero(w.pt_obs_cam < nf))
    free_l = int(np.count_nonzero(np.repeat(w.ln_obs_cam < nf, 2)[(np.stack([np.ones(w.n_ln_obs, bool), w.ln_obs_right[:, 0] >= 0], 1)).reshape(-1)]))
    wb = 144 * free_p + 192 * free_l
    v = 72 * w.n_points + 128 * w.n_lines
    x = 56 * w.n_cams + 24 * w.n_points + 40 * w.n_lines
    s_blocks = nf * nf                                   # the kernel stores the full symmetric matrix
    return {
        "ba_linearize": n_iters * (e_in + wb + v + x // 2),
        "ba_schur": n_trials * (wb + v + 288 * s_blocks),
        "ba_solve": n_trials * 288 * s_blocks + pcg_iters * (288 * s_blocks + 5 * 48 * nf),     # S read once per exact solve (+ the PCG stream when it runs)
        "ba_backsub": n_trials * (wb + v + e_in + x),
        "ba_control": 0,
    }


def schur_fmas(w, n_trials):
    """fp64 FMAs of the Schur family for ONE window over a whole solve (the arithmetic that actually bounds it): per landmark with k
    free-camera observations, k x (rebuild the 6xD Hpl block in closed form ~70 for a point / 0 for a line whose block is stored,
    Z = W L^-T 6*D*(D+1)/2, Z (L^-1 b) 6*D) + one D x D Cholesky (~10 / ~20) + k(k+1)/2 block products Z_a Z_b^T of 6*6*D."""
    import numpy as np
    nf = w.n_free_cams
    kp = np.add.reduceat((w.pt_obs_cam < nf).astype(np.int64), w.pt_obs_start[:-1]) if w.n_points else np.zeros(0, np.int64)
    kp = np.where(np.diff(w.pt_obs_start) > 0, kp, 0)
    kl = np.add.reduceat((w.ln_obs_cam < nf).astype(np.int64), w.ln_obs_start[:-1]) if w.n_lines else np.zeros(0, np.int64)
    kl = np.where(np.diff(w.ln_obs_start) > 0, kl, 0)
    pts = np.sum(kp * (70 + 36 + 18) + 10 * (kp > 0) + kp * (kp + 1) // 2 * 108)
    lns = np.sum(kl * (60 + 24) + 20 * (kl > 0) + kl * (kl + 1) // 2 * 144)
    return int(n_trials * (pts + lns))


def pose_fmas(n_points, n_line_edges, iterations, trials):
    """fp64 FMAs of one PoseOptimization (counted from lld_pose.hip's arithmetic): a linearising sweep costs ~125 per point
    edge (map 12, project 8, 3x6 Jacobian 25, 21 + 6 accumulators x 3 rows 80) and ~180 per line edge (two maps 24, image line 14,
    2x6 Jacobian 80, accumulators 54, rest 8), an error-only sweep ~20 / ~45; one linearising sweep per LM iteration, one error sweep per trial."""
    return iterations * (125 * n_points + 180 * n_line_edges) + trials * (20 * n_points + 45 * n_line_edges)


def _issue_table():
    """profiles/roofline_issue.json: SQ counters per launch of every kernel family (tools/make_roofline_issue.py)."""
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "roofline_issue.json")))
    except Exception:
        return {}


def _secondary_rulers(kernel_substr):
    """Counter-backed rulers of a secondary kernel (profiles/secondary_rulers.json, tools/make_secondary_rulers.py): VALU issue, LDS pipe, HBM bytes
    per dispatch as rocprofv3 --pmc passes of tools/run_secondary_kernels.py saw them - NOT re-measured in this run."""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "secondary_rulers.json")))
    except Exception:
        return None
    for k, v in t.items():
        if kernel_substr in k:
            return dict(v, kernel=k, source="profiles/secondary_rulers.json (" + str(t.get("_taken_on", "")) + ")")
    return None


def _traffic_table():
    path = os.path.join(ROOT, "profiles", "roofline_traffic.json")
    try:
        t = json.load(open(path))
        if "ba_pcg" in t and "ba_solve" not in t:
            t["ba_solve"] = t["ba_pcg"]
        return t
    except Exception:
        return {}


def _spread(xs):
    import numpy as np
    return {"min": round(float(np.min(xs)), 3), "median": round(float(np.median(xs)), 3), "max": round(float(np.max(xs)), 3), "repeats": len(xs)}


class StreamTimer:
    """HIP events on the library's OWN stream (torch.cuda.Event.record() defaults to torch's current stream, which the C ABI never uses)."""

    def __init__(self, ctx):
        import torch
        self.torch = torch
        self.stream = torch.cuda.ExternalStream(ctx.stream())

    def time_ms(self, fn):
        e0 = self.torch.cuda.Event(enable_timing=True); e1 = self.torch.cuda.Event(enable_timing=True)
        e0.record(self.stream); fn(); e1.record(self.stream); e1.synchronize()
        return e0.elapsed_time(e1)


# ================================================================================================== secondary configs (N = 1, rank 0, untimed by `value`)
def sharded_secondary(ctx, dev, world, rank, repeats=5):
    """N > 1: the PO frames and the ORB / LBD frame pairs of the `secondary` block split over the ranks (north_star: "independent local-BA
    windows and frame-pair match batches shard embarrassingly across the 8 GPUs ... RCCL only for the final gather").  Every rank solves
    its contiguous share (dist.shard, strong form: the totals are the config's), the rate is total items / the slowest rank's median
    launch, and the result rows travel to rank 0 through dist.gather_rows.  No CPU legs here (N = 1 carries them).
    Every leg is `local work -> all ranks agree that it went well -> collectives`: a rank that fails locally (allocation, an assert) tells
    the others through ONE all-reduce that every rank always reaches, and all of them skip the leg's collectives together - a rank alone in
    a collective would hang the job until RCCL's timeout."""
    import numpy as np
    import torch
    from lld_slam_amd import PoseBatch, dist as D, synth
    timer = StreamTimer(ctx)
    out = {}

    def leg(name, local, collect):
        err = None; data = None
        try:
            data = local()
        except Exception as ex:
            err = repr(ex)[:300]
        if not D.all_ranks_ok(err is None, dev, True):
            out[name] = {"error": err or "another rank failed in this leg; its collectives were skipped on every rank"}
            return
        out[name] = collect(data)

    def agg(n_total, med_ms, counts, unit, workload, extra=None):
        worst = D.max_over_ranks(med_ms, dev, True)
        r = {"workload": workload, "value": round(n_total / (worst * 1e-3), 1), "unit": unit, "n_gpus": world, "items_per_rank": counts,
             "slowest_rank_median_launch_ms": round(worst, 4), "this_rank_median_launch_ms": round(med_ms, 4)}
        if extra: r.update(extra)
        return r

    # ---- PoseOptimization
    nf = 4096
    def po_local():
        f0, fc = D.shard(nf, world, rank, True)
        distinct = [synth.make_pose_frame(i) for i in range(64)]
        frames = [distinct[(f0 + i) % 64] for i in range(fc)]
        with PoseBatch(ctx, frames, gamma=0.5) as b:
            b.solve(); ctx.synchronize()
            ms = [timer.time_ms(b.solve) for _ in range(repeats)]
            res = [b.download(i) for i in range(fc)]
        rows = torch.from_numpy(np.array([list(r.pose_qt) + [float(r.n_inliers)] for r in res], np.float64).reshape(fc, 8)).to(dev)
        return fc, ms, rows
    def po_collect(d):
        fc, ms, rows = d
        counts = D.gather_counts(fc, dev, True, world)
        got = D.gather_rows(rows, counts, world, rank)
        ok = None
        if rank == 0:
            allr = torch.cat(got).cpu().numpy()
            # frame i of the whole set is distinct[i % 64]: equal inputs must have given equal rows on whatever rank they ran
            ok = bool(allr.shape == (nf, 8) and np.isfinite(allr).all() and all(np.allclose(allr[i, :7], allr[i % 64, :7], rtol=0, atol=1e-12) for i in range(0, nf, 97)))
        return agg(nf, float(np.median(ms)), counts, "frames/s", f"{nf} PO frames split over {world} GPUs, 1000 stereo point + 400 line edges each, 4 x 10 LM iterations",
                   {"gathered_rows_ok": ok})
    leg("pose_opt", po_local, po_collect)

    # ---- ORB / LBD
    B = 1024
    p0, pc = D.shard(B, world, rank, True)
    nq = nt = 2000
    def orb_local():
        qs, ts = zip(*[synth.make_match_orb(i, nq, nt) for i in range(8)])
        q = torch.from_numpy(np.stack([qs[(p0 + i) % 8] for i in range(pc)]).view(np.int32)).to(dev); tt = torch.from_numpy(np.stack([ts[(p0 + i) % 8] for i in range(pc)]).view(np.int32)).to(dev)
        outs = [torch.empty((pc, nq), dtype=torch.int32, device=dev) for _ in range(4)]
        fn = ctx.lib.fn("match_hamming256_batch_dev")
        def run_orb():
            assert fn(ctx.handle, pc, q.data_ptr(), nq, tt.data_ptr(), nt, *[o.data_ptr() for o in outs]) == 0
        torch.cuda.synchronize(); run_orb(); ctx.synchronize()
        ms = [timer.time_ms(run_orb) for _ in range(repeats)]
        return ms, torch.stack(outs, 2)
    def orb_collect(d):
        ms, rows = d
        counts = D.gather_counts(pc, dev, True, world)
        got = D.gather_rows(rows, counts, world, rank)            # [pairs, queries, 4] int32
        ok = None
        if rank == 0:
            allm = torch.cat(got)
            ok = bool(tuple(allm.shape) == (B, nq, 4) and all(bool(torch.equal(allm[i], allm[i % 8])) for i in range(0, B, 61)))
        return agg(B, float(np.median(ms)), counts, "frame pairs/s", f"{B} frame pairs split over {world} GPUs, {nq} x {nt} 256-bit ORB descriptors", {"gathered_rows_ok": ok})
    leg("orb_hamming256", orb_local, orb_collect)

    n1 = n2 = 300; Dd = 72
    def lbd_local():
        ql, tl = zip(*[synth.make_match_lbd(i, n1, n2, Dd) for i in range(8)])
        q2 = torch.from_numpy(np.stack([ql[(p0 + i) % 8] for i in range(pc)])).to(dev); t2 = torch.from_numpy(np.stack([tl[(p0 + i) % 8] for i in range(pc)])).to(dev)
        bi = torch.empty((pc, n1), dtype=torch.int32, device=dev); si = torch.empty_like(bi)
        bd = torch.empty((pc, n1), dtype=torch.float64, device=dev); sd = torch.empty_like(bd)
        fn2 = ctx.lib.fn("match_l2f32_batch_dev")
        def run_lbd():
            assert fn2(ctx.handle, pc, q2.data_ptr(), n1, t2.data_ptr(), n2, Dd, bi.data_ptr(), bd.data_ptr(), si.data_ptr(), sd.data_ptr()) == 0
        torch.cuda.synchronize(); run_lbd(); ctx.synchronize()
        ms = [timer.time_ms(run_lbd) for _ in range(repeats)]
        return ms, torch.stack([bi, si], 2)
    def lbd_collect(d):
        ms, rows = d
        counts = D.gather_counts(pc, dev, True, world)
        got = D.gather_rows(rows, counts, world, rank)
        ok = None
        if rank == 0:
            allm = torch.cat(got)
            ok = bool(tuple(allm.shape) == (B, n1, 2) and all(bool(torch.equal(allm[i], allm[i % 8])) for i in range(0, B, 61)))
        return agg(B, float(np.median(ms)), counts, "frame pairs/s", f"{B} frame pairs split over {world} GPUs, {n1} x {n2} LBD descriptors of {Dd} floats", {"gathered_rows_ok": ok})
    leg("lbd_l2f32", lbd_local, lbd_collect)
    return out


def small_batch_block(ctx, windows, repeats=5):
    """Resident rate of batches of 32 and 64 windows (the per-GPU share of BASELINE config 5 at 8 and 4 GPUs): the strong-scaling
    predictor one GPU offers."""
    import numpy as np
    from lld_slam_amd import BABatch
    out = {}
    for nw in (32, 64):
        if len(windows) < nw:
            continue
        with BABatch(ctx, windows[:nw]) as b:
            b.solve()
            wall = []
            for _ in range(repeats):
                t0 = time.perf_counter(); b.solve(); wall.append((time.perf_counter() - t0) * 1e3)
        out[f"{nw}_windows"] = {"value": round(nw / (float(np.median(wall)) * 1e-3), 1), "unit": "windows/s", "solve_ms": _spread(wall)}
    return out


def deterministic_block(ctx, windows, repeats=3):
    """The bit-reproducible DEFAULT mode on the same resident windows - the result records of repeats + 1 solves compared byte for byte on the
    device - next to lld_ba_params.deterministic = 0 (shared accumulator copies: faster by what `cost_of_the_default` says, reproducible
    to rounding only).  VERDICT r3 item 3."""
    import numpy as np
    import torch
    from lld_slam_amd import BABatch
    out = {}
    for name, mode in (("default_bit_reproducible", 2), ("shared_accumulators", 0)):
        with BABatch(ctx, windows, deterministic=mode) as b:
            b.solve(); ptr, stride = b.result_records()
            class _Dev:
                __cuda_array_interface__ = {"shape": (stride * len(windows),), "typestr": "|u1", "data": (ptr, False), "version": 2}
            rec0 = torch.as_tensor(_Dev(), device=f"cuda:{ctx.device}").clone()
            wall = []; same = True
            for _ in range(repeats):
                t0 = time.perf_counter(); b.solve(); wall.append((time.perf_counter() - t0) * 1e3)
                same = same and bool(torch.equal(rec0, torch.as_tensor(_Dev(), device=f"cuda:{ctx.device}")))
        out[name] = {"deterministic": mode, "value": round(len(windows) / (float(np.median(wall)) * 1e-3), 1), "unit": "windows/s", "solve_ms": _spread(wall),
                     "result_records_bit_identical": same, "solves_compared": repeats + 1}
    out["cost_of_the_default"] = round(1.0 - out["default_bit_reproducible"]["value"] / out["shared_accumulators"]["value"], 4)
    out["workload"] = f"the same {len(windows)} resident windows, one batch per mode; per-wavefront accumulator copies and a fixed summation order against copies shared by all wavefronts of a workgroup"
    return out


def tracking_frame_block(ctx, repeats=200):
    """The Tracking thread's per-frame chain on ONE synthetic stereo frame (2000 keypoints + 300 stereo lines; 1200 points and 140 lines tracked in
    the last frame; 2500 local MapPoints, 260 local MapLines): TrackWithMotionModel = SearchByProjection(Current, Last) -> AddLinesFrom ->
    PoseOptimization -> outlier discard, TrackLocalMap = SearchLocalPoints -> AddLinesFrom -> PoseOptimization (src/Tracking.cc:885-994,
    :1126-1220) as ONE device-resident sequence behind the C ABI (lld_frame_track_*), driven from COMPILED C++ (examples/harness track, a child
    process: `repeats` frames on one handle, host wall clock per frame), next to the CPU oracle's own run of the whole sequence
    (oracle/oracle_tracking.py) whose per-stage records are compared with the device's."""
    import numpy as np
    import oracle_tracking as OT
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import time_track_chain as TT
    res, sc, (g1, g2) = TT.run(repeats, 0, False)
    res_between = TT.run(repeats, 0, True)[0]
    res_points = TT.run(repeats, 0, False, n_lines=0)[0]
    OT.track_frame(sc)                                            # (first call loads the oracle library)
    cpu = []
    for _ in range(5):
        tc = time.perf_counter(); e1, e2 = OT.track_frame(sc); cpu.append((time.perf_counter() - tc) * 1e3)

    def same(g, e):
        ids = all(np.array_equal(g[k], e[k]) for k in ("kp_point_id", "kp_outlier", "ln_line_id", "ln_outlier"))
        cnt = all(g[k] == e[k] for k in ("n_inliers", "n_edges", "n_search", "n_points", "n_points_map", "n_lines_matched", "n_lines", "n_discarded"))
        dq = float(np.max(np.abs(g["pose_qt"][:4] - e["pose_qt"][:4]))); dt = float(np.linalg.norm(g["pose_qt"][4:] - e["pose_qt"][4:]) / max(1.0, np.linalg.norm(e["pose_qt"][4:])))
        return ids, cnt, max(dq, dt), abs(g["chi2"] - e["chi2"]) / max(abs(e["chi2"]), 1e-12)
    a, b = same(g1, e1), same(g2, e2)
    err0 = float(np.linalg.norm(np.asarray(sc["pose_guess"])[4:] - np.asarray(sc["pose_true"])[4:]))
    err2 = float(np.linalg.norm(g2["pose_qt"][4:] - np.asarray(sc["pose_true"])[4:]))
    return {"workload": "one stereo frame: 2000 keypoints + 300 lines; last frame 1200 points + 140 lines; local map 2500 MapPoints + 260 MapLines; both stages of the "
                        "Tracking thread (search -> AddLinesFrom -> PoseOptimization -> discard, twice) with the Frame's state resident in HBM",
            "unit": "ms per frame (host wall clock around TrackWithMotionModel + TrackLocalMap + download in examples/harness.cpp; uploads of the stage inputs included, "
                    "the Frame's own keypoints / lines are uploaded once per frame handle, outside)",
            "driven_from": "compiled C++ (examples/harness track), child process",
            "one_download_at_the_end": res, "download_between_the_stages": res_between, "points_only_no_lines": res_points,
            "translation_error_m": {"predicted_pose": round(err0, 4), "after_the_sequence": round(err2, 5)},
            "cpu_baseline": {"value": round(float(np.median(cpu)), 2), "unit": "ms per frame", "cores": 1, "kind": "port",
                             "sample": "the same two stages, lines included, through oracle/oracle_tracking.py (median of 5)"},
            "parity": {"against": "the oracle's own run of the sequence (no device state handed over)",
                       "stage1_ids_and_outlier_flags_bit_exact": bool(a[0]), "stage2_ids_and_outlier_flags_bit_exact": bool(b[0]),
                       "counters_equal": bool(a[1] and b[1]), "pose_max_rel": max(a[2], b[2]), "chi2_max_rel": max(a[3], b[3]),
                       "lm_iterations_trials_device": [g1["lm_iterations"], g1["lm_trials"], g2["lm_iterations"], g2["lm_trials"]],
                       "lm_iterations_trials_oracle": [e1["lm_iterations"], e1["lm_trials"], e2["lm_iterations"], e2["lm_trials"]]}}


def secondary_block(ctx, dev, repeats=5):
    """PO / MATCH / LBA-A / single call.  Every figure: `repeats` timed runs (min / median / max - the spread is what round 2's
    unexplained -22 % / -8 % between two single-shot runs lacked), HIP-event time of the kernel on the library's stream, its ruler, the
    CPU oracle on a bounded sample of the same inputs, and a parity check of the first item against the oracle."""
    import numpy as np
    import torch
    import oracle_py as O
    from lld_slam_amd import BABatch, Optimizer, PoseBatch, synth
    timer = StreamTimer(ctx)
    out = {}

    # ---- PoseOptimization: 4096 frames of 1000 stereo points + 200 stereo lines (400 line edges), gamma 0.5, 4 x 10 LM iterations
    nf = 4096
    distinct = [synth.make_pose_frame(i) for i in range(64)]
    frames = (distinct * (nf // 64))[:nf]
    with PoseBatch(ctx, frames, gamma=0.5) as b:
        b.solve(); ctx.synchronize()
        ms = [timer.time_ms(b.solve) for _ in range(repeats)]
        res = [b.download(i) for i in range(64)]
    tc = time.perf_counter(); ores = [O.pose_opt(f, gamma=0.5) for f in distinct[:16]]; cpu_s = time.perf_counter() - tc
    med = float(np.median(ms)) * 1e-3
    fma = sum(pose_fmas(f.n_points, int(f.n_lines + np.count_nonzero(f.ln_right[:, 0] >= 0)), r.lm_iterations, r.lm_trials) for f, r in zip(distinct, res)) / 64.0
    model_bytes = 68e3 * 2 * float(np.mean([r.lm_iterations for r in res]))          # 68 KB edge scan x 2 passes x iterations
    out["pose_opt"] = {
        "workload": f"{nf} PO frames resident (64 distinct x {nf // 64}), 1000 stereo point + 400 line edges each, 4 x 10 LM iterations",
        "value": round(nf / med, 1), "unit": "frames/s", "kernel": "pose_opt_kernel", "launch_ms": _spread(ms),
        "roofline": {"bound": "fp64_fma", "achieved": round(fma * nf / med / 1e12, 3), "peak": FP64_FMA_PEAK_T, "unit": "TFMA/s",
                     "frac": round(fma * nf / med / 1e12 / FP64_FMA_PEAK_T, 4), "fma_per_frame": int(fma),
                     "hbm_model": {"bytes_per_frame": int(model_bytes), "achieved_GBps": round(model_bytes * nf / med / 1e9, 1), "frac_of_8TBps": round(model_bytes * nf / med / 1e9 / HBM_PEAK_GBS, 4),
                                   "note": "the kernel keeps a frame in LDS: it moves 68 KB per frame once, not once per sweep"},
                     "counters": _secondary_rulers("pose_opt_kernel<true, float, 256>"), "counters_single_frame": _secondary_rulers("pose_opt_kernel<true, float, 512>")},
        "cpu_baseline": {"value": round(16 / cpu_s, 2), "unit": "frames/s", "cores": 1, "kind": "port", "sample": "16 PO frames through oracle/liblld_oracle.so"},
        "parity": {"frames_checked": 16, "inliers_equal": bool(all(r.n_inliers == o.n_inliers and np.array_equal(r.pt_outlier, o.pt_outlier) for r, o in zip(res, ores))),
                   "max_rel_chi2": float(max(abs(r.chi2 - o.chi2) / max(o.chi2, 1e-300) for r, o in zip(res, ores)))},
    }

    # ---- ORB 2000 x 2000 x 256 bit and LBD 300 x 300 x 72 float, 1024 frame pairs resident
    B = 1024
    nq = nt = 2000
    qs, ts = zip(*[synth.make_match_orb(i, nq, nt) for i in range(8)])
    q = torch.from_numpy(np.stack(qs * (B // 8)).view(np.int32)).to(dev); tt = torch.from_numpy(np.stack(ts * (B // 8)).view(np.int32)).to(dev)
    outs = [torch.empty((B, nq), dtype=torch.int32, device=dev) for _ in range(4)]
    fn = ctx.lib.fn("match_hamming256_batch_dev")
    def run_orb():
        assert fn(ctx.handle, B, q.data_ptr(), nq, tt.data_ptr(), nt, *[o.data_ptr() for o in outs]) == 0
    torch.cuda.synchronize(); run_orb(); ctx.synchronize()
    ms = [timer.time_ms(run_orb) for _ in range(repeats)]
    tc = time.perf_counter(); e = O.match_hamming256(qs[0], ts[0]); cpu_s = time.perf_counter() - tc
    med = float(np.median(ms)) * 1e-3
    lane_ops = 16.0 * nq * nt                                   # 8 x (v_xor_b32 + v_bcnt_u32_b32 accumulate) per descriptor pair
    out["orb_hamming256"] = {
        "workload": f"{B} frame pairs resident (8 distinct x {B // 8}), {nq} x {nt} 256-bit ORB descriptors, best + second best per query",
        "value": round(B / med, 1), "unit": "frame pairs/s", "kernel": "hamming256_best2_kernel", "launch_ms": _spread(ms),
        "roofline": {"bound": "valu_int32", "achieved": round(lane_ops * B / med / 1e12, 3), "peak": VALU32_PEAK_T, "unit": "T lane-ops/s",
                     "frac": round(lane_ops * B / med / 1e12 / VALU32_PEAK_T, 4), "lane_ops_per_pair": int(lane_ops),
                     "hbm_model": {"bytes_per_pair": 152000, "achieved_GBps": round(152e3 * B / med / 1e9, 1), "frac_of_8TBps": round(152e3 * B / med / 1e9 / HBM_PEAK_GBS, 5)},
                     "counters": _secondary_rulers("hamming256_best2_kernel")},
        "cpu_baseline": {"value": round(1 / cpu_s, 2), "unit": "frame pairs/s", "cores": 1, "kind": "port", "sample": "1 frame pair through oracle/liblld_oracle.so"},
        "parity": {"bit_exact": bool(all(np.array_equal(o[0].cpu().numpy(), x) for o, x in zip(outs, e)))},
    }
    del q, tt, outs
    n1 = n2 = 300; D = 72
    ql, tl = zip(*[synth.make_match_lbd(i, n1, n2, D) for i in range(8)])
    q2 = torch.from_numpy(np.stack(ql * (B // 8))).to(dev); t2 = torch.from_numpy(np.stack(tl * (B // 8))).to(dev)
    bi = torch.empty((B, n1), dtype=torch.int32, device=dev); si = torch.empty_like(bi)
    bd = torch.empty((B, n1), dtype=torch.float64, device=dev); sd = torch.empty_like(bd)
    fn2 = ctx.lib.fn("match_l2f32_batch_dev")
    def run_lbd():
        assert fn2(ctx.handle, B, q2.data_ptr(), n1, t2.data_ptr(), n2, D, bi.data_ptr(), bd.data_ptr(), si.data_ptr(), sd.data_ptr()) == 0
    torch.cuda.synchronize(); run_lbd(); ctx.synchronize()
    ms = [timer.time_ms(run_lbd) for _ in range(repeats)]
    tc = time.perf_counter(); e2 = O.match_l2f32(ql[0], tl[0]); cpu_s = time.perf_counter() - tc
    med = float(np.median(ms)) * 1e-3
    fma2 = float(n1 * n2 * D)                                   # one fp32 subtract + one fp64 FMA per component
    out["lbd_l2f32"] = {
        "workload": f"{B} frame pairs resident (8 distinct x {B // 8}), {n1} x {n2} LBD descriptors of {D} floats, float L2 accumulated in fp64 in index order",
        "value": round(B / med, 1), "unit": "frame pairs/s", "kernel": "l2f32_best2_kernel", "launch_ms": _spread(ms),
        "roofline": {"bound": "fp64_fma", "achieved": round(fma2 * B / med / 1e12, 3), "peak": FP64_FMA_PEAK_T, "unit": "TFMA/s", "frac": round(fma2 * B / med / 1e12 / FP64_FMA_PEAK_T, 4),
                     "fma_per_pair": int(fma2),
                     "hbm_model": {"bytes_per_pair": 176000, "achieved_GBps": round(176e3 * B / med / 1e9, 1), "frac_of_8TBps": round(176e3 * B / med / 1e9 / HBM_PEAK_GBS, 5)},
                     "counters": _secondary_rulers("l2f32_best2_kernel")},
        "cpu_baseline": {"value": round(1 / cpu_s, 2), "unit": "frame pairs/s", "cores": 1, "kind": "port", "sample": "1 frame pair through oracle/liblld_oracle.so"},
        "parity": {"bit_exact": bool(np.array_equal(bi[0].cpu().numpy(), e2[0]) and np.array_equal(bd[0].cpu().numpy(), e2[1]))},
    }
    del q2, t2, bi, si, bd, sd

    # ---- LBA-A: 20 KF / 5k points / 1k lines (40k edges), 128 windows resident
    nla = 128
    wa = synth.generate_windows(0, 16, maker=synth.make_lba_a)
    wa = (wa * (nla // 16))[:nla]
    with BABatch(ctx, wa) as b:
        b.solve()
        wall = []
        for _ in range(repeats):
            t0 = time.perf_counter(); b.solve(); wall.append((time.perf_counter() - t0) * 1e3)
        st = b.stats(); ga = b.download(0)
        b.set_groups(1); b.set_phase_timing(True); b.solve(); ph = b.phase_ms(); b.set_phase_timing(False); b.set_groups(0)
    tc = time.perf_counter(); oa = [O.local_ba(w) for w in wa[:2]]; cpu_s = time.perf_counter() - tc
    med = float(np.median(wall)) * 1e-3
    per = {k: 0 for k in PHASES}
    for w, s in zip(wa, st):
        ab = algorithmic_bytes(w, sum(s["lm_trials"]), sum(s["lm_iterations"]), s["pcg_iterations"])
        for k in PHASES:
            per[k] += ab[k]
    kdom = int(np.argmax(ph[:5])); kname = PHASES[kdom]
    ach = per[kname] / (ph[kdom] * 1e-3) / 1e9
    out["local_ba_lba_a"] = {
        "workload": f"{nla} LBA-A windows resident (16 distinct x {nla // 16}), 20 free + 5 fixed KF, 5k points x 6, 1k lines x 5 x 2 = 40k edges",
        "value": round(nla / med, 1), "unit": "windows/s", "solve_ms": _spread(wall),
        # no HBM counters were collected for this batch shape, and the headline's rule withdraws the SURVEY byte model for the Schur family (it charges
        # point Hpl blocks the kernels recompute: model > 1.5 x counters on LBA-B) - so no `frac` is claimed here; the model figure stays as a named
        # secondary, the family split of the step is what this entry measures
        "roofline": {"bound": None, "kernel": kname, "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None,
                     "model_only": {"achieved_GBps": round(ach, 1), "frac_of_8TBps": round(ach / HBM_PEAK_GBS, 4), "note": "SURVEY 8d byte model; withdrawn as a ruler (see the headline's families: model_over_counter)"},
                     "phase_ms_single_stream_step": {k: round(float(ph[i]), 3) for i, k in enumerate(PHASES)}},
        "cpu_baseline": {"value": round(2 / cpu_s, 3), "unit": "windows/s", "cores": 1, "kind": "port", "sample": "2 LBA-A windows through oracle/liblld_oracle.so"},
        "parity": {"max_rel_chi2_final": float(abs(ga.stats["chi2_final"] - oa[0].stats["chi2_final"]) / oa[0].stats["chi2_final"]),
                   "outlier_sets_identical": bool(np.array_equal(ga.pt_obs_outlier, oa[0].pt_obs_outlier) and np.array_equal(ga.line_removed, oa[0].line_removed))},
    }

    # ---- what ONE LocalMapping-thread call sees: lld_local_ba on one LBA-B window, host buffers in and out
    wb = synth.make_lba_b(0)
    opt = Optimizer(ctx)
    opt.LocalBundleAdjustment(wb)
    ts_ = []
    for _ in range(repeats):
        t0 = time.perf_counter(); opt.LocalBundleAdjustment(wb); ts_.append((time.perf_counter() - t0) * 1e3)
    laps = {"create_ms": [], "solve_ms": [], "download_ms": []}
    for _ in range(repeats):
        t0 = time.perf_counter(); b1 = BABatch(ctx, [wb]); t1 = time.perf_counter(); b1.solve(); t2 = time.perf_counter(); b1.download(0); t3 = time.perf_counter(); b1.close()
        laps["create_ms"].append((t1 - t0) * 1e3); laps["solve_ms"].append((t2 - t1) * 1e3); laps["download_ms"].append((t3 - t2) * 1e3)
    out["single_window_call"] = {"workload": "lld_local_ba on one LBA-B window through the Python mirror, host buffers in and out (one window cannot fill the GPU: ~21 dependent super-steps)",
                                 "local_ba_ms": _spread(ts_), "phases_through_the_batch_api": {k: round(float(np.median(v)), 3) for k, v in laps.items()}}
    return out


# ================================================================================================== --dump-outputs
DUMP_BYTES_MAX = 64 * 10 ** 6       # every file of one dump together, .npy headers included
DUMP_SAMPLE_SEED = 0x0D0D


def dump_outputs(path, batch):
    """What the last solve handed its caller (lld_ba_batch_download_range over the batch) as DIR/<name>.npy: float64, the 0/1 outlier flags float32.
    Poses and statistics of every window; landmarks, lines and outlier flags of a seeded sample of windows (sample_window_ids.npy), as many
    as fit in DUMP_BYTES_MAX.  Per-window arrays are concatenated along their first axis in window order."""
    import numpy as np
    outs = batch.download_all()
    stats = [o.stats for o in outs]
    files = {"cam_qt": np.concatenate([o.cam_qt for o in outs])}
    for k in stats[0]:
        files["stats_" + k] = np.array([s[k] for s in stats], dtype=np.float64)

    def window_arrays(o):
        return {"pt_xyz": o.pt_xyz, "line_x0": o.line_x0, "line_dir": o.line_dir, "pt_obs_outlier": o.pt_obs_outlier.astype(np.float32),
                "ln_edge_outlier": o.ln_edge_outlier.astype(np.float32), "line_removed": o.line_removed.astype(np.float32)}
    header = 128
    used = sum(a.nbytes + header for a in files.values()) + 7 * header + 8 * len(outs)     # + the sampled files' headers and the id list
    ids = []
    for i in np.random.default_rng(DUMP_SAMPLE_SEED).permutation(len(outs)):
        nb = sum(a.nbytes for a in window_arrays(outs[i]).values())
        if used + nb > DUMP_BYTES_MAX:
            break
        used += nb; ids.append(int(i))
    if not ids:
        raise SystemExit(f"--dump-outputs: not even one window's landmarks fit in {DUMP_BYTES_MAX} bytes")
    ids.sort()
    files["sample_window_ids"] = np.array(ids, dtype=np.float64)
    per = [window_arrays(outs[i]) for i in ids]
    for k in per[0]:
        files[k] = np.concatenate([p[k] for p in per])
    os.makedirs(path, exist_ok=True)
    for k, a in files.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(a))
    return {"dir": path, "files": len(files), "bytes": sum(os.path.getsize(os.path.join(path, k + ".npy")) for k in files), "windows": len(outs), "sampled_windows": len(ids)}


# ================================================================================================== host buffers in -> results out
def e2e_block(windows, device, lanes=3, batches_per_lane=16):
    """Steady-state rate at the C ABI with HOST buffers on both sides: `lanes` host threads, each with its own context, loop
    lld_ba_batch_create -> lld_ba_batch_solve -> lld_ba_batch_download_range -> lld_ba_batch_destroy on the same 256 host windows.
    Flattening + upload of one lane's next batch and the download of its previous one overlap the other lane's solve (solves of large
    batches take turns on a device, lld_ba.hip; a batch created while another one solves gets two stream groups instead of four, which leaves
    the other lanes' copies room next to the solve).  One untimed warm-up batch per lane (first touch of the pinned arenas, slab growth).
    `e2e_windows_per_s` is from a STANDING start (all lanes begin with a create, the device idles for the first ~60 ms) to the last download;
    `steady_state_windows_per_s` starts once every lane has one batch behind it."""
    import ctypes as C
    import threading
    import numpy as np
    from lld_slam_amd import Context, abi, host
    lib = abi.product()
    nw = len(windows)
    cw = (abi.BAWindow * nw)(*[w.to_c() for w in windows])
    params = host.ba_params(lib)
    laps = np.zeros((lanes, 3)); t_done = [0.0] * lanes; t_first = [0.0] * lanes; chi = [0.0] * lanes
    ready = threading.Barrier(lanes + 1); go = threading.Barrier(lanes + 1)

    def one(ctx, crs, acc):
        h = C.c_void_p(); flag = C.c_int(0)
        t0 = time.perf_counter()
        host.check(lib.fn("ba_batch_create")(ctx.handle, nw, cw, C.byref(params), C.byref(h)), "ba_batch_create")
        t1 = time.perf_counter()
        host.check(lib.fn("ba_batch_solve")(h, C.byref(flag)), "ba_batch_solve")
        t2 = time.perf_counter()
        host.check(lib.fn("ba_batch_download_range")(h, 0, nw, crs), "ba_batch_download_range")
        lib.fn("ba_batch_destroy")(h)
        t3 = time.perf_counter()
        if acc is not None:
            acc += [t1 - t0, t2 - t1, t3 - t2]

    def lane(k):
        ctx = Context(device)
        outs = [host.BAOutput.alloc(w) for w in windows]
        crs = (abi.BAResult * nw)(*[o.to_c() for o in outs])
        one(ctx, crs, None)                        # warm-up
        ready.wait(); go.wait()
        for b_ in range(batches_per_lane):
            one(ctx, crs, laps[k])
            if b_ == 0: t_first[k] = time.perf_counter()
        t_done[k] = time.perf_counter(); chi[k] = crs[nw - 1].stats.chi2_final
        ctx.close()

    th = [threading.Thread(target=lane, args=(k,)) for k in range(lanes)]
    for t in th: t.start()
    ready.wait(); t0 = time.perf_counter(); go.wait()
    for t in th: t.join()
    el = max(t_done) - t0
    nb = lanes * batches_per_lane
    m = laps.sum(0) / nb * 1e3
    steady = (nb - lanes) * nw / max(1e-9, max(t_done) - max(t_first)) if batches_per_lane > 1 else None      # once every lane has a batch behind it (no common standing start)
    return {"e2e_windows_per_s": round(nb * nw / el, 1), "steady_state_windows_per_s": None if steady is None else round(steady, 1), "batches": nb, "lanes": lanes, "windows_per_batch": nw, "elapsed_ms": round(el * 1e3, 1),
            "mean_ms_per_batch_in_a_lane": {"create_flatten_and_queue_upload": round(float(m[0]), 2), "solve_incl_waiting_for_the_upload_and_for_its_turn": round(float(m[1]), 2),
                                            "download_all_and_destroy": round(float(m[2]), 2)},
            "note": "host buffers in, results out, at the C ABI; `value` times resident windows.  The Python mirror (BABatch(ctx, windows)) adds its ctypes marshalling on top."}


# ================================================================================================== --full: roofline, CPU baseline
def roofline_block(windows, stats, phase, launches, step_s, stream_gbs):
    """Roofline of the dominant kernel family (HIP events of the single-stream roofline pass, recorded on the library's own stream) and
    both rulers of every other family.  `step_s`: seconds per timed step; `stream_gbs`: copy_ceiling_gbs()."""
    import numpy as np
    wpg = len(windows)
    per = {k: 0 for k in PHASES}
    for w, s in zip(windows, stats):
        ab = algorithmic_bytes(w, sum(s["lm_trials"]), sum(s["lm_iterations"]), s["pcg_iterations"])
        for k in PHASES:
            per[k] += ab[k]
    kdom = int(np.argmax(phase[:5])); kname = PHASES[kdom]
    traffic_tab = _traffic_table() if wpg == 256 else {}          # the committed counters were collected on 256-window launches
    issue_tab = _issue_table() if wpg == 256 else {}
    def rulers(k):
        i = PHASES.index(k); ms_k = float(phase[i]); n = max(float(launches[i]), 1.0)
        if ms_k <= 0:
            return None
        model = per[k] / (ms_k * 1e-3) / 1e9
        r = {"avg_launch_ms": round(ms_k / n, 4), "model_bytes_per_launch": int(per[k] / n), "model_GBps": round(model, 1), "model_frac_of_8TBps": round(model / HBM_PEAK_GBS, 4)}
        tb = traffic_tab.get(k)
        if tb:
            cnt = tb / (ms_k / n * 1e-3) / 1e9
            r.update({"counter_bytes_per_launch": int(tb), "counter_GBps": round(cnt, 1), "counter_frac_of_8TBps": round(cnt / HBM_PEAK_GBS, 4),
                      "counter_frac_of_6.3TBps_achievable": round(cnt / HBM_ACHIEVABLE_GBS, 4), "model_over_counter": round(per[k] / n / tb, 3)})
        iq = issue_tab.get(k)
        if iq:
            # the compute ruler that exists for EVERY family (round 6): VALU instructions the counters saw per launch against the issue peak of
            # one instruction per 4 clocks and SIMD, and how busy the LDS pipe was - next to the HBM ruler, the larger of the two names the
            # resource the family is closest to
            t_launch = ms_k / n * 1e-3
            r["valu_issue_frac"] = round(iq["SQ_INSTS_VALU"] * 4.0 / (1024 * t_launch * 2.4e9), 4)
            r["lds_pipe_busy_frac"] = round(iq["SQ_LDS_IDX_ACTIVE"] / (256 * t_launch * 2.4e9), 4)
            r["lds_bank_conflict_of_lds_cycles"] = round(iq["SQ_LDS_BANK_CONFLICT"] / max(iq["SQ_LDS_IDX_ACTIVE"], 1.0), 4)
            cand = {"valu_issue": r["valu_issue_frac"], "lds_pipe": r["lds_pipe_busy_frac"], "hbm": r.get("counter_frac_of_8TBps") or 0.0}
            r["closest_ruler"] = max(cand, key=cand.get)
        if tb and per[k] / n / tb > 1.5:
            # the SURVEY model charges this family bytes its kernels do not move (point Hpl blocks are recomputed, not stored): the
            # model ruler would print an impossible fraction of the peak - it is withdrawn here, the counter ruler stands
            r["model_frac_of_8TBps"] = None
            r["model_ruler"] = "invalid for this family (model bytes > 1.5 x the bytes the HBM counters saw); use the counter ruler"
        return r
    fam = {k: rulers(k) for k in PHASES if k != "ba_control"}
    dom = fam[kname]
    # HBM ruler of the dominant family: the bytes the counters SAW (per launch, committed passes) over this run's HIP-event time, against the
    # 8 TB/s of the data sheet; the SURVEY model (which charges every point edge a 144 B block the kernels recompute) stays beside it
    hbm = {"achieved": dom.get("counter_GBps"), "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": None if "counter_GBps" not in dom else round(dom["counter_GBps"] / HBM_PEAK_GBS, 4), "source": "counters" if "counter_GBps" in dom else None,
           "frac_of_6.3TBps_achievable": dom.get("counter_frac_of_6.3TBps_achievable"),
           "model": {"achieved": dom["model_GBps"], "frac": round(dom["model_GBps"] / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": dom["model_bytes_per_launch"],
                     "note": "SURVEY 8d bytes: W + V + S per launch; charges point Hpl blocks the kernel does not move"}}
    if hbm["achieved"] is None:                      # no counters for this batch size: the model is all there is
        hbm.update({"achieved": dom["model_GBps"], "frac": round(dom["model_GBps"] / HBM_PEAK_GBS, 4), "source": "model"})
    # the whole step: counter bytes of every family x its launches in the single-stream step, over the TIMED step
    step_ruler = None
    if traffic_tab:
        step_bytes = sum(float(traffic_tab.get(k, 0)) * float(launches[i]) for i, k in enumerate(PHASES)) + float(traffic_tab.get("_other_per_solve", 0))
        step_gbs = step_bytes / step_s / 1e9
        step_ruler = {"counter_bytes_per_step": int(step_bytes), "achieved_GBps": round(step_gbs, 1), "frac_of_8TBps": round(step_gbs / HBM_PEAK_GBS, 4),
                      "note": "sum over the kernel families of (counter bytes per launch x launches of the single-stream step) / ms_per_step of the timed steps"}
    roofline = {"kernel": kname, "traffic": dom.get("counter_bytes_per_launch"),
                "traffic_source": None if not traffic_tab else "profiles/roofline_traffic.json (" + str(traffic_tab.get("_taken_on", "see its _note")) + "): TCC FETCH_SIZE (doubled on gfx950) + WRITE_SIZE of separate "
                                  "rocprofv3 --pmc passes over `bench.py --windows-per-gpu 256` (tools/profile_pmc.sh + tools/make_roofline_traffic.py); NOT re-measured in this run "
                                  "(a bench process cannot run under --pmc and time itself)",
                "hbm": hbm, "step": step_ruler,
                "measured_copy_ceiling_GBps": stream_gbs,
                "launches_per_step": float(launches[kdom]), "avg_launch_ms": dom["avg_launch_ms"], "algorithmic_bytes_per_launch": dom["model_bytes_per_launch"],
                "families": fam,
                "rulers": "model = SURVEY §8d bytes (charges every point edge a 144 B Hpl block the kernels recompute instead of moving: where model_over_counter > 1 "
                          "the model ruler overstates traffic and the counter ruler is the honest one); counter = FETCH_SIZE (doubled on gfx950) + WRITE_SIZE of separate rocprofv3 --pmc passes",
                "phase_ms_single_stream_step": {k: round(float(phase[i]), 3) for i, k in enumerate(PHASES)},
                "solve_ms_single_stream_step": round(float(phase[5]), 3)}
    if kname == "ba_schur":
        # The ruler that BINDS this family is arithmetic (fp64 vector FMA; the blocks are 6x6 / 6x3 / 6x4, no matrix cores): it goes first.
        fma_total = sum(schur_fmas(w, sum(st_["lm_trials"])) for w, st_ in zip(windows, stats))
        tf = fma_total / (float(phase[kdom]) * 1e-3) / 1e12
        roofline.update({"bound": "fp64_fma", "achieved": round(2.0 * tf, 2), "peak": round(2.0 * FP64_FMA_PEAK_T, 1), "unit": "TFLOP/s", "frac": round(tf / FP64_FMA_PEAK_T, 4),
                         "fp64_fma": {"achieved_TFMA_per_s": round(tf, 2), "peak_TFMA_per_s": FP64_FMA_PEAK_T, "frac": round(tf / FP64_FMA_PEAK_T, 4),
                                      "note": "useful FMAs of the family (bench.schur_fmas) over its HIP-event time; vector fp64 peak = 256 CU x 4 SIMD x 16 lanes/clk x 2.4 GHz"}})
    else:
        roofline.update({"bound": "hbm", "achieved": hbm["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": hbm["frac"]})
    return roofline


def cpu_baseline_block(batch, windows, cpu_sample):
    """CPU baseline + matched-chi2 check (N=1 only): the single-threaded oracle on a bounded sample spread over the batch, its results against
    what the batch's last solve computed, then the same port with one window per host thread."""
    import numpy as np
    import oracle_py as O
    wpg = len(windows)
    O.lib()
    ns = min(cpu_sample, wpg)
    ids = sorted(set(int(round(i * (wpg - 1) / max(1, ns - 1))) for i in range(ns)))     # spread over the batch: every stream group is sampled
    tc = time.perf_counter(); ores = [O.local_ba(windows[i]) for i in ids]; cpu_s = time.perf_counter() - tc
    gres = [batch.download(i) for i in ids]
    rel = max(abs(g.stats["chi2_final"] - o.stats["chi2_final"]) / max(o.stats["chi2_final"], 1e-300) for g, o in zip(gres, ores))
    same = all(np.array_equal(g.pt_obs_outlier, o.pt_obs_outlier) and np.array_equal(g.ln_edge_outlier, o.ln_edge_outlier) and np.array_equal(g.line_removed, o.line_removed)
               for g, o in zip(gres, ores))
    # the same port with one window per host thread (the reference's g2o is single-threaded per window; ctypes drops the GIL)
    from concurrent.futures import ThreadPoolExecutor
    nthr = max(1, min(os.cpu_count() or 1, 32, wpg))
    tp = time.perf_counter()
    with ThreadPoolExecutor(nthr) as ex:
        list(ex.map(lambda i: O.local_ba(windows[i]), range(nthr)))
    par_s = time.perf_counter() - tp
    cpu = {"value": round(len(ids) / cpu_s, 4), "unit": "windows/s", "cores": 1, "kind": "port",
           "sample": f"{len(ids)} LBA-B windows (ids {ids}) through oracle/liblld_oracle.so, 1 thread, exact dense LDLT of the reduced system",
           "all_cores": {"value": round(nthr / par_s, 4), "cores": nthr, "sample": f"{nthr} windows, one per thread, concurrently"}}
    pose_err = max(float(np.max(np.abs(g.cam_qt - o.cam_qt)) / np.max(np.abs(o.cam_qt))) for g, o in zip(gres, ores))
    pt_err = np.concatenate([np.linalg.norm(g.pt_xyz - o.pt_xyz, axis=1) / np.linalg.norm(o.pt_xyz, axis=1) for g, o in zip(gres, ores)])
    parity = {"windows_checked": len(ids), "window_ids": ids, "max_rel_chi2_final": float(rel), "outlier_sets_identical": bool(same),
              "max_rel_pose": pose_err, "median_rel_point": float(np.median(pt_err)), "points_within_1e-5": float(np.mean(pt_err <= 1e-5))}
    return cpu, parity


def copy_ceiling_gbs(dev):
    """Measured stream ceiling of this GPU (SURVEY.md §8d asks for it next to the nominal 8 TB/s): a device-to-device copy of 2 GiB,
    bytes read + bytes written over the HIP-event time, best of 5."""
    import torch
    try:
        a = torch.empty(1 << 31, dtype=torch.uint8, device=dev); b = torch.empty_like(a)
        b.copy_(a); torch.cuda.synchronize()
        best = 1e30
        for _ in range(5):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        gbs = round(2.0 * a.numel() / (best * 1e-3) / 1e9, 1)
        del a, b
        return gbs
    except Exception:
        return None


# ================================================================================================== main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ramp-seconds", type=float, default=1.5, help="untimed solves before the warm-up steps until this much wall clock has passed (clock ramp of a fresh process; 0 = none)")
    ap.add_argument("--ramp-steps-max", type=int, default=60)
    ap.add_argument("--windows-per-gpu", type=int, default=256, help="windows per GPU (weak scaling); with --strong: windows in total")
    ap.add_argument("--strong", action="store_true", help="strong scaling: the same --windows-per-gpu windows split over the ranks (SURVEY §8d: 256 windows, 32 per GPU at 8)")
    ap.add_argument("--full", action="store_true", help="after the headline, measure and check everything else: roofline pass and copy ceiling, gathered-record check, "
                    "rccl_overhead, CPU baseline and parity, e2e, secondary configs (a plain run does none of these)")
    ap.add_argument("--cpu-sample", type=int, default=40, help="LBA-B windows timed on the CPU oracle (--full; rank 0, N=1 only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline and its parity block")
    ap.add_argument("--no-secondary", action="store_true", help="--full without the PO / MATCH / LBA-A / single-call block")
    ap.add_argument("--no-e2e", action="store_true", help="--full without the host-buffers-in / results-out pipeline (N=1 only anyway)")
    ap.add_argument("--e2e-lanes", type=int, default=3, help="host threads of the e2e leg of --full (solves take turns on the device; a third lane keeps a batch ready: 4250 -> 4490 windows/s)")
    ap.add_argument("--shared-accumulators", action="store_true", help="run the timed leg with lld_ba_params.deterministic = 0 (not bit-reproducible; the default is)")
    ap.add_argument("--groups", type=int, default=0, help="stream groups of the timed solves (0 = the library's choice; 1 under rocprofv3: per-kernel times of one stream)")
    ap.add_argument("--gen-workers", type=int, default=0, help="processes generating the synthetic windows (0 = auto; use 1 under rocprofv3)")
    ap.add_argument("--no-rccl-check", action="store_true", help="--full at N = 1 without the untimed step through a one-rank RCCL group and rccl_overhead")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed (rank 0's windows) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(1, args.gpus) and world != 1:
        raise SystemExit(f"--gpus {args.gpus} does not match WORLD_SIZE {world}")

    from lld_slam_amd import dist as D, synth
    # the node's cores are shared by `world` ranks: staging threads of the library and generator processes are budgeted per rank
    budget = D.host_thread_budget(world)
    if world > 1:                                             # one rank per node: the library's own choice stands (16 threads, 4 while a solve runs on the device)
        os.environ.setdefault("LLD_HOST_THREADS", str(budget))

    # ---- synthetic windows for this rank (generated before anything touches the GPU)
    first, wpg = D.shard(args.windows_per_gpu, world, rank, args.strong)
    if min(D.shard(args.windows_per_gpu, world, r, args.strong)[1] for r in range(world)) < 1:
        raise SystemExit("fewer windows than ranks")          # every rank sees the same shard table: all leave here, none enters a collective alone
    workers = args.gen_workers if args.gen_workers > 0 else budget
    t0 = time.time()
    windows = synth.generate_windows(first, wpg, workers)
    gen_s = time.time() - t0

    import numpy as np
    import torch
    import torch.distributed as dist
    from lld_slam_amd import BABatch, Context

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # LLD_BENCH_FORCE_DIST=1 takes the RCCL path even with one rank (checks the collective plumbing on a 1-GPU box)
    use_dist = world > 1 or os.environ.get("LLD_BENCH_FORCE_DIST") == "1"
    saved_stdout = None
    if use_dist:
        # RCCL prints a version banner on stdout when its first communicator comes up: keep stdout for the one JSON line
        sys.stdout.flush(); saved_stdout = os.dup(1); os.dup2(2, 1)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if world == 1:                                          # LLD_BENCH_FORCE_DIST without a launcher: a one-rank group of our own
            for k_, v_ in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29577")):
                os.environ.setdefault(k_, v_)
        dist.init_process_group("nccl", device_id=dev)          # RCCL

    ctx = Context(local_rank)
    batch = BABatch(ctx, windows, gamma=1.0, deterministic=0 if args.shared_accumulators else 2)
    if args.groups > 0:
        batch.set_groups(args.groups)
    rec_ptr, rec_stride = batch.result_records()
    assert rec_stride == D.record_stride(windows), "record layout of lld_slam_amd/dist.py out of step with the library"
    rec_bytes = rec_stride * wpg

    class _Dev:                                                   # zero-copy torch view of the library's record buffer
        __cuda_array_interface__ = {"shape": (rec_bytes,), "typestr": "|u1", "data": (rec_ptr, False), "version": 2}
    records = torch.as_tensor(_Dev(), device=dev)
    counts = D.gather_counts(wpg, dev, use_dist, world)
    common_stride = D.max_count_stride(rec_stride, dev, use_dist)       # a batch's stride is its own largest record: the gather needs one for all ranks
    gather = D.RecordGather(records, world, rank, n_bytes=max(counts) * common_stride, enabled=use_dist, local_stride=rec_stride, common_stride=common_stride)

    def step():
        batch.solve()                     # synchronous on the library's stream (it polls the LM state every super-step)
        gather.step()                     # the final gather over xGMI, the only collective: asynchronous, overlaps the next solve

    # Clock ramp (untimed, before the W warm-up steps): a fresh process on an idle GPU runs its first second of solves 8 - 10 % slower (the window
    # generation above leaves the GPU idle for seconds; power management, cold TLBs and the first touch of the batch's work slab) - measured on fresh
    # boxes: 6.2 k windows/s for W = 1 straight after start-up against 6.8 k - 6.9 k a second later on the same box.  Reported in config.ramp.
    ramp_steps, ramp_t0 = 0, time.perf_counter()
    while ramp_steps < args.ramp_steps_max and time.perf_counter() - ramp_t0 < args.ramp_seconds:
        batch.solve(); ramp_steps += 1       # the solve alone: the number of ramp steps is decided by each rank's own clock, so no collective may sit in this loop
    ramp_s = time.perf_counter() - ramp_t0
    D.barrier(use_dist, True)
    for _ in range(args.warmup):
        step()
    gather.drain()
    D.barrier(use_dist, True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    gather.drain()                        # the last gather is inside the timed region
    D.barrier(use_dist, True)
    elapsed = time.perf_counter() - t0
    dumped = dump_outputs(args.dump_outputs, batch) if args.dump_outputs and rank == 0 else None     # before any further solve overwrites them
    phase = launches = stream_gbs = None
    if args.full:
        # Roofline pass (untimed): the timed steps keep several window groups in flight on separate streams, so their HIP-event
        # brackets overlap; one more step with a single group gives disjoint per-kernel-family event times on that stream.
        # Per-phase events are off in the timed steps, as in the product's default (lld_ba_batch_set_phase_timing: six event records per
        # super-step cost 1.6 % of a 256-window solve and 10 - 15 % of a small batch's); this pass turns them on.
        batch.set_groups(1); batch.set_phase_timing(True)
        batch.solve()
        phase = batch.phase_ms()
        launches = np.array([batch.kernel_stats(k)[0] for k in range(5)], dtype=np.float64)
        batch.set_phase_timing(False); batch.set_groups(args.groups)
        if rank == 0:
            stream_gbs = copy_ceiling_gbs(dev)
    elapsed = D.max_over_ranks(elapsed, dev, use_dist)

    stats = batch.stats()
    # --full, one rank, no launcher: the timed steps above had no collective to run.  ONE untimed step now goes through a one-rank RCCL group - the
    # same RecordGather the N > 1 line times, the same check of the gathered records - so that the driver's N = 1 line says whether the
    # collective path works on this box (`gathered_records_ok`), not null.  Failing to bring RCCL up must not cost the headline line.
    late_gather = None
    pg_inited = use_dist                                          # a process group we must destroy, whatever happens after its creation
    rccl_overhead = None
    if args.full and world == 1 and not use_dist and not args.no_rccl_check:
        try:
            sys.stdout.flush(); saved_stdout = os.dup(1); os.dup2(2, 1)          # (RCCL's banner goes to stderr)
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            for k_, v_ in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29577")):
                os.environ.setdefault(k_, v_)
            dist.init_process_group("nccl", device_id=dev)
            pg_inited = True
            late_counts = D.gather_counts(wpg, dev, True, 1)
            late_stride = D.max_count_stride(rec_stride, dev, True)
            late = D.RecordGather(records, 1, 0, n_bytes=max(late_counts) * late_stride, enabled=True, local_stride=rec_stride, common_stride=late_stride)
            batch.set_groups(args.groups); batch.solve(); late.step(); late.drain()
            D.barrier(True, True)
            late_gather = (late, late_counts, late_stride)
            # ... and the proxy of what N > 1 ranks pay for the collective: the SAME K timed steps once more with the gather of
            # every step started behind its solve (asynchronous, overlapping the next solve's stream groups - exactly the N > 1 step), against
            # the plain K steps timed above on this box.  rccl_overhead = rate with the gather / rate without.
            # Three alternating pairs right here (K steps with the gather, K plain), medians: a single pair against the timed region above moved between
            # 0.90 and 1.09 from run to run (the headline's K steps are a second old by now).
            with_g, plain = [], []
            for _ in range(3):
                t0g = time.perf_counter()
                for _ in range(args.steps):
                    batch.solve(); late.step()
                late.drain(); D.barrier(True, True)
                with_g.append(time.perf_counter() - t0g)
                t0p = time.perf_counter()
                for _ in range(args.steps):
                    batch.solve()
                D.barrier(True, True)
                plain.append(time.perf_counter() - t0p)
            rccl_overhead = {"value": round(float(np.median(plain) / np.median(with_g)), 4), "what": "windows/s of K steps with the asynchronous one-rank RCCL gather of every "
                             "step's records inside the timed region / windows/s of K plain steps (same box, same batch; medians of three alternating pairs)", "steps": args.steps,
                             "seconds_with_gather": [round(x, 4) for x in with_g], "seconds_plain": [round(x, 4) for x in plain]}
        except Exception as ex:
            print(f"[bench] one-rank RCCL check skipped: {ex!r}", file=sys.stderr)
            late_gather = None
    result = None
    if rank == 0:
        # every rank's records arrived AND are the windows shard() assigned: per rank, the first and the last record are checked against
        # the window id of their slot (index + edge count in the header, fixed cameras bit for bit against the generator), all headers
        # for a finished protocol (--full)
        gathered_ok = None
        if late_gather is not None:                        # N = 1: the untimed one-rank RCCL step above
            gather, counts_g, common_stride = late_gather[0], late_gather[1], late_gather[2]
            assert counts_g == counts
        if args.full and (use_dist or late_gather is not None):
            gathered_ok = True
            try:
                D.verify_gathered_records(gather.rank_records, counts, common_stride, args.windows_per_gpu, world, args.strong, synth.make_lba_b)
            except AssertionError as ex:
                gathered_ok = False; print(f"[bench] gathered records: {ex}", file=sys.stderr)
            for r in range(world):
                buf = gather.rank_records(r)
                for k in range(counts[r]):
                    h = D.RECORD_HEADER.unpack_from(buf[k * common_stride:k * common_stride + D.RECORD_HEADER.size].tobytes())
                    gathered_ok = bool(gathered_ok and np.isfinite(h[1]) and h[1] > 0 and h[2] >= 1 and h[8] == k)
        total_windows = sum(counts) * args.steps
        value = total_windows / elapsed
        roofline = cpu = parity = None
        if args.full:
            roofline = roofline_block(windows, stats, phase, launches, elapsed / args.steps, stream_gbs)
            if world == 1 and not args.no_cpu_baseline and args.cpu_sample > 0:
                cpu, parity = cpu_baseline_block(batch, windows, args.cpu_sample)
        result = {
            "metric": METRIC, "value": round(value, 3), "unit": "windows/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "full": args.full,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "strong" if args.strong else "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"batched LocalBundleAdjustment, {'%d LBA-B windows in total' % sum(counts) if args.strong else '%d LBA-B windows per GPU' % wpg} "
                                   f"(50 free + 10 fixed KF, 10k points x 6 stereo obs, 2k lines x 5 KF x 2 images = 80k edges), 5+15 LM iterations, gamma=1; "
                                   f"windows resident in HBM, every step restarts from the uploaded state",
                       "bit_reproducible": not args.shared_accumulators, "windows_per_gpu": counts if args.strong else wpg, "edges_per_window": int(windows[0].n_edges()),
                       "parallelism": f"{world} x independent window batches, RCCL gather of result records", "resident": True,
                       "result_record_bytes": int(rec_stride), "generate_s": round(gen_s, 1), "ramp": {"untimed_solves_before_the_warmup_steps": ramp_steps, "seconds": round(ramp_s, 2)}, "host_threads_per_rank": budget, "gathered_records_ok": gathered_ok,
                       "gathered_records_how": ("RCCL gather inside every timed step" if use_dist else ("one untimed step through a one-rank RCCL group after the timed region" if late_gather is not None else None))},
            "roofline": roofline, "cpu_baseline": cpu, "parity": parity,
            "lm": {"mean_trials_per_window": float(np.mean([sum(s["lm_trials"]) for s in stats])),
                   "mean_pcg_iterations_per_trial": float(np.sum([s["pcg_iterations"] for s in stats]) / max(1, np.sum([sum(s["lm_trials"]) for s in stats])))},
            # what this line was measured on: N > 1 figures exist only when a multi-GPU node ran this script (the builder's box has one GPU)
            "n_gpus_measured": world,
            # one rank, measured: what the asynchronous RCCL gather of every step costs the solve it overlaps (null under a launcher: there the
            # gather IS inside `value`); DESIGN.md 5 states the policy that follows from it
            "rccl_overhead": rccl_overhead,
            "dumped_outputs": dumped,
        }
    batch.close()
    if args.full and world > 1 and not args.no_secondary:
        # every rank takes part (collectives inside); rank 0 keeps the figures
        try:
            sec = sharded_secondary(ctx, dev, world, rank)
        except Exception as ex:
            sec = {"error": repr(ex)[:300]}
        if rank == 0:
            result["secondary"] = sec
    if args.full and rank == 0 and world == 1 and not use_dist:
        if not args.no_e2e:
            try:
                result["e2e"] = e2e_block(windows, local_rank, lanes=max(1, args.e2e_lanes))
                by = {str(l): e2e_block(windows, local_rank, lanes=l, batches_per_lane=6)["e2e_windows_per_s"] for l in (1, 2) if l != args.e2e_lanes}
                by[str(max(1, args.e2e_lanes))] = result["e2e"]["e2e_windows_per_s"]
                result["e2e"]["by_lanes"] = by
            except Exception as ex:           # the headline line must not die with an auxiliary figure
                result["e2e"] = dict(result.get("e2e") or {}, error=repr(ex)[:300])
        if not args.no_secondary:
            try:
                result["secondary"] = secondary_block(ctx, dev)
                result["secondary"]["tracking_frame"] = tracking_frame_block(ctx)
                result["secondary"]["small_batch"] = small_batch_block(ctx, windows)
                result["secondary"]["deterministic"] = deterministic_block(ctx, windows)
            except Exception as ex:
                result["secondary"] = dict(result.get("secondary") or {}, error=repr(ex)[:300])
    ctx.close()
    if pg_inited:
        try:
            dist.barrier()
        finally:
            dist.destroy_process_group()
    if saved_stdout is not None:
        sys.stdout.flush()
        try:                                  # what native libraries (RCCL: "Librccl path : ...") left in the C stdio buffer goes where fd 1 points NOW
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        os.dup2(saved_stdout, 1); os.close(saved_stdout)
    if rank == 0:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
