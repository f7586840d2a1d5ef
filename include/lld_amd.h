/*
 * lld_amd.h — C ABI of the MI355X-native point+line local-BA / pose-optimisation /
 * descriptor-matching core.
 *
 * This is the drop-in boundary for the hot path of alexandervakhitov/lld-slam.  The
 * reference has no FFI layer: its boundary is a set of C++ static/member functions that
 * take live SLAM objects (include/Optimizer.h:49-50, include/ORBmatcher.h:41-83,
 * include/TwoFrameLineMatcher.h:31-42).  Each entry point below names the reference
 * function it stands in for; the host adapter that gathers KeyFrame/MapPoint/MapLine
 * state into these flat structs is sketched in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, caller-allocated buffers, `int` status return (0 ok, <0 error), no globals;
 *   - a context is bound to one HIP device and one stream; it is re-entrant per handle
 *     (one handle per host thread, as Tracking / LocalMapping each would own one);
 *   - all pointers in the *input* structs are HOST pointers unless the function name ends
 *     in `_dev`; batch handles keep their inputs resident in HBM between solves;
 *   - poses are world->camera, stored as 7 doubles (qx,qy,qz,qw,tx,ty,tz) exactly as
 *     g2o::SE3Quat holds them (Thirdparty/g2o/g2o/types/se3quat.h:47-48);
 *   - floating point parity target: 1e-5 relative on final chi2 / poses / landmarks,
 *     identical outlier sets; matcher indices and integer distances bit-exact.
 *
 * The same structs are consumed by the CPU oracle (oracle/lld_oracle.cpp, symbols
 * `lldo_*`), which is test infrastructure only.
 */
#ifndef LLD_AMD_H
#define LLD_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* liblld_amd.so is built with -fvisibility=hidden: only the declarations of this header are exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ------------------------------------------------------------------ status codes */
#define LLD_OK               0
#define LLD_ERR_INVALID     -1   /* bad argument / inconsistent sizes               */
#define LLD_ERR_NO_DEVICE   -2   /* no HIP device: the product path never falls back */
#define LLD_ERR_HIP         -3   /* a HIP runtime call failed                        */
#define LLD_ERR_ALLOC       -4
#define LLD_ERR_UNSUPPORTED -5   /* size outside the compiled limits                 */

const char* lld_status_string(int status);

/* ------------------------------------------------------------------ context */
typedef struct lld_ctx lld_ctx;

/* Binds to HIP device `device`, creates a private stream.  Fails with LLD_ERR_NO_DEVICE
 * when no GPU is visible (there is no CPU fallback). */
int  lld_ctx_create(int device, lld_ctx** out);
void lld_ctx_destroy(lld_ctx* ctx);
/* Stream the context launches on (hipStream_t as void*), so callers can record events. */
void* lld_ctx_stream(lld_ctx* ctx);
int  lld_ctx_synchronize(lld_ctx* ctx);
/* Threading and memory contract of a context.
 *   - ONE host thread drives a context at a time (Tracking and LocalMapping each own one).  Two threads on one handle are not
 *     supported; the one case the library guards is two lld_ba_batch_create calls racing for the cached resources below (the flag
 *     is taken with an atomic exchange: the loser gets private resources and frees them with its batch).
 *   - A context KEEPS what the batched local BA needs between batches, grow-only: the device slab of the largest batch created so
 *     far (3.4 GB for 256 LBA-B windows, 13 MB for one), two pinned upload arenas (1.1 GB for that batch), the pinned landing buffer
 *     of the result records (100 MB), the group streams and events.  lld_ba_batch_destroy does NOT return them - allocating and,
 *     worse, freeing them per batch (hipFree synchronises the device) was most of the cost of a pipelined caller.  At most one live
 *     batch per context borrows the cached set; a second live batch on the same context allocates its own and frees it on destroy.
 *   - lld_ctx_release_cache gives the cached memory back without destroying the context (e.g. after a one-off global BA, or when a
 *     pipelined caller goes idle).  It fails with LLD_ERR_INVALID while a live batch borrows the set; the next batch re-grows it.
 *   - Environment: the library reads exactly one variable, LLD_HOST_THREADS (host threads that flatten / unpack a batch, 1..64,
 *     default min(cores, 16)).  Experiment knobs exist only in the experiments build (make -C lld_slam_amd/csrc exp). */
int  lld_ctx_release_cache(lld_ctx* ctx);

/* ------------------------------------------------------------------ shared types */
typedef struct {
  double fx, fy, cx, cy;   /* pinhole; line edges use fx for both axes (LineOptimizer.cc:66-68) */
  double bf;               /* baseline * fx (KeyFrame::mbf)                                      */
} lld_camera;

/* Converter::toSE3Quat (src/Converter.cc:37-47): float 4x4 row-major Tcw -> SE3Quat 7-vector. */
void lld_se3_from_tcw_f32(const float* tcw16, double* qt7);
/* Converter::toCvMat(SE3Quat) (src/Converter.cc:49-70): SE3Quat -> float 4x4 row-major. */
void lld_se3_to_tcw_f32(const double* qt7, float* tcw16);
/* ORBextractor level table mvInvLevelSigma2 (src/ORBextractor.cc:416-430), float arithmetic. */
void lld_orb_inv_level_sigma2(float scale_factor, int n_levels, float* out);

/* ================================================================== local bundle adjustment
 * Stands in for Optimizer::LocalBundleAdjustment (src/Optimizer.cc:936-1388) from the point
 * where the local window has been collected (:938-1018) to the point where results are
 * written back (:1334-1386), including LineOptimizer::{AddLineMinimal,DisableOutliers,
 * GetLineData} (src/LineOptimizer.cc:39-201) and everything g2o does underneath.
 *
 * Window layout (the order is the reference's insertion order, so sums run the same way):
 *   cameras   [0,n_free_cams) are optimised, in ascending KeyFrame::mnId order (g2o orders
 *             unknowns by vertex id, sparse_optimizer.cpp:166-190); [n_free_cams,n_cams) are
 *             fixed (lFixedCameras and the mnId==0 keyframe, Optimizer.cc:1037-1063).
 *   points    each point owns a contiguous run of observations pt_obs_start[p]..[p+1]
 *             (the loop over MapPoint::GetObservations, Optimizer.cc:1107-1178).
 *             uR < 0 marks a monocular observation (Optimizer.cc:1119).
 *   lines     each line owns a run of (line,KF) observations ln_obs_start[l]..[l+1]
 *             (proj_map, Optimizer.cc:1189-1218); every observation yields a left-image edge
 *             and, when right xs >= 0, a right-image edge (LineOptimizer.cc:58-65).
 */
typedef struct {
  lld_camera cam;
  int32_t n_cams;
  int32_t n_free_cams;
  const double*  cam_qt;             /* [n_cams][7]                                           */

  int32_t n_points;
  const double*  pt_xyz;             /* [n_points][3]  (Converter::toVector3d of the f32 pos) */
  const int32_t* pt_obs_start;       /* [n_points+1]                                          */
  int32_t n_pt_obs;
  const int32_t* pt_obs_cam;         /* [n_pt_obs] camera index                               */
  const double*  pt_obs_uvr;         /* [n_pt_obs][3] u, v, uR (uR<0: mono)                   */
  const double*  pt_obs_inv_sigma2;  /* [n_pt_obs] mvInvLevelSigma2[octave] widened           */

  int32_t n_lines;
  const double*  line_x0;            /* [n_lines][3]  MapLine::GetMinimalPos                  */
  const double*  line_dir;           /* [n_lines][3]                                          */
  const int32_t* ln_obs_start;       /* [n_lines+1]                                           */
  int32_t n_ln_obs;
  const int32_t* ln_obs_cam;         /* [n_ln_obs]                                            */
  const double*  ln_obs_left;        /* [n_ln_obs][4] xs,ys,xe,ye of the left KeyLine         */
  const double*  ln_obs_right;       /* [n_ln_obs][4] right KeyLine; xs<0 -> no stereo match  */
  const int32_t* ln_obs_octave;      /* [n_ln_obs][2] octave of left / right KeyLine          */
} lld_ba_window;

typedef struct {
  double  gamma;            /* line weight; LocalMapping passes 1.0 (Optimizer.h:49)           */
  int32_t its_round1;       /* 5  (Optimizer.cc:1224); >= 1: optimize(0) evaluates no error, the classification that follows would read g2o's uninitialised _error (undefined in the reference) -> LLD_ERR_INVALID */
  int32_t its_round2;       /* 15 (Optimizer.cc:1273); >= 1 for protocol 0 */
  int32_t ln_filter;        /* 4  (LineOptimizer.h:90)                                         */
  int32_t max_trials;       /* 10 (maxTrialsAfterFailure, optimization_algorithm_levenberg.cpp:50) */
  double  pcg_rel_tol;      /* reduced-system PCG stops at |r|_M / |b|_M <= tol (GPU only)     */
  int32_t pcg_max_iter;     /* 0 -> 10 * 6 * n_free_cams                                        */
  int32_t reduced_solver;   /* GPU only: 0 = exact Cholesky (default; the reference factorises exactly,
                               linear_solver_eigen.h:94-124) on the fp64 matrix cores when 6*n_free <= 304 - along the
                               block structure of S in an elimination order chosen per window, as the reference's sparse
                               LDL^T does after computeSymbolicDecomposition (linear_solver_eigen.h:147-232), wherever the
                               symbolic factor fits the kernel (lld_ba_chol_plan), dense otherwise,
                               1 = block-Jacobi PCG, 2 = exact 6x6-block Cholesky on the vector ALUs,
                               3 = the matrix-core Cholesky over all tiles in the caller's camera order (round 4's default);
                               diagnostic: 4 = structure-following in the caller's camera order as ONE chain of tile columns,
                               5 = structure-following with the two-chain (separator) plan only, dense where none exists */
  int32_t protocol;         /* 0 = Optimizer::LocalBundleAdjustment: optimize(its_round1), outlier protocol, optimize(its_round2).
                               1 = Optimizer::BundleAdjustment / GlobalBundleAdjustment (src/Optimizer.cc:312-559) on the same
                                   kernels: ONE optimize(its_round1) call and nothing else - no classification, no line removal, all
                                   result flags 0; line edges carry identity information and the Huber delta thHuber3D/2
                                   (AddLineMinimalGlobal, :149-240), `gamma` and `ln_filter` are ignored.  The window holds the whole
                                   map: every keyframe but mnId==0 free.  Limits of this build: n_free_cams <= 170 per window in general,
                                   <= 8192 when the batch has at most 8 windows (then the reduced system - dense, 6 n_free squared
                                   doubles of HBM - is solved by the multi-workgroup PCG whatever `reduced_solver` says, except 2;
                                   beyond 590 cameras the camera accumulators and pose copies of the landmark kernels live in HBM
                                   instead of LDS and are summed with global fp64 atomics: results of such maps are reproducible
                                   to rounding, not bit for bit, from run to run; parity-tested to 600 free cameras, timed to 4000) */
  int32_t robust_points;    /* protocol 1 only: bRobust (Huber kernels on the point edges, default 1); lines are always robust */
  int32_t abort_after_trials; /* TEST HOOK, 0 = off: behave as if *abort_flag had been raised right after the k-th LM trial of the
                               window (trials counted over both rounds) and stayed up - a deterministic stand-in for the asynchronous
                               pbStopFlag, honoured identically by the library and by the CPU oracle (tests/test_gpu_ba.py)          */
  int32_t deterministic;    /* 2 (default): bit-reproducible wherever the build can be - every wavefront of a linearisation workgroup adds the
                               per-camera sums Hpp / b_p into its OWN accumulator copy in program order, and the copies, workgroup partials
                               and everything downstream are summed in a fixed order: two solves of the same input on the same build are
                               BIT-IDENTICAL, as the reference is within a run (it walks its edges in a fixed order,
                               sparse_optimizer.cpp:482-487).  Maps beyond 590 free cameras keep their accumulators in HBM under global
                               atomics and fall back to "agree to rounding" silently.
                               1: the same, but such a map is refused (LLD_ERR_UNSUPPORTED) instead of falling back.
                               0: all wavefronts of a workgroup share the accumulator copies (LDS fp64 atomics whose order varies from run
                               to run): two solves agree to rounding (1e-16 per sum, amplified by 20 LM iterations to 1e-9 .. 1e-6 on the
                               weakest landmarks, and an observation whose chi2 ends within that of a threshold may come out on either side).
                               Faster by 0.4 - 0.7 % on 256 LBA-B windows (`secondary.deterministic` of the bench line); the default
                               until round 4. */
} lld_ba_params;

/* ALWAYS start from lld_ba_params_default(): a zero-initialised struct is NOT the default (deterministic = 0 selects the shared-accumulator
 * mode, its_* = 0 is refused), and fields added by later versions get their defaults here. */
void lld_ba_params_default(lld_ba_params* p);

typedef struct {
  double  chi2_round1;      /* LM cost (robust) after optimize(its_round1)                      */
  double  chi2_final;       /* LM cost after optimize(its_round2) (kernels removed)             */
  int32_t lm_iterations[2]; /* outer iterations executed per round                              */
  int32_t lm_trials[2];     /* linear solves (trials) executed per round                        */
  int32_t pcg_iterations;   /* total PCG iterations (0 for the oracle's direct solve)           */
  int32_t n_pt_obs_outlier; /* size of vToErase                                                 */
  int32_t n_ln_edge_outlier;
  int32_t n_lines_removed;
  int32_t aborted;          /* 1 iff the stop flag was up at the protocol's LAST poll: the check before optimising (Optimizer.cc:1220,
                               nothing is touched then), the check after optimize(its_round1) (:1230, round 2 is skipped, the final
                               classification still runs on the round-1 state), or - when round 2 ran - the last terminate() of
                               optimize(its_round2) (sparse_optimizer.cpp:376, levenberg.cpp:149).  The reference returns void; the
                               adapter needs only "aborted && lm_iterations[0]==0 -> leave the map alone"                          */
  int32_t reserved;
} lld_ba_stats;

typedef struct {
  double*  cam_qt;          /* [n_cams][7]    optimised poses (fixed ones copied through)        */
  double*  pt_xyz;          /* [n_points][3]                                                     */
  double*  line_x0;         /* [n_lines][3]   LineOptimizer::GetLineData; removed lines keep input */
  double*  line_dir;        /* [n_lines][3]                                                      */
  uint8_t* pt_obs_outlier;  /* [n_pt_obs]     1 -> (KF,MapPoint) goes to vToErase (Optimizer.cc:1281-1307) */
  uint8_t* ln_edge_outlier; /* [n_ln_obs][2]  1 -> kf id pushed by GetLineData for left/right edge */
  uint8_t* line_removed;    /* [n_lines]      1 -> vertex deleted by DisableOutliers            */
  lld_ba_stats stats;
} lld_ba_result;

/* One window, synchronous.  `abort_flag` may be NULL; it is the reference's pbStopFlag
 * (Optimizer.cc:1030-1031, sparse_optimizer.h:188), polled between LM trials. */
int lld_local_ba(lld_ctx* ctx, const lld_ba_window* in, const lld_ba_params* params,
                 volatile const int* abort_flag, lld_ba_result* out);

/* The same call with the stop flag as a BYTE: the reference's pbStopFlag is a `bool*` (LocalMapping::mbAbortBA, Optimizer.h:49); an
 * adapter passes it as `(volatile const unsigned char*)pbStopFlag` - character types may alias any object, an `int*` may not. */
int lld_local_ba_stopflag(lld_ctx* ctx, const lld_ba_window* in, const lld_ba_params* params,
                          volatile const unsigned char* stop_flag, lld_ba_result* out);

/* Batched, HBM-resident form: windows are uploaded once, then solved any number of times
 * (each solve restarts from the uploaded initial state).  This is the throughput path:
 * independent windows are what shards across GPUs (one batch per rank). */
typedef struct lld_ba_batch lld_ba_batch;
int  lld_ba_batch_create(lld_ctx* ctx, int n_windows, const lld_ba_window* windows,
                         const lld_ba_params* params, lld_ba_batch** out);
/* Error contract of a solve: when lld_ba_batch_solve returns anything but LLD_OK (a HIP call failed, a launch the build cannot express),
 * every stream the solve used has been drained before the call returns, and the batch is FAILED: its device state is somewhere inside an
 * LM trial, so solve / download / download_range / stats / result_records / phase_ms return LLD_ERR_INVALID from then on.  Destroy it and
 * create it again; the context stays usable. */
int  lld_ba_batch_solve(lld_ba_batch* batch, volatile const int* abort_flag); /* async on ctx stream until the final sync */
int  lld_ba_batch_download(lld_ba_batch* batch, int window, lld_ba_result* out);
/* Windows [first, first + count) into out[0..count): the same as `count` calls of lld_ba_batch_download, unpacked by several host
 * threads (a caller that wants every result of a 256-window batch moves 100 MB out of the landing buffer). */
int  lld_ba_batch_download_range(lld_ba_batch* batch, int first, int count, lld_ba_result* out /* [count] */);
int  lld_ba_batch_stats(lld_ba_batch* batch, lld_ba_stats* stats /* [n_windows] */);
/* Device buffer holding the fixed-stride result records of all windows (for the RCCL
 * gather): returns base pointer and record stride in bytes. */
int  lld_ba_batch_result_records(lld_ba_batch* batch, void** dev_ptr, uint64_t* stride_bytes);
/* Per-phase device time of the last solve in ms (HIP events on the stream the kernels are launched on):
 * [0] linearise (residuals + Jacobians + Hll/Hpl/Hpp), [1] Schur complement, [2] PCG on the reduced system,
 * [3] back-substitution + update + chi2, [4] LM control / outlier classification, [5] whole solve.
 * Mirrors G2OBatchStatistics (core/batch_stats.h:41-70), and like it ([0..4]) is OFF unless asked for: lld_ba_batch_set_phase_timing(batch, 1)
 * makes the following solves record an event at every phase boundary of every super-step.  An event between two dependent kernels costs
 * ~4 us of device time: 15 % of one window's solve, 10 % of a 32-window batch's, 1.6 % at 256 windows.  [5] is always measured. */
#define LLD_BA_N_PHASES 6
int  lld_ba_batch_set_phase_timing(lld_ba_batch* batch, int on);
int  lld_ba_batch_phase_ms(lld_ba_batch* batch, double* ms6);
/* Launch count (always) and summed HIP-event time (phase timing on) of one kernel family in the last solve; `kernel` uses the phase ids 0..4. */
int  lld_ba_batch_kernel_stats(lld_ba_batch* batch, int kernel, int64_t* launches, double* total_ms);
/* Tuning: number of window groups solved concurrently on separate HIP streams (1..8; 0 restores the default: one group below 8 windows,
 * three from 8, four from 16 - the device runs four streams side by side and time-slices a fifth -, and two for a batch of >= 64 windows
 * that was CREATED WHILE ANOTHER BATCH'S SOLVE RAN on the device: such a batch belongs to a pipelined caller whose other contexts' uploads
 * and downloads need streams of their own during its solve).  One group makes the HIP-event times of lld_ba_batch_phase_ms disjoint,
 * which is what a roofline measurement wants; several groups hide the latency-bound reduced solve and the per-super-step host poll.
 * Results do not depend on the grouping (bit-identical in the default deterministic mode). */
int  lld_ba_batch_set_groups(lld_ba_batch* batch, int n_groups);
void lld_ba_batch_destroy(lld_ba_batch* batch);

/* ------------------------------------------------------------------ the batch over several GPUs of one node
 * SURVEY.md 7 step 7 / 8e, north_star: independent windows shard across the GPUs of one node, the only exchange is the final gather of the
 * fixed-stride result records.  For a C++ host (LocalMapping / a relocalisation service keeps its threads): ONE process, one host thread
 * and one context per shard, created and driven by the library.  devices[] lists the HIP device of every shard; a device may appear
 * more than once (two shards share it).  Shard d owns the windows lld_ba_multi_shard(n_windows, n_devices, d) - the block partition of
 * lld_slam_amd/dist.py's shard(strong=True).  lld_ba_multi_solve runs every shard's lld_ba_batch_solve concurrently and, as each shard
 * finishes, copies its records into one buffer on devices[0] with hipMemcpyPeerAsync (a peer-to-peer copy over xGMI; a DEVIATION from north_star's
 * "RCCL for the final gather", chosen so that a torch process does not host a second RCCL instance - the torchrun path of bench.py uses RCCL itself): record k of the whole batch at k * stride.
 * lld_ba_multi_verify_gathered is the receiver's check that every record IS the window the partition put there (win_index and edge count
 * in the header) with a finished protocol.  Results per window are those of lld_ba_batch_* on that shard's batch, bit for bit. */
int  lld_device_count(void);                                          /* visible HIP devices; 0 without a GPU */
void lld_ba_multi_shard(int32_t n_windows, int32_t n_parts, int32_t part, int32_t* first, int32_t* count);   /* host only */
typedef struct lld_ba_multi lld_ba_multi;
int  lld_ba_multi_create(int32_t n_devices, const int32_t* devices, int32_t n_windows, const lld_ba_window* windows,
                         const lld_ba_params* params, lld_ba_multi** out);   /* n_windows >= n_devices */
int  lld_ba_multi_solve(lld_ba_multi* m, volatile const int* abort_flag);
int  lld_ba_multi_result_records(lld_ba_multi* m, void** dev_ptr, uint64_t* stride_bytes, int32_t* device);   /* the gathered buffer, on `device` = devices[0] */
int  lld_ba_multi_verify_gathered(lld_ba_multi* m, int32_t* n_checked);
int  lld_ba_multi_download(lld_ba_multi* m, int32_t window, lld_ba_result* out);   /* window of the whole batch, from the shard that solved it */
int  lld_ba_multi_times_ms(lld_ba_multi* m, double* slowest_solve_ms, double* slowest_gather_ms);   /* host clocks of the last lld_ba_multi_solve */
void lld_ba_multi_destroy(lld_ba_multi* m);

/* Diagnostic, host only (no device needed): the symbolic factorisation `reduced_solver = 0` runs per window - the stand-in for
 * LinearSolverEigen::computeSymbolicDecomposition (linear_solver_eigen.h:147-232).  block_nz[a * n_free_cams + b] != 0: free cameras a and
 * b share a landmark (symmetric; the diagonal is implied).  force: 0 = the plan a batch would use, 1 = the caller's camera order as one
 * chain of tile columns, 2 = the best two-chain (separator) plan only.  Writes the kernel's schedule (struct CholPlan of
 * lld_slam_amd/csrc/lld_ba_chol_plan.h, *plan_size bytes; its first byte is 1 when the structure-following kernel takes the window, 0
 * when it goes to the dense kernel) to plan_out if plan_bytes suffices.  tests/test_chol_plan.py executes such plans in numpy. */
int lld_ba_chol_plan(int32_t n_free_cams, const uint8_t* block_nz, int32_t force, void* plan_out, uint64_t plan_bytes, uint64_t* plan_size);

/* ================================================================== pose optimisation
 * Stands in for Optimizer::PoseOptimization (src/Optimizer.cc:653-932) including
 * AddLineMinOnlyPose (:562-650): 4 rounds x 10 LM iterations on one SE3 vertex. */
typedef struct {
  lld_camera cam;
  double pose_qt[7];                /* Converter::toSE3Quat(pFrame->mTcw)                       */
  int32_t n_points;                 /* matched keypoints with a MapPoint                        */
  const double*  pt_xw;             /* [n_points][3] world position widened from f32            */
  const double*  pt_uvr;            /* [n_points][3] u,v,uR (uR<0: mono)                        */
  const double*  pt_inv_sigma2;     /* [n_points]                                               */
  int32_t n_lines;
  const double*  ln_x0;             /* [n_lines][3]                                             */
  const double*  ln_dir;            /* [n_lines][3]                                             */
  const double*  ln_left;           /* [n_lines][4]                                             */
  const double*  ln_right;          /* [n_lines][4] xs<0 -> no stereo match                     */
  const int32_t* ln_octave;         /* [n_lines][2]                                             */
  const int32_t* ln_frame_index;    /* [n_lines] index i of the line in pFrame->mvLinesLeft (what AddLineMinOnlyPose pushes to
                                       vnIndexLines, Optimizer.cc:640); NULL = 0..n_lines-1 (every frame line has a MapLine).
                                       The reference classifies the edges of line i against the stereo or the mono threshold by
                                       vnStereoLines[i] (:898) although vnStereoLines is filled per EDGE (:643-648): the entry read
                                       is the stereo flag of the i-th edge added, whichever line that edge belongs to.  Reproduced
                                       as is; an index beyond the edge count (undefined behaviour there) counts as stereo.      */
} lld_pose_problem;

typedef struct {
  double  gamma;                    /* yaml `gamma` (0.5 for KITTI04-12_LBD.yaml:71)            */
  int32_t n_rounds;                 /* 4                                                         */
  int32_t its_per_round;            /* 10                                                        */
  int32_t max_trials;               /* 10                                                        */
  int32_t reserved;
} lld_pose_params;

void lld_pose_params_default(lld_pose_params* p);

typedef struct {
  double   pose_qt[7];
  int32_t  n_inliers;               /* return value of PoseOptimization (:931); 0 if <3 points  */
  int32_t  lm_iterations;           /* summed over rounds                                        */
  int32_t  lm_trials;
  int32_t  reserved;
  double   chi2;                    /* LM cost at the end of the last round                      */
  uint8_t* pt_outlier;              /* [n_points] pFrame->mvbOutlier                             */
  uint8_t* ln_outlier;              /* [n_lines]  pFrame->mvbOutlierLines                        */
} lld_pose_result;

int lld_pose_opt(lld_ctx* ctx, const lld_pose_problem* in, const lld_pose_params* params,
                 lld_pose_result* out);

/* Many frames in ONE launch (a relocalisation's candidates, a benchmark): one workgroup per frame.  A batch with more frames than the
 * device has compute units whose frames are small enough for two of them to share a CU's LDS (up to about 1100 points + 250 stereo
 * lines when the image observations are widened floats, as the reference's are) runs 256 lanes per frame and two frames per CU;
 * smaller batches and lld_pose_opt run 512 lanes per frame.  The two forms add a frame's edges in different (each fixed) orders: a
 * frame's result agrees between them to rounding (poses to 1e-9, identical inlier / outlier sets in every test and fuzz campaign),
 * and is bit-reproducible within a form - repeat solves, equal frames at other positions of a batch. */
typedef struct lld_pose_batch lld_pose_batch;
int  lld_pose_batch_create(lld_ctx* ctx, int n_frames, const lld_pose_problem* frames,
                           const lld_pose_params* params, lld_pose_batch** out);
int  lld_pose_batch_solve(lld_pose_batch* batch);
int  lld_pose_batch_download(lld_pose_batch* batch, int frame, lld_pose_result* out);
void lld_pose_batch_destroy(lld_pose_batch* batch);

/* ================================================================== Optimizer::OptimizeSim3 (src/Optimizer.cc:1656-1851)
 * One Sim3 vertex (S12, 7 dof, `_fix_scale` zeroes the scale update), the matched MapPoints of the two keyframes as FIXED points
 * in their own camera frames, two edges per correspondence (EdgeSim3ProjectXYZ: x1 = K1 proj(S12 X2); EdgeInverseSim3ProjectXYZ:
 * x2 = K2 proj(S12^-1 X1)) with Huber delta sqrt(th2), LM on the dense 7x7 system.  g2o differentiates these edges NUMERICALLY
 * (central differences, delta 1e-9, core/base_binary_edge.hpp:131-197): so do the oracle and the device.  Protocol: optimize(5);
 * a correspondence whose e12 or e21 chi2 exceeds th2 is dropped (both edges; vpMatches1[idx] = NULL); nMoreIterations = 10 if any
 * was dropped else 5; fewer than 10 correspondences left -> return 0 WITHOUT updating S12; optimize(nMoreIterations); count the
 * correspondences still within th2 (the others are NULLed too); S12 <- estimate.  `n`, the arrays and their order are the loop
 * :1704-1786 restricted to the correspondences that pass its tests (pMP1 && pMP2, neither bad, i2 >= 0). */
typedef struct {
  double fx1, fy1, cx1, cy1;        /* pKF1->mK (floats widened)                                   */
  double fx2, fy2, cx2, cy2;        /* pKF2->mK                                                    */
  double s12_q[4];                  /* g2oS12.rotation().coeffs(): x, y, z, w                      */
  double s12_t[3];
  double s12_s;
  int32_t n;
  int32_t reserved;
  const double* p1c;                /* [n][3] P3D1c = R1w*P3D1w + t1w (Converter::toVector3d)      */
  const double* p2c;                /* [n][3] P3D2c                                                */
  const double* obs1;               /* [n][2] pKF1->mvKeysUn[i].pt                                 */
  const double* obs2;               /* [n][2] pKF2->mvKeysUn[i2].pt                                */
  const double* inv_sigma2_1;       /* [n] pKF1->mvInvLevelSigma2[kpUn1.octave]                    */
  const double* inv_sigma2_2;       /* [n]                                                         */
} lld_sim3_problem;
typedef struct {
  double  th2;                      /* float th2 of the caller, widened (LoopClosing passes 10)    */
  int32_t fix_scale;                /* bFixScale (true for stereo / RGB-D)                         */
  int32_t its_first;                /* 5                                                           */
  int32_t its_more_bad;             /* 10 (when the first round dropped something)                 */
  int32_t its_more_clean;           /* 5                                                           */
  int32_t min_inliers;              /* 10                                                          */
  int32_t max_trials;               /* 10                                                          */
} lld_sim3_params;
void lld_sim3_params_default(lld_sim3_params* p);
typedef struct {
  double   s12_q[4], s12_t[3], s12_s;  /* g2oS12 on return (unchanged when the function returns 0 early) */
  uint8_t* dropped;                 /* [n] 1 -> vpMatches1[idx] = NULL                             */
  int32_t  n_inliers;               /* the return value (nIn, or 0)                                */
  int32_t  n_bad_first;             /* nBad of the first check                                     */
  int32_t  lm_iterations[2];
  int32_t  lm_trials[2];
  double   chi2;                    /* LM cost at the end of the last optimize()                   */
} lld_sim3_result;
int lld_optimize_sim3(lld_ctx* ctx, const lld_sim3_problem* in, const lld_sim3_params* params, lld_sim3_result* out);
/* several loop / relocalisation candidates in one launch (one workgroup each) */
int lld_optimize_sim3_batch(lld_ctx* ctx, int n, const lld_sim3_problem* problems, const lld_sim3_params* params, lld_sim3_result* outs);

/* ================================================================== Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1391-1654)
 * The pose graph itself: one Sim3 vertex per keyframe (Siw; `fixed[k]` for pLoopKF), one EdgeSim3 per loop / spanning-tree / old
 * loop / covisibility (>= 100) connection in the reference's insertion order, error = log(Sji * Siw * Sjw^-1)
 * (types_seven_dof_expmap.h:99-127), identity information, no robust kernel, NUMERIC Jacobians for both vertices like g2o
 * (core/base_binary_edge.hpp:131-197), Levenberg-Marquardt with setUserLambdaInit(1e-16), optimize(15).  Nothing is marginalised:
 * H is the 7N x 7N system, solved by the block-Jacobi PCG spread over the GPU (g2o: sparse Cholesky).
 * Building the edge list from the map (:1447-1585) stays with the adapter; the write-back (:1601-1653: SE3 recovery [R t/s],
 * MapPoint correction through the reference keyframe) is lld_essential_graph_apply.  LLD_ERR_INVALID for an edge whose end is out of range or whose two ends are the
 * same vertex (edge_i == edge_j: the reference never builds one). */
typedef struct {
  int32_t n_vertices;
  int32_t n_edges;
  const double*  sim3;          /* [n_vertices][8] Siw: rotation x, y, z, w, translation, scale      */
  const uint8_t* fixed;         /* [n_vertices] 1 = setFixed(true)                                    */
  const int32_t* edge_i;        /* [n_edges] vertex 0 of the edge (nIDi)                              */
  const int32_t* edge_j;        /* [n_edges] vertex 1 of the edge (nIDj)                              */
  const double*  edge_sji;      /* [n_edges][8] measurement Sji                                       */
} lld_pose_graph;
typedef struct {
  int32_t iterations;           /* 15                                                                 */
  int32_t fix_scale;            /* bFixScale                                                          */
  double  lambda_init;          /* 1e-16 (solver->setUserLambdaInit)                                  */
  int32_t max_trials;           /* 10                                                                 */
  int32_t pcg_max_iter;         /* 0 -> 10 * 7 * n_vertices                                           */
  double  pcg_rel_tol;          /* |r|_M / |b|_M of the PCG                                           */
  int32_t solver;               /* 0 auto (dense Cholesky up to 7*unknowns <= 32768, else PCG), 1 dense Cholesky, 2 PCG */
  int32_t reserved;
} lld_pose_graph_params;
void lld_pose_graph_params_default(lld_pose_graph_params* p);
typedef struct {
  double* sim3;                 /* [n_vertices][8] CorrectedSiw                                       */
  double  chi2;                 /* active chi2 after the last accepted step                           */
  int32_t lm_iterations, lm_trials, pcg_iterations, solver_used;   /* solver_used: 1 dense Cholesky, 2 PCG, 0 nothing to solve */
} lld_pose_graph_result;
int lld_optimize_essential_graph(lld_ctx* ctx, const lld_pose_graph* graph, const lld_pose_graph_params* params, lld_pose_graph_result* out);

/* ================================================================== descriptor matching
 * lld_match_hamming256*: ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1647-1663) plus
 * the best / second-best loops of the Search* family (e.g. :76-125, :201-249).  Strict '<'
 * everywhere, so the FIRST candidate in iteration order wins ties.
 *   - brute force: candidates are all train rows in index order (mask NULL);
 *   - mask: byte matrix [nq][nt], non-zero = candidate (index order);
 *   - csr : explicit candidate lists in the reference's own list order
 *           (Frame::GetFeaturesInArea / BoW node lists); outputs are train indices.
 * Unmatched queries (no candidate) return idx -1 and dist 256 (the reference initialises
 * bestDist=256, ORBmatcher.cc:72).
 */
int lld_match_hamming256(lld_ctx* ctx, const uint32_t* q, int nq, const uint32_t* t, int nt,
                         const uint8_t* mask_or_null,
                         int32_t* best_idx, int32_t* best_dist,
                         int32_t* second_idx, int32_t* second_dist);
int lld_match_hamming256_csr(lld_ctx* ctx, const uint32_t* q, int nq, const uint32_t* t, int nt,
                             const int32_t* cand_start /*[nq+1]*/, const int32_t* cand_idx,
                             int32_t* best_idx, int32_t* best_dist,
                             int32_t* second_idx, int32_t* second_dist);
/* `batch` independent frame pairs of identical shape, inputs/outputs are DEVICE pointers:
 * q [batch][nq][8], t [batch][nt][8], outputs [batch][nq]. */
int lld_match_hamming256_batch_dev(lld_ctx* ctx, int batch, const uint32_t* q_dev, int nq,
                                   const uint32_t* t_dev, int nt,
                                   int32_t* best_idx_dev, int32_t* best_dist_dev,
                                   int32_t* second_idx_dev, int32_t* second_dist_dev);

/* lld_match_l2f32*: LineMatcher::MatchLineDescriptors call sites
 * (src/TwoFrameLineMatcher.cc:112, src/Tracking.cc:1092,1532).  The function itself lives in
 * the un-vendored LBDMOD library (parity unpinned); this build defines it as
 * d = sqrt( sum_i (double)(a_i - b_i)^2 ), the float difference squared and accumulated in
 * double in ascending i — the arithmetic of cv::norm(a - b) used at src/MapLine.cc:175. */
int lld_match_l2f32(lld_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim,
                    const uint8_t* mask_or_null,
                    int32_t* best_idx, double* best_dist,
                    int32_t* second_idx, double* second_dist);
int lld_match_l2f32_batch_dev(lld_ctx* ctx, int batch, const float* q_dev, int nq,
                              const float* t_dev, int nt, int dim,
                              int32_t* best_idx_dev, double* best_dist_dev,
                              int32_t* second_idx_dev, double* second_dist_dev);

/* TwoFrameLineMatcher::MatchLines (src/TwoFrameLineMatcher.cc:26-77): sequential greedy
 * assignment.  For left line j = 0..nq-1 in order: over right lines oi not yet taken and
 * with gate[j][oi] != 0 (CheckLinePair's geometric gates, :81-109, computed by the caller),
 * pick the strict running minimum of the descriptor distance below `tau`; the winner is
 * masked for all later j.  matches[j] = oi or -1.
 *
 * Limits of the line matchers (lld_line_match_greedy, lld_line_match_stereo, lld_line_track_match; rows = nq or
 * n_map, columns = nt or n_cur).  Each is decided on the host from the arguments alone and refused BEFORE anything is
 * allocated, copied or queued; the context stays usable and the next valid call is unaffected:
 *   LLD_ERR_INVALID      a required pointer is NULL, a count is negative, dim <= 0, sx / sy not > 0, an octave outside
 *                        0..64, a stereo partner index >= the count of right lines;
 *   LLD_ERR_UNSUPPORTED  dim > LLD_LINE_DIM_MAX (128) - lld_line_match_last_frame alone takes up to
 *                        LLD_LINE_LASTKF_DIM_MAX (4096);
 *   LLD_ERR_UNSUPPORTED  columns * 8 + dim * 4 > LLD_LINE_LDS_CEILING (150 KiB): one row of distances and the row's
 *                        descriptor live in LDS (19 164 columns at dim 72);
 *   LLD_ERR_UNSUPPORTED  (rows + columns) * 4 + 16 > LLD_LINE_LDS_CEILING: the greedy resolve keeps one word per row
 *                        and per column in LDS (38 396 rows and columns together).
 * lld_line_match_last_frame has no size ceiling of this kind (its LDS holds one descriptor: dim * 4 + 16 bytes). */
#define LLD_LINE_DIM_MAX 128
#define LLD_LINE_LASTKF_DIM_MAX 4096
#define LLD_LINE_LDS_CEILING (150 * 1024)
int lld_line_match_greedy(lld_ctx* ctx, const float* desc_left, int nq, const float* desc_right,
                          int nt, int dim, const uint8_t* gate /*[nq][nt]*/, double tau,
                          int32_t* matches /*[nq]*/, double* match_dist /*[nq] or NULL*/);

/* TwoFrameLineMatcher::MatchLines with CheckLinePair's geometric gates computed ON THE DEVICE
 * (src/TwoFrameLineMatcher.cc:26-124; the only caller is the left/right line association of the
 * Frame constructor, src/Frame.cc:121-122, so T = identity and T_right = GetTForRight(T, b),
 * src/LineMatching.cc:228-237).  For every (left j, right oi) pair the gate is
 *   same octave (:81-84)  &&  both lengths >= min_line_length (:86-91)
 *   && vgl::TriangulateLine succeeds (src/vgl.cc:78-108: back-projected plane normals
 *      n = R*GetNormalizedLineEq(kl,K) not closer than |cos| 0.975, direction n1 x n2, X0 from
 *      the 3x3 system [n1; n2; dir] X0 = [n1.t1; n2.t2; 0])  &&  |X0| >= 0.5 (:100-103)
 *   && both detected endpoints of the LEFT line, re-projected onto the 3D line by the 3x2 least
 *      squares of vgl::ReprojectLinePointTo3D (src/vgl.cc:336-346, src/LineMatching.cc:277-292),
 *      have z >= 0 (:104-109);
 * then the greedy, order-dependent descriptor assignment of lld_line_match_greedy.
 * lines: [n][4] float startPointX, startPointY, endPointX, endPointY of the KeyLines.
 * K: row-major 3x3 (Frame.cc:118-120).  b: mbf / fx.  gate_out: [nq][nt] bytes or NULL.
 * Refusals and size ceilings: see lld_line_match_greedy (LLD_ERR_INVALID / LLD_ERR_UNSUPPORTED, nothing is queued). */
typedef struct {
  double K[9];
  double b;
  double tau;               /* thrDD / mdThr */
  int32_t min_line_length;  /* minLineLen */
  int32_t is_stereo;        /* 1: octaves must be equal (:81) */
} lld_line_stereo_params;
int lld_line_match_stereo(lld_ctx* ctx, const lld_line_stereo_params* params,
                          const float* left_lines, const int32_t* left_octave, const float* desc_left, int nq,
                          const float* right_lines, const int32_t* right_octave, const float* desc_right, int nt,
                          int dim, int32_t* matches /*[nq]*/, double* match_dist /*[nq] or NULL*/,
                          uint8_t* gate_out /*[nq][nt] or NULL*/);

/* Tracking::AddLinesFrom (src/Tracking.cc:996-1124): the per-frame association of map lines (lines of the last frame /
 * of the local map) with the lines of the current frame, candidate selection and geometric gates ON THE DEVICE.
 * For map line i = 0..n_map-1 in order (skip[i] != 0: NULL, already tracked in this frame or bad, :1023-1034):
 *   candidates = SubselectWithGrid (src/LineMatching.cc:154-180): the projected line's Hough cell neighbourhood
 *     (GetHoughCoordinates, :63-152, 3 cells to each side in distance and angle) looked up in the frame's 50 x 50
 *     line grid, in ascending line index (the reference collects them in a std::set);
 *   a candidate si is dropped if it already holds a map line (:1054), has no stereo partner (:1059-1063, unless
 *     monocular), if one of the map line's main points X1, X2 lies behind the camera (:1066-1074), or if the L1
 *     reprojection error of its left / right detected endpoints against the projected 3D line
 *     (GetReprojErrPixelsL1 = vgl::LineReprojErrorL1, src/vgl.cc:548-559) exceeds thr_reproj_base * 1.44^octave
 *     (GetReprojThrPyramid, src/LineMatching.cc:239-247) in EITHER image (:1085);
 *   the strict running minimum of MatchLineDescriptors (float L2, see lld_match_l2f32) wins if it is <= md_thr
 *     (:1099) and then occupies its line for all later i (:1117).
 * The reference allocates the line grid (Frame.cc:746-755) but never fills it (SURVEY hazard 10), so its loop never
 * sees a candidate; this build DEFINES the fill it lacks: a frame line sits in the cell (dist_ind, ang_ind) that
 * GetHoughCoordinates computes for the image line through its left KeyLine's endpoints (GetLineEq, :255-268).
 * use_grid = 0 makes every line of the frame a candidate (brute force under the same gates).
 * T_curr: camera-to-world 4x4, row-major (the callers pass mTcw.inv()); the right camera is GetTForRight(T_curr, b).
 * map_x0 / map_dir: MapLine::GetMinimalPos; map_x1 / map_x2: GetMainPoints3D.  lines: [n][4] float startPointX,
 * startPointY, endPointX, endPointY.  line_matches[si]: index of the right line matched to left line si or -1.
 * matches[i] = frame line or -1; gate_out [n_map][n_cur] (optional): 1 where a pair passed every test but the
 * descriptor threshold.
 * Refusals and size ceilings (rows = n_map, columns = n_cur): see lld_line_match_greedy; LLD_ERR_INVALID or
 * LLD_ERR_UNSUPPORTED is returned before anything is allocated or queued. */
typedef struct {
  double K[9];
  double T_curr[16];
  double b;
  double thr_reproj_base;   /* thrReprojLineBase */
  double md_thr;            /* mdThr (KITTI04-12_LBD.yaml:70) */
  double sx, sy;            /* 1 / mnMaxX, 1 / mnMaxY */
  int32_t monocular;
  int32_t use_grid;
} lld_line_track_params;
int lld_line_track_match(lld_ctx* ctx, const lld_line_track_params* params,
                         int n_map, const double* map_x0, const double* map_dir, const double* map_x1, const double* map_x2,
                         const uint8_t* map_skip /*[n_map] or NULL*/, const float* map_desc,
                         int n_cur, const float* left_lines, const int32_t* left_octave,
                         int n_right, const float* right_lines, const int32_t* line_matches /*[n_cur]*/,
                         const uint8_t* occupied /*[n_cur] or NULL*/, const float* cur_desc, int dim,
                         int32_t* matches /*[n_map]*/, double* match_dist /*[n_map] or NULL*/,
                         uint8_t* gate_out /*[n_map][n_cur] or NULL*/);
/* Tracking::MatchLinesLastKF (src/Tracking.cc:1449-1611): new map lines from the lines the current and the last
 * stereo frame share.  For every line i of the current frame that holds no map line and has a stereo partner
 * (:1477-1487): vgl::TriangulateLine of its left / right KeyLine (src/vgl.cc:78-108) in the current pose; the Hough
 * cell neighbourhood of that 3D line projected into the LAST frame (SubselectWithGrid, :1504) gives the candidates
 * li; li is dropped without stereo partner (:1511-1515), if last_skip[li] (its map line was tracked in this frame,
 * :1517-1520) or if the L1 reprojection error exceeds 6 px * 1.44^octave in BOTH images of the last frame (:1526 -
 * `&&`, where AddLinesFrom has `||`); strict running minimum of MatchLineDescriptors, accepted if <= md_thr
 * (:1558); then vgl::MultiTriangulateLine over the four views (src/vgl.cc:28-76: unit plane normals, |cos| <= 0.975
 * against the first one, direction = right singular vector of the smallest singular value of the normal matrix,
 * X0 = least-squares point of the four planes minus its component along the direction), ReprojectKeyLineTo3D of
 * the current left KeyLine (src/LineMatching.cc:277-292) and the depth test of both end points in all four views
 * (:1580-1592).  No step depends on another line: rows run in parallel.
 * match_last[i]: the accepted line of the last frame or -1; created[i]: 1 if the reference would construct the
 * MapLine (x0 / dir [n_cur][3] valid).  The sign of dir is the build's (largest component positive): Eigen's JacobiSVD
 * is not restated and a 3D line has no orientation.  T_curr, T_last: camera-to-world, row-major 4x4.
 * Refused before anything is queued: LLD_ERR_INVALID for a NULL required pointer, a negative count, dim <= 0, sx / sy
 * not > 0, an octave of the last frame outside 0..64 or a partner index >= its right count; LLD_ERR_UNSUPPORTED for
 * dim > LLD_LINE_LASTKF_DIM_MAX (4096). */
typedef struct {
  double K[9];
  double T_curr[16], T_last[16];
  double b;
  double thr_reproj_base;   /* 6 px (Tracking.cc:1451) */
  double md_thr;
  double sx, sy;
  int32_t use_grid;
  int32_t pad;
} lld_line_lastkf_params;
int lld_line_match_last_frame(lld_ctx* ctx, const lld_line_lastkf_params* params,
                              int n_cur, const float* cur_left, int n_cur_right, const float* cur_right,
                              const int32_t* cur_line_matches, const uint8_t* cur_occupied /*or NULL*/, const float* cur_desc,
                              int n_last, const float* last_left, const int32_t* last_left_octave, int n_last_right,
                              const float* last_right, const int32_t* last_line_matches, const uint8_t* last_skip /*or NULL*/,
                              const float* last_desc, int dim,
                              int32_t* match_last /*[n_cur]*/, uint8_t* created /*[n_cur]*/, double* x0 /*[n_cur][3]*/,
                              double* dir /*[n_cur][3]*/);
/* The grid cell of that fill: cell[si] = dist_ind * 50 + ang_ind (host helper, no device work). */
int lld_line_hough_cells(const float* lines, int n, double sx, double sy, int32_t* cell);

/* ================================================================== guided ORB search
 * lld_orb_search: the complete body of one ORBmatcher::Search* / Fuse / ComputeStereoMatches
 * routine for one (query set, keypoint set) pair: candidate generation ON THE DEVICE, the
 * per-candidate skip rules, DescriptorDistance, best / second-best, the accept rules, the
 * order-dependent "keypoint already taken" rule and the rotation-histogram filter
 * (SURVEY Appendix B).  The caller (the reference-side adapter) supplies what the reference
 * computes per query BEFORE its inner loop - projected position, window radius, predicted
 * level range, predicted right coordinate - and per keypoint the frame's own vectors.
 *
 * Candidate sets (lld_orb_search.candidates), always visited in the reference's order, which
 * decides ties (strict '<': the first candidate in order wins, unless tie_last):
 *   LLD_ORB_CAND_ALL   every keypoint, index order.
 *   LLD_ORB_CAND_GRID  Frame::GetFeaturesInArea (src/Frame.cc:391-444) / KeyFrame::
 *                      GetFeaturesInArea (src/KeyFrame.cc:592-631) over the 64x48 grid built
 *                      by Frame::AssignFeaturesToGrid + PosInGrid (:294-313, :446-456): cells
 *                      ix in [nMinCellX,nMaxCellX] outer, iy inner, keypoints of a cell in index
 *                      order; |dx|<r && |dy|<r; keypoints whose cell falls outside the grid are
 *                      never candidates.  All in float, as the reference.
 *   LLD_ORB_CAND_CSR   explicit lists: query q visits cand_idx[cand_range[q][0] .. cand_range[q][1]) in that order;
 *                      ranges may be shared between queries (all keypoints of one BoW node search the same
 *                      node list of the other frame: src/ORBmatcher.cc:185-187,561,700).
 *   LLD_ORB_CAND_ROWS  Frame::ComputeStereoMatches (src/Frame.cc:541-613): right keypoint iR is a
 *                      candidate of left keypoint iL iff (int)vL lies in [floor(yR-r), ceil(yR+r)],
 *                      r = 2*scale[octave_R]; index order; uR in [uL-disp_max, uL-disp_min];
 *                      a query with uL-disp_min < 0 is skipped (:577-578).  The reference indexes
 *                      vRowIndices[vL] unchecked; with image_rows > 0 a query whose row (long long)vL is
 *                      outside [0, image_rows) has no candidates (vL in (-1, 0) truncates to row 0).
 * Gates (lld_orb_search.gates, OR of LLD_ORB_GATE_*), each skips a candidate:
 *   LEVEL    octave < q_level_min || (q_level_max >= 0 && octave > q_level_max)
 *   STEREO   t_uright > 0 && fabs(q_uright - t_uright) > q_stereo_radius   (ORBmatcher.cc:90-95,1400-1406)
 *   CHI2     Fuse's reprojection gate (ORBmatcher.cc:912-936): stereo keypoints (t_uright>=0)
 *            e2*invSigma2[octave] > 7.8, others > 5.99, e = (q_uv - t_xy [, q_uright - t_uright])
 *   EPIPOLAR SearchForTriangulation (ORBmatcher.cc:720-751): only_stereo filter; epipole distance
 *            when neither side is stereo; CheckDistEpipolarLine (:138-157) with the query's line
 *   t_occupied[k] != 0 always skips; with `sequential` a keypoint taken by an accepted EARLIER
 *   query whose q_blocks flag is set is skipped too (the reference writes mvpMapPoints /
 *   vpMatched / vbMatched2 inside its loop).  The device reaches the sequential answer by
 *   fixed-point rounds over all queries and reports the number of rounds.
 *   sequential = 2 is the rule of ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405-520), the one routine whose order
 *   dependence is not an occupancy: a candidate is skipped when an EARLIER query holds it with a distance <= this one
 *   (`vMatchedDistance[i2]<=dist`, :443), an accepted query takes the keypoint away from its holder, whose match is cleared
 *   (:458-465), and the rotation histogram counts every acceptance, also those taken away later (:466-476).  match[] is
 *   vnMatches12 before the orientation filter, owner[] vnMatches21, `rounds` 1 + the number of queries whose cached candidate
 *   list ran dry; GRID or ALL candidates, ratio_mode 0 or 1, no tie_last.
 * Accept: best <= accept_max, then ratio_mode 0 none | 1 (float)best < nn*(float)second
 * (:226-228) | 2 reject iff level(best)==level(second) && best > nn*second (:118-121).
 * check_orientation: 30-bin histogram of q_angle - t_angle, factor 1/30, ComputeThreeMaxima
 * (:1601-1642); matches outside the three kept bins are flagged `removed`.
 * Outputs (host arrays): match[nq] accepted keypoint or -1 (before the orientation filter);
 * removed[nq]; best/second distances (256 = none); owner[nt] = the query that holds keypoint k at
 * the end of the routine (last accepted writer; -1 if none or if any writer was removed by the
 * orientation filter - the reference NULLs the slot, :1452-1460); n_matches = the routine's
 * return value. */
enum { LLD_ORB_CAND_ALL = 0, LLD_ORB_CAND_GRID = 1, LLD_ORB_CAND_CSR = 2, LLD_ORB_CAND_ROWS = 3 };
enum { LLD_ORB_GATE_LEVEL = 1, LLD_ORB_GATE_STEREO = 2, LLD_ORB_GATE_CHI2 = 4, LLD_ORB_GATE_EPIPOLAR = 8 };
#define LLD_ORB_MAX_KEYPOINTS 4096
#define LLD_ORB_MAX_LEVELS 16

typedef struct {
  /* keypoints searched (Frame / KeyFrame; the right image for ROWS) */
  int32_t nt;
  const uint32_t* t_desc;       /* [nt][8]                                                       */
  const float*    t_xy;         /* [nt][2] mvKeysUn[k].pt (ROWS: mvKeysRight[k].pt)              */
  const int32_t*  t_octave;     /* [nt]                                                          */
  const float*    t_uright;     /* [nt] mvuRight; NULL = all -1                                  */
  const float*    t_angle;      /* [nt] degrees; needed with check_orientation                   */
  const uint8_t*  t_occupied;   /* [nt] or NULL                                                  */
  /* queries, in the order the reference's outer loop visits them */
  int32_t nq;
  const uint32_t* q_desc;       /* [nq][8]                                                       */
  const uint8_t*  q_valid;      /* [nq] or NULL; 0 = the reference `continue`s before the search */
  const uint8_t*  q_blocks;     /* [nq] or NULL (= all 1); see `sequential`                      */
  const float*    q_uv;         /* [nq][2] GRID: window centre; ROWS: left keypoint; CHI2: projection */
  const float*    q_radius;     /* [nq]    GRID                                                  */
  const int32_t*  q_level_min;  /* [nq]    LEVEL                                                 */
  const int32_t*  q_level_max;  /* [nq]    LEVEL                                                 */
  const float*    q_uright;     /* [nq]    STEREO / CHI2                                         */
  const float*    q_stereo_radius; /* [nq] STEREO                                                */
  const float*    q_angle;      /* [nq]    check_orientation                                     */
  const float*    q_epiline;    /* [nq][3] EPIPOLAR: a,b,c of x1'F12 (ORBmatcher.cc:141-143)     */
  const uint8_t*  q_stereo;     /* [nq]    EPIPOLAR: bStereo1                                    */
  const int32_t*  cand_range;   /* [nq][2] CSR: begin, end into cand_idx                         */
  const int32_t*  cand_idx;     /* [n_cand] CSR                                                  */
  int32_t         n_cand;
  /* frame constants */
  float grid_min_x, grid_min_y, grid_width_inv, grid_height_inv;   /* mnMinX, mnMinY, mfGridElement*Inv */
  int32_t grid_cols, grid_rows;                                    /* 64, 48 (Frame.h:43-44)     */
  int32_t n_levels;
  const float* level_scale;       /* [n_levels] mvScaleFactors     (ROWS, EPIPOLAR)              */
  const float* level_sigma2;      /* [n_levels] mvLevelSigma2      (EPIPOLAR)                    */
  const float* level_inv_sigma2;  /* [n_levels] mvInvLevelSigma2   (CHI2)                        */
  float disp_min, disp_max;       /* ROWS: minD, maxD (Frame.cc:558-560)                         */
  float epipole_x, epipole_y;     /* EPIPOLAR (ORBmatcher.cc:669-671)                            */
  int32_t only_stereo;            /* EPIPOLAR: bOnlyStereo                                       */
  /* rules */
  int32_t candidates;             /* LLD_ORB_CAND_*                                              */
  int32_t gates;                  /* OR of LLD_ORB_GATE_*                                        */
  int32_t tie_last;               /* 1: `dist>bestDist -> skip`, later equal distance replaces (ORBmatcher.cc:733) */
  int32_t accept_max;             /* accept iff best <= accept_max                               */
  int32_t ratio_mode;
  float   nnratio;                /* mfNNratio                                                   */
  int32_t sequential;             /* 0 | 1 occupancy by earlier queries | 2 SearchForInitialization's take-over rule        */
  int32_t check_orientation;
  int32_t image_rows;             /* ROWS: rows of the image (vRowIndices.size(), Frame.cc:536); 0 = the query's row is not checked */
} lld_orb_search;

typedef struct {
  int32_t* match;        /* [nq] */
  int32_t* best_dist;    /* [nq] */
  int32_t* second_dist;  /* [nq] */
  uint8_t* removed;      /* [nq] */
  int32_t* owner;        /* [nt] or NULL */
  int32_t  n_matches;
  int32_t  rounds;       /* fixed-point rounds executed (1 without `sequential`) */
} lld_orb_search_result;

int lld_orb_search_run(lld_ctx* ctx, const lld_orb_search* s, lld_orb_search_result* out);
/* Tracking::SearchLocalPoints (src/Tracking.cc:1613-1664) in one call: Frame::isInFrustum (src/Frame.cc:333-389) for every
 * local MapPoint ON THE DEVICE - camera transform, projection, image bounds, scale-invariance distance band, viewing angle,
 * MapPoint::PredictScale (src/MapPoint.cc:402-417), mTrackProjXR - and then ORBmatcher::SearchByProjection(F, vpMapPoints, th)
 * (src/ORBmatcher.cc:45-129) on the projected points without a trip through the host.
 * The float / double mixture follows the reference's OpenCV calls as this build restates them (OpenCV is not in the image:
 * parity unpinned): `mRcw*P+mtcw` is one cv::gemm, i.e. float(sum_k double(R_ik) double(P_k) + double(t_i)); `P-mOw` a float
 * subtraction; cv::norm and Mat::dot accumulate in double; everything else is float arithmetic in source order; log() of a
 * float is the float overload - computed the way glibc (>= 2.27) computes logf, so that PredictScale's ceil() flips at the same
 * float as on the reference's host (lld_orb_search.hip glibc_logf; a libm with another logf moves one level in ~1e8).
 * `frame`: only the keypoint side (nt, t_*), the grid constants and n_levels / level_scale are read.
 * frustum outputs (any may be NULL): in_view[n] (mbTrackInView), proj_uvr[n][3] (mTrackProjX, mTrackProjY, mTrackProjXR),
 * level[n] (mnTrackScaleLevel), view_cos[n] (mTrackViewCos); values of points outside the frustum are unspecified. */
typedef struct {
  float Rcw[9], tcw[3], Ow[3];          /* Frame::mRcw, mtcw, mOw (UpdatePoseMatrices, src/Frame.cc:325-331) */
  float fx, fy, cx, cy, bf;             /* mbf = baseline * fx */
  float min_x, max_x, min_y, max_y;     /* mnMinX ... */
  float log_scale_factor;               /* mfLogScaleFactor */
  int32_t n_levels;                     /* mnScaleLevels */
} lld_frame_view;
typedef struct {
  int32_t n;
  const float*    world_pos;            /* [n][3] MapPoint::GetWorldPos */
  const float*    normal;               /* [n][3] GetNormal */
  const float*    max_distance;         /* [n] mfMaxDistance (GetMaxDistanceInvariance = 1.2f * it) */
  const float*    min_distance;         /* [n] mfMinDistance (0.8f * it) */
  const uint32_t* desc;                 /* [n][8] GetDescriptor */
  const uint8_t*  has_obs;              /* [n] Observations()>0, or NULL = all 1 */
  const uint8_t*  skip;                 /* [n] or NULL: mnLastFrameSeen == frame id || isBad (src/Tracking.cc:1640-1643) */
} lld_map_points;
typedef struct { uint8_t* in_view; float* proj_uvr; int32_t* level; float* view_cos; } lld_frustum_result;
int lld_orb_search_local_points(lld_ctx* ctx, const lld_orb_search* frame, const lld_frame_view* view, const lld_map_points* points,
                                float viewing_cos_limit, float th, float nnratio,
                                lld_frustum_result* frustum_or_null, lld_orb_search_result* out);
/* ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th, bMono) (src/ORBmatcher.cc:1328-1470, the matcher of
 * Tracking::TrackWithMotionModel) in one call: the projection of the last frame's MapPoints into the current frame (:1358-1377:
 * cv::gemm transform, invzc = float(1.0 / double(z)), image bounds), the window radius th*scale[octave], the octave range chosen by
 * `direction` (+1 bForward, -1 bBackward, 0 neither; the caller evaluates :1343-1350 once per frame pair), ur = u - mbf*invzc, then
 * the search with occupancy and the rotation histogram.  last_valid[i] = LastFrame.mvpMapPoints[i] && !LastFrame.mvbOutlier[i].
 * proj_uvr (may be NULL): [n][3] u, v, ur of the projected points. */
typedef struct {
  int32_t n;
  const float*    world_pos;    /* [n][3] pMP->GetWorldPos() of LastFrame.mvpMapPoints[i] */
  const uint8_t*  valid;        /* [n] */
  const int32_t*  octave;       /* [n] LastFrame.mvKeys[i].octave */
  const float*    angle;        /* [n] LastFrame.mvKeysUn[i].angle */
  const uint32_t* desc;         /* [n][8] pMP->GetDescriptor() */
  const uint8_t*  has_obs;      /* [n] Observations()>0, or NULL = all 1 */
} lld_last_frame_points;
int lld_orb_search_last_frame(lld_ctx* ctx, const lld_orb_search* frame, const lld_frame_view* view, const lld_last_frame_points* last,
                              int direction, float th, int check_orientation, float* proj_uvr_or_null, lld_orb_search_result* out);
/* A frame RESIDENT on the device for the time the Tracking thread works on it (round 5).  The reference runs, on one Frame, the matcher of
 * TrackWithMotionModel (src/Tracking.cc:904), PoseOptimization (:937), SearchLocalPoints (:1133), PoseOptimization (:1152); the two
 * matchers above re-send the frame's 2000 keypoints (descriptors, positions, octaves, right coordinates, angles: 106 KB through pinned
 * memory) on every call.  lld_frame_create uploads the keypoint side of `keypoints` (nt, t_desc, t_xy, t_octave, t_uright, t_angle, the grid
 * constants and level tables; the query side is ignored) ONCE; lld_frame_search_last_frame / lld_frame_search_local_points are
 * lld_orb_search_last_frame / lld_orb_search_local_points on that frame - same arguments, same results bit for bit - and move only their
 * queries and the per-call occupancy bytes (t_occupied[nt] or NULL: Frame::mvpMapPoints[k] != NULL at the time of the call).  The handle
 * belongs to the context (and host thread) it was created on; destroy it before the context. */
typedef struct lld_frame lld_frame;
int  lld_frame_create(lld_ctx* ctx, const lld_orb_search* keypoints, lld_frame** out);
int  lld_frame_search_last_frame(lld_frame* frame, const uint8_t* t_occupied, const lld_frame_view* view, const lld_last_frame_points* last,
                                 int direction, float th, int check_orientation, float* proj_uvr_or_null, lld_orb_search_result* out);
int  lld_frame_search_local_points(lld_frame* frame, const uint8_t* t_occupied, const lld_frame_view* view, const lld_map_points* points,
                                   float viewing_cos_limit, float th, float nnratio, lld_frustum_result* frustum_or_null, lld_orb_search_result* out);
void lld_frame_destroy(lld_frame* frame);
/* ------------------------------------------------------------------ the Tracking thread's per-frame chain, device resident (round 6)
 * On one stereo Frame the reference runs
 *   TrackWithMotionModel (src/Tracking.cc:885-994): SearchByProjection(Current, Last, th) - again with 2*th when it finds fewer than 20
 *     (:904-911) -> AddLinesFrom(mLastFrame.mvpMapLines) (:924) -> Optimizer::PoseOptimization (:937) -> outlier discard (:940-975);
 *   TrackLocalMap (:1126-1220): SearchLocalPoints (:1133, :1613-1664) -> AddLinesFrom(local_lines) (:1140) -> PoseOptimization (:1152)
 *     -> statistics / discard (:1155-1187),
 * and between those calls the Frame carries mvpMapPoints, mvbOutlier, mvpMapLines, mvbOutlierLines and mTcw.  lld_frame_track_* keeps
 * exactly that state in HBM next to the resident keypoints: every stage reads what the stage before it left on the device, the edges of
 * PoseOptimization are gathered from the match tables by a kernel (what Optimizer.cc:683-804 does from mvpMapPoints / mvpMapLines), and
 * NOTHING travels to the host between the stages.  Both calls only upload their map-side inputs (one copy), queue their kernels on the
 * context's stream and return; lld_frame_track_download fetches both stages' records in one copy and is the only synchronisation.
 * (The reference's host needs the MapPoints of stage 1 for UpdateLocalMap before it can name the local map of stage 2.  A caller that keeps
 * its map on the host downloads between the two calls - 10 KB - and gathers the local map into arrays; a caller that keeps it in an lld_map
 * queues lld_frame_track_update_local_map and lld_frame_track_local_map_resident instead and downloads once, after stage 2: see "the resident
 * map" at the end of this header.)
 *
 * MapPoints / MapLines are named by caller-chosen ids >= 0 (MapPoint::mnId / MapLine ids, or indices into the caller's own tables):
 *   - "pMP->mnLastFrameSeen == mCurrentFrame.mnId" (:1640), which makes SearchLocalPoints skip the points the frame already holds (:1629)
 *     AND those the outlier discard of stage 1 marked (:949), is an id look-up against the frame's held + discarded ids;
 *   - "pML->tracked_last_id == mCurrentFrame.mnId" (:1023) likewise against the lines stage 1 assigned (kept even when PoseOptimization
 *     then threw the line out, as in the reference, which never resets tracked_last_id).
 * Stale state the reference keeps is kept: mvbOutlierLines is not cleared when an outlier line leaves the frame (:962-975), so a line
 * edge that never reaches a classification (fewer than 10 edges, Optimizer.cc:878) reads the old flag.
 * Deviations (both inside the "OpenCV restated" caveat of the searches above): the camera-to-world matrix AddLinesFrom receives is the
 * frame's own Rwc = Rcw^T, Ow (Frame::UpdatePoseMatrices) widened to double, where the reference inverts mTcw with cv::Mat::inv() (a float
 * LU, equal up to float rounding); stage 2's float view is formed on the device from the optimised SE3Quat exactly as
 * lld_se3_to_tcw_f32 + UpdatePoseMatrices form it on the host.
 * `params` of the two calls of one frame must agree.  The handle belongs to one context / host thread like every lld_frame call. */
typedef struct {
  int32_t n_left;  const float* left;  const int32_t* left_octave;    /* mvLinesLeft: [n][4] startPointX, startPointY, endPointX, endPointY; octave */
  int32_t n_right; const float* right; const int32_t* right_octave;   /* mvLinesRight                                                              */
  const int32_t* line_matches;                                         /* [n_left] Frame::line_matches: right line of left line i, or -1            */
  const float* desc; int32_t dim;                                      /* mDescriptorsLines [n_left][dim], dim <= 128                                */
  int32_t reserved;
  double sx, sy;                                                       /* 1 / mnMaxX, 1 / mnMaxY (the Hough grid of lld_line_track_match)            */
} lld_frame_lines;
/* Uploads the frame's lines ONCE (and fills the 50 x 50 Hough grid cells on the device); NULL or n_left = 0: a frame without lines.  Resets the
 * tracking state of the frame.  Call it after lld_frame_create and before lld_frame_track_motion_model; synchronous.
 * Line limit: LLD_ERR_UNSUPPORTED (the frame unchanged) above the most lines the chain can track next to the frame's nt keypoints.  TrackLocalMap's
 * "already seen / tracked" test keeps two hash tables in 150 KB of LDS, pow2(4 max(nt, 1)) point slots and pow2(4 n_left + 32) line slots
 * (pow2: the next power of two, at least 64), and PoseOptimization takes at most 16384 lines: n_left <= 4088 for every nt <= LLD_ORB_MAX_KEYPOINTS,
 * n_left <= 8184 when nt <= 1024. */
int  lld_frame_set_lines(lld_frame* frame, const lld_frame_lines* lines);
typedef struct {
  int32_t n;
  const double* x0; const double* dir;                                 /* [n][3] MapLine::GetMinimalPos                                              */
  const double* x1; const double* x2;                                  /* [n][3] GetMainPoints3D                                                     */
  const uint8_t* skip;                                                 /* [n] or NULL: NULL entry / isBad (src/Tracking.cc:1018-1034)                */
  const float* desc;                                                   /* [n][dim] descs[i] / mLastFrame.mDescriptorsLines.row(i)                    */
  const int32_t* id;                                                   /* [n] >= 0                                                                   */
} lld_map_lines;
typedef struct {
  lld_camera cam;                   /* PoseOptimization's intrinsics (fx, fy, cx, cy, bf as doubles of the Frame's floats)                           */
  lld_pose_params pose;             /* gamma, 4 x 10 iterations                                                                                      */
  float   th_motion;                /* 7 (stereo) / 15 (src/Tracking.cc:899-903)                                                                     */
  float   th_local;                 /* 1; 3 RGBD; 5 after a relocalisation (:1652-1658)                                                              */
  float   nnratio_local;            /* 0.8 (:1651)                                                                                                   */
  float   viewing_cos_limit;        /* 0.5 (:1646)                                                                                                   */
  int32_t direction;                /* lld_orb_search_last_frame's: +1 bForward, -1 bBackward, 0 neither                                             */
  int32_t check_orientation;        /* 1: ORBmatcher(0.9, true) (:888)                                                                               */
  int32_t wide_retry;               /* 1: search again with 2 * th_motion when the first search finds < 20 (:907-911), decided on the device          */
  int32_t monocular;                /* 0 (the chain is the stereo system's)                                                                          */
  double  line_thr_reproj_base;     /* 2 (:924, :1140)                                                                                               */
  double  line_md_thr;              /* mdThr                                                                                                         */
  int32_t line_use_grid;            /* as lld_line_track_params.use_grid                                                                             */
  int32_t reserved;
} lld_track_params;
void lld_track_params_default(lld_track_params* p);     /* cam is zeroed: the caller sets it (the track calls refuse fx, fy <= 0) */
typedef struct {
  double  pose_qt[7];               /* mTcw after the stage's PoseOptimization (pFrame->SetPose, Optimizer.cc:918)                                   */
  double  chi2;
  int32_t n_inliers;                /* PoseOptimization's return value                                                                               */
  int32_t lm_iterations, lm_trials, n_edges;
  int32_t n_search_first;           /* nmatches of the (first) search                                                                                */
  int32_t n_search;                 /* nmatches of the search whose matches the frame took (stage 1: the wide one if used_wide)                      */
  int32_t used_wide;
  int32_t n_points;                 /* MapPoints the frame holds after the stage's discard (stage 1: `nmatches`, :952)                               */
  int32_t n_points_map;             /* ... of which Observations() > 0 (stage 1: nmatchesMap, :955; stage 2: mnMatchesInliers, :1164)                */
  int32_t n_lines_matched;          /* MapLines the frame held when PoseOptimization started (lcnt_init / lcnt, :926-932, :1142-1149)                */
  int32_t n_lines;                  /* ... and after the outlier lines left (:962-975, :1176-1187)                                                   */
  int32_t n_discarded;
  int32_t n_point_edges;            /* nInitialCorrespondences of the stage's PoseOptimization (below 3 it returned without touching the pose, Optimizer.cc:809) */
  int32_t n_in_view;                /* stage 2: nToMatch of SearchLocalPoints (local MapPoints inside the frustum, src/Tracking.cc:1645-1649)              */
  /* caller-allocated, any may be NULL.  Ids / flags as the stage's PoseOptimization saw them, BEFORE its discard:                                   */
  int32_t* kp_point_id;             /* [nt] id of mvpMapPoints[k] or -1                                                                              */
  uint8_t* kp_outlier;              /* [nt] mvbOutlier[k] of those (the discard removes exactly the flagged ones)                                    */
  int32_t* ln_line_id;              /* [n_left] id of mvpMapLines[i] or -1                                                                           */
  uint8_t* ln_outlier;              /* [n_left] mvbOutlierLines[i] of those                                                                          */
  uint8_t* mp_in_view;              /* stage 2 only, [local_points->n] or NULL: Frame::isInFrustum of every local MapPoint that was not skipped (what the
                                       reference leaves in pMP->mbTrackInView and counts with IncreaseVisible, src/Tracking.cc:1645-1649)            */
} lld_track_result;
/* With n_search < 10 the stage-1 record describes a run the reference does not make: TrackWithMotionModel returns false there (src/Tracking.cc:913-917)
 * before AddLinesFrom, PoseOptimization and the discard, while the chain runs on.  The frame then holds only the search's matches (kp_point_id >= 0,
 * flags ignored) with the predicted pose; a caller hands the device that state with lld_frame_track_set_state before anything follows. */
/* Stage 1.  `view`: Frame::UpdatePoseMatrices of the predicted pose mVelocity * mLastFrame.mTcw (as for lld_frame_search_last_frame);
 * `pose_qt`: Converter::toSE3Quat of the same matrix (lld_se3_from_tcw_f32).  last / last_point_id: LastFrame.mvpMapPoints as for
 * lld_frame_search_last_frame plus the id of every entry; last_lines: mLastFrame.mvpMapLines (NULL: none).
 * LLD_ERR_INVALID before anything is queued when params->cam.fx or .fy is not > 0, or the frame was created without level_inv_sigma2
 * (PoseOptimization's information per level); the same for lld_frame_track_set_state. */
int  lld_frame_track_motion_model(lld_frame* frame, const lld_track_params* params, const lld_frame_view* view, const double* pose_qt,
                                  const lld_last_frame_points* last, const int32_t* last_point_id, const lld_map_lines* last_lines);
/* Stage 1 by Tracking::TrackReferenceKeyFrame (src/Tracking.cc:773-817): ORBmatcher(0.7, true).SearchByBoW(mpReferenceKF, mCurrentFrame)
 * (src/ORBmatcher.cc:159-288) -> mvpMapPoints = the matches, SetPose(mLastFrame.mTcw) (:788-789) -> Optimizer::PoseOptimization (:792) ->
 * outlier discard (:796-814), as a third entry into the chain next to lld_frame_track_motion_model: one upload of the keyframe side, no
 * host trip, no synchronisation.  The frame's FeatureVector is the one lld_frame_compute_bow left in HBM; the keyframe's arrives as CSR
 * and the node merge (:180-264) runs on the device: one wavefront per keyframe node looks its id up in the frame's node list, walks the
 * node's keyframe features in list order and keeps the node's occupancy in registers, so one pass is exact.  The rotation histogram and
 * ComputeThreeMaxima (:267-285, :1601-1642) follow in one small kernel that writes the kept matches into the frame's tables.
 * mfNNratio = 0.7 and mbCheckOrientation = true are fixed (lld_track_params has no room for them); the frame needs its angles.
 * The reference adds no lines here: the frame's line tables stay empty through stage 1, its lines stay uploaded for stage 2.
 * The stage-1 record: n_search_first = n_search = SearchByBoW's return value, used_wide = 0, n_lines_matched = n_lines = 0, the rest as
 * for lld_frame_track_motion_model.  With n_search < 15 the record describes a run the reference does not make: TrackReferenceKeyFrame
 * returns false there (:785-786) before SetPose, PoseOptimization and the discard, while the chain runs on.  The frame then holds only the
 * raw matches (kp_point_id >= 0, flags ignored) with the handed-in pose, as in the note on n_search < 10 above.
 * LLD_ERR_INVALID before anything is queued, the frame unchanged: no lld_frame_compute_bow on this frame yet, a NULL argument, n outside
 * [0, LLD_ORB_MAX_KEYPOINTS], n_nodes outside [0, n], node ids not strictly ascending, node_start not ascending from 0, feature
 * indices outside [0, n), cam.fx or cam.fy not > 0, a frame without level_inv_sigma2 or (nt > 0) without angles. */
typedef struct {
  int32_t n;                        /* keypoints of mpReferenceKF                                                                                    */
  const uint32_t* desc;             /* [n][8] pKF->mDescriptors                                                                                      */
  const float*    angle;            /* [n] pKF->mvKeysUn[k].angle                                                                                    */
  const int32_t*  point_id;         /* [n] id of GetMapPointMatches()[k], -1 = NULL or isBad (:193-197)                                              */
  const float*    world_pos;        /* [n][3] GetWorldPos() of those (ignored where the id is -1)                                                    */
  const uint8_t*  has_obs;          /* [n] Observations() > 0, or NULL: all                                                                          */
  int32_t n_nodes;                  /* pKF->mFeatVec as lld_bow_result gives it: node ids strictly ascending, CSR node_start [n_nodes + 1], feature  */
  const int32_t* node; const int32_t* node_start; const int32_t* feature;   /* a keyframe feature listed under two nodes is tolerated: it is tried in both, and the frame's
                                                                               own FeatureVector keeps every frame feature under one node, which is what exactness needs */
} lld_ref_keyframe;
/* view / pose_qt: Frame::UpdatePoseMatrices and Converter::toSE3Quat of mLastFrame.mTcw (:789), formed as for lld_frame_track_motion_model. */
int  lld_frame_track_reference_keyframe(lld_frame* frame, const lld_track_params* params, const lld_frame_view* view, const double* pose_qt,
                                        const lld_ref_keyframe* kf);
/* Stage 1 by Tracking::Relocalization (src/Tracking.cc:1837-1998) is lld_frame_relocalize, declared after lld_pnp_params below.
 * Stage 1 ran elsewhere: a caller that runs Tracking::TrackReferenceKeyFrame (src/Tracking.cc:770-816) or Tracking::Relocalization call by
 * call - they end with the same PoseOptimization + outlier discard but find their matches by bag of words / PnP - hands the device what such a
 * routine left in the frame, so that lld_frame_track_local_map can follow on the same handle (Tracking::Track runs TrackLocalMap after whichever
 * routine produced the pose, :401-407).  The record of stage 1 reads as empty afterwards. */
typedef struct {
  const int32_t* kp_point_id;       /* [nt] id of mvpMapPoints[k] or -1                                                                              */
  const float*   kp_world_pos;      /* [nt][3] GetWorldPos() of those (ignored where the id is -1)                                                   */
  const uint8_t* kp_has_obs;        /* [nt] Observations() > 0, or NULL: all                                                                         */
  const uint8_t* kp_outlier;        /* [nt] mvbOutlier, or NULL: none                                                                                */
  int32_t        n_seen;            /* MapPoints with mnLastFrameSeen == mCurrentFrame.mnId the frame does not hold (the discard's, :805-808); <= nt */
  const int32_t* seen_point_id;
  const int32_t* ln_line_id;        /* [n_left] id of mvpMapLines[i] or -1; NULL: the frame holds no lines (TrackReferenceKeyFrame adds none)        */
  const double*  ln_x0;             /* [n_left][3] GetMinimalPos of those                                                                            */
  const double*  ln_dir;
  const uint8_t* ln_outlier;        /* [n_left] mvbOutlierLines, or NULL: none                                                                       */
  int32_t        n_tracked;         /* further MapLines with tracked_last_id == mCurrentFrame.mnId (<= n_left + 16 together with the held ones)      */
  const int32_t* tracked_line_id;
} lld_frame_held;
/* view / pose_qt: Frame::UpdatePoseMatrices and Converter::toSE3Quat of the frame's mTcw, as for lld_frame_track_motion_model. */
int  lld_frame_track_set_state(lld_frame* frame, const lld_track_params* params, const lld_frame_view* view, const double* pose_qt, const lld_frame_held* held);
/* Stage 2, on the pose and the MapPoints / MapLines stage 1 left in the frame.  local_points->skip: isBad only - what the frame holds or
 * discarded is skipped by id on the device.  local_lines: Tracking::local_lines with their descriptors (NULL: none). */
int  lld_frame_track_local_map(lld_frame* frame, const lld_track_params* params, const lld_map_points* local_points, const int32_t* local_point_id,
                               const lld_map_lines* local_lines);
/* Waits for the queued stages and fetches their records (either may be NULL; stage2 is meaningful only after lld_frame_track_local_map). */
int  lld_frame_track_download(lld_frame* frame, lld_track_result* stage1, lld_track_result* stage2);
/* ------------------------------------------------------------------ the frame's lines, matched and turned into map lines on the device
 * lld_frame_build_lines: what the Frame constructor does with its two line sets (src/Frame.cc:121-122: TwoFrameLineMatcher::MatchLines with
 * T = identity, T_right = GetTForRight) and what lld_frame_set_lines does with the result, in one call that leaves Frame::line_matches in HBM
 * where the chain reads it.  Both line sets, both octave arrays and both descriptor sets travel in ONE copy from a pinned buffer the frame
 * owns; the Hough-cell fill, CheckLinePair's gates and distances (the kernels of lld_line_match_stereo) and the in-order greedy assignment
 * are queued on the context's stream and the call returns: lld_frame_track_* follow on the same stream, nothing goes through the host.  The
 * call waits for the stream first only when the frame already has a tracking state (which it replaces, as lld_frame_set_lines does).
 * The result is bit-identical to lld_line_match_stereo followed by lld_frame_set_lines on the same arrays: same matches, same cells, same
 * reset of the tracking state.  n_right = 0: every left line gets -1 and no matching kernel is launched.  lines = NULL or n_left = 0: a
 * frame without lines.  The right descriptors are read by the match only; they stay allocated with the frame's line block (n_right * dim
 * floats) but nothing reads them afterwards.
 * Refused before anything is queued, the frame unchanged: LLD_ERR_INVALID for a NULL frame or required array, a negative count, dim <= 0,
 * sx or sy not > 0, an octave outside 0..64; LLD_ERR_UNSUPPORTED for n_left above lld_frame_set_lines' line limit, dim > LLD_LINE_DIM_MAX,
 * n_right * 8 + dim * 4 > LLD_LINE_LDS_CEILING or (n_left + n_right) * 4 + 16 > LLD_LINE_LDS_CEILING (see lld_line_match_greedy). */
typedef struct {
  int32_t n_left;  const float* left;  const int32_t* left_octave;  const float* desc_left;    /* mvLinesLeft, mDescriptorsLines [n_left][dim]  */
  int32_t n_right; const float* right; const int32_t* right_octave; const float* desc_right;   /* mvLinesRight, mDescriptorsLinesRight           */
  int32_t dim, reserved;
  double  sx, sy;                    /* as lld_frame_lines */
  lld_line_stereo_params stereo;     /* K, b, tau, min_line_length, is_stereo: as lld_line_match_stereo */
} lld_frame_lines_build;
int  lld_frame_build_lines(lld_frame* frame, const lld_frame_lines_build* lines);
/* Waits for the frame's queued work and fetches Frame::line_matches (and, when match_dist is not NULL, the accepted descriptor distances) in
 * one copy: the host needs them for KeyFrame::line_matches and the counts at src/Tracking.cc:978.  On a frame whose lines came from
 * lld_frame_set_lines: the uploaded line_matches, and match_dist filled with lld_line_match_stereo's "no distance" value (DBL_MAX).  A frame
 * without lines: LLD_OK, nothing is written. */
int  lld_frame_lines_download(lld_frame* frame, int32_t* line_matches /*[n_left]*/, double* match_dist /*[n_left] or NULL*/);
/* Tracking::MatchLinesLastKF (src/Tracking.cc:1449-1611, called from CreateNewKeyFrame :1433) between two RESIDENT frames: the kernel of
 * lld_line_match_last_frame on what the two handles already hold - both frames' lines, line_matches, Hough cells, octaves and descriptors -
 * with nothing uploaded but this parameter struct.
 *   cameras       each frame's camera-to-world R, t and right-camera centre as its chain left them in device memory after its last stage
 *                 (or lld_frame_track_set_state): [Rwc | Ow] widened to double instead of mTcw.inv(), the deviation AddLinesFrom documents
 *                 above; K, b, sx, sy are the current frame's;
 *   cur_occupied  mCurrentFrame.mvpMapLines[i] != NULL (:1477): the lines the current frame holds now;
 *   last_skip     mLastFrame.mvpMapLines[li] && ...->tracked_last_id == mCurrentFrame.mnId (:1518): the last frame holds a line on li whose id
 *                 is among the lines the current frame tracked (by id, on the device, against the table TrackLocalMap's skip test uses).
 * A second kernel numbers the created lines in ascending i - the reference's creation order - first_new_id + rank (the caller passes
 * MapLine::nNextId), and writes them into the current frame's state (held, id, X0, direction; mvbOutlierLines as it is): the handle then
 * holds what mCurrentFrame.mvpMapLines holds after :1602, and when this frame is the next call's `last`, that call sees them.
 * ml->tracked_last_id = mnId (:1603) has no reader left in this frame's life (no AddLinesFrom follows CreateNewKeyFrame on it), so the
 * frame's tracked table is left alone: its capacity and the hash budget of TrackLocalMap's skip test do not change.
 * One download, one wait.  Stereo only, like lld_line_match_last_frame.  The stage records of lld_frame_track_download predate this call.
 * LLD_ERR_INVALID, both frames unchanged: a NULL argument, cur == last, frames of different contexts or different dim, a frame without
 * lines or without a pose (no lld_frame_track_* stage and no lld_frame_track_set_state has run on it), first_new_id < 0 or
 * first_new_id + n_left > INT32_MAX. */
typedef struct {
  double  thr_reproj_base;          /* 6 px (Tracking.cc:1451) */
  double  md_thr;                   /* mdThr */
  int32_t use_grid;                 /* as lld_line_lastkf_params.use_grid */
  int32_t first_new_id;             /* MapLine::nNextId */
} lld_frame_new_lines_params;
typedef struct {
  int32_t n_created;                /* mapline_cnt */
  int32_t n_held;                   /* cnt0: lines the frame held on entry; the reference returns n_created + n_held (:1610) */
  /* caller-allocated [n_left] / [n_left][3] of the current frame, as lld_line_match_last_frame; any may be NULL */
  int32_t* match_last; uint8_t* created; double* x0; double* dir;
  int32_t* new_id;                  /* [n_left] id given to a created line, else -1; may be NULL */
} lld_frame_new_lines_result;
int  lld_frame_new_map_lines(lld_frame* cur, lld_frame* last, const lld_frame_new_lines_params* params, lld_frame_new_lines_result* out);
/* ------------------------------------------------------------------ the tail of Tracking::Track on the resident frame: keyframe decision, new stereo points
 * lld_frame_track_finish: what Tracking::Track does with mCurrentFrame after TrackLocalMap succeeded (src/Tracking.cc:429-476), in ONE kernel
 * on the arrays the chain left in HBM - mvDepth and mvKeysUn of the built frame, kp_has / kp_id / kp_obs / kp_outlier, the view and stage 2's
 * record of the tracking state - queued on the context's stream like the stages; the only wait is the fetch of the result (one copy).
 * In the reference's order:
 *   1. Clean VO matches (:446-453): a keypoint whose MapPoint has no observations loses it, and its mvbOutlier flag is cleared.
 *   2. NeedNewKeyFrame's counts (:1250-1264): a keypoint is close when depth > 0 && depth < th_depth (strict); a close keypoint that holds a
 *      MapPoint and is no outlier counts as n_tracked_close, every other close keypoint as n_non_tracked_close.  (monocular != 0: both stay 0, :1252.)
 *   3. NeedNewKeyFrame's decision (:1227-1309) from the scalars below, in the reference's types: frame ids summed in 64 bits,
 *      mnMatchesInliers < nRefMatches*0.25 in double, mnMatchesInliers < nRefMatches*thRefRatio in float with thRefRatio 0.75f, 0.4f when
 *      n_keyframes < 2, 0.9f when monocular.  need = its return value; interrupt_ba = 1 when the reference calls mpLocalMapper->InterruptBA() (:1296) -
 *      the caller must then call it; made = need && set_not_stop_ok (CreateNewKeyFrame returns at once when SetNotStop(true) fails, :1369).
 *      force = 0 / 1 replaces `made` for a caller that decides elsewhere (-1: the decision above); need and interrupt_ba are reported either way.
 *   4. If made, CreateNewKeyFrame's points (:1386-1430).  The candidates are the keypoints with depth > 0 in the order std::sort gives
 *      pair<float,int>: by depth, equal depths by index (+inf sorts last, NaN and depth <= 0 never enter).  Every visited entry increments nPoints
 *      whether or not a point is made, so entry j (from 0) is visited iff j <= J, J the first j >= 100 with depth_j > th_depth (strict, and NOT the
 *      count's inequality: a depth equal to th_depth is neither close nor a reason to stop); the entry that stops the loop is itself processed.
 *      A visited keypoint gets a new MapPoint when it holds none or one without observations.  Its position is Frame::UnprojectStereo
 *      (src/Frame.cc:730-744): x = (u-cx)*z*invfx, y = (v-cy)*z*invfy in float with invfx = 1.0f/fx, (u, v) = mvKeysUn, then mRwc*x3Dc + mOw with
 *      the frame's own view as stage 2 left it (Rwc = Rcw^T).  The matrix step is the library's un-projection of lld_new_points_triangulate: float
 *      products summed in double in index order, one rounding, then the float addition of mOw; bit parity with OpenCV's gemm is not pinned, as
 *      for every cv::Mat product restated in this header.  New ids are first_new_id + k, k the rank among the created points in visiting order
 *      (the caller passes MapPoint::nNextId and news its MapPoints in that order).  The state takes kp_has = 1, kp_id, kp_world, kp_obs = 1
 *      (AddObservation(pKF, i), :1415); kp_outlier stays as it is.
 *   5. Drop outliers (:472-476), whenever the call runs: a keypoint that holds a MapPoint and is flagged loses it.
 * RGB-D: TrackLocalMap takes its outlier MapPoints out of the frame for mSensor == System::STEREO only (:1171-1172), and stage 2 of the chain
 * always does.  With sensor_rgbd != 0 the call first puts back what stage 2 took out (the ids and flags of its record; positions and
 * observation flags never left the state), so that steps 1-5 see the frame the reference's RGB-D system sees: such a keypoint counts as not
 * tracked, gets no new point while its MapPoint has observations, and loses it in step 5.  After lld_frame_track_set_state there is no
 * stage-2 record and the state is taken as handed in.
 * The handle then holds what mCurrentFrame holds when Track() returns: lld_frame_new_map_lines may follow on it with nothing in between, and
 * the frame can serve as the next frame's `last`.  The stage records of lld_frame_track_download predate this call.
 *
 * lld_frame_create_stereo_points: the same depth-ordered creation, by the same kernel, where the reference runs it outside Track()'s tail:
 *   LLD_POINTS_LAST_FRAME       Tracking::UpdateLastFrame's "visual odometry" points (:830-882): view / pose_qt (both or neither; formed as for
 *                               lld_frame_track_motion_model) first replace the frame's pose (mLastFrame.SetPose, :825); the visiting rule is 4.; the
 *                               new points are temporal: kp_obs = 0 (MapPoint(x3D, mpMap, &mLastFrame, i) adds no observation).  No cleaning, no
 *                               decision, no outlier drop.  The frame needs a pose (a stage, or lld_frame_track_set_state, or view here).
 *   LLD_POINTS_INITIALIZATION   Tracking::StereoInitialization (:535-550): every keypoint with depth > 0 gets a point, in index order, ids in index
 *                               order, kp_obs = 1.  view / pose_qt are required (SetPose(eye), :526: the identity); the tracking state is reset
 *                               to that of a new frame first, and a frame without a tracking state gets one.  th_depth is not read.
 * Wherever view is given, `params` is required as for lld_frame_track_set_state (the line camera of the new pose is formed from it).
 * n_tracked_close, n_non_tracked_close, need and interrupt_ba read 0; made reads 1.
 *
 * Depth: the frame's own mvDepth when a device build made it (lld_frame_build_stereo*, lld_frame_build_mono* - without a depth image every
 * depth is -1 and nothing is close or created); for a frame of lld_frame_create, which keeps no depth, the host array depth[nt] (uploaded with
 * the call; ignored on a built frame).
 * LLD_ERR_INVALID before anything is queued, the frame unchanged: a NULL frame, params or out; no depth from either source;
 * lld_frame_track_finish on a frame whose last chain call was neither lld_frame_track_local_map nor lld_frame_track_set_state; th_depth not > 0
 * (finish and LLD_POINTS_LAST_FRAME); first_new_id < 0 or first_new_id + nt > INT32_MAX; force outside -1..1; an unknown mode; one of view / pose_qt
 * without the other, or view without params (or with params lld_frame_track_set_state refuses); LLD_POINTS_LAST_FRAME on a frame without a
 * pose; LLD_POINTS_INITIALIZATION without view.
 * nt = 0 or no positive depth: LLD_OK with zeros. */
typedef struct {
  float   th_depth;                 /* mThDepth                                                                                                      */
  int32_t first_new_id;             /* MapPoint::nNextId                                                                                             */
  int32_t force;                    /* -1: made = need && set_not_stop_ok; 0 / 1: made = force                                                       */
  int32_t only_tracking;            /* mbOnlyTracking (:1227)                                                                                        */
  int32_t mapper_stopped;           /* mpLocalMapper->isStopped() || stopRequested() (:1231)                                                         */
  int32_t mapper_idle;              /* mpLocalMapper->AcceptKeyFrames() (:1247)                                                                      */
  int32_t keyframes_in_queue;       /* mpLocalMapper->KeyframesInQueue() (:1299)                                                                     */
  int32_t set_not_stop_ok;          /* mpLocalMapper->SetNotStop(true) (:1369); the caller evaluates it only when need is possible, or undoes it    */
  int32_t monocular;                /* mSensor == System::MONOCULAR                                                                                  */
  int32_t max_frames, min_frames;   /* mMaxFrames, mMinFrames                                                                                        */
  int32_t n_keyframes;              /* mpMap->KeyFramesInMap() (:1234)                                                                               */
  int32_t n_ref_matches;            /* mpReferenceKF->TrackedMapPoints(nMinObs), nMinObs = n_keyframes <= 2 ? 2 : 3 (:1241-1244)                     */
  int32_t n_matches_inliers;        /* mnMatchesInliers; -1: n_points_map of the frame's own stage-2 record                                          */
  int32_t sensor_rgbd;              /* mSensor == System::RGBD: see "RGB-D" above                                                                     */
  int32_t reserved;
  int64_t frame_id;                 /* mCurrentFrame.mnId                                                                                            */
  int64_t last_reloc_frame_id;      /* mnLastRelocFrameId                                                                                            */
  int64_t last_keyframe_id;         /* mnLastKeyFrameId                                                                                              */
  const float* depth;               /* [nt] mvDepth for a frame of lld_frame_create, else NULL                                                       */
} lld_frame_finish_params;
typedef struct {
  int32_t n_tracked_close, n_non_tracked_close;   /* nTrackedClose, nNonTrackedClose                                                                 */
  int32_t need, interrupt_ba, made;
  int32_t n_visited;                /* entries of the sorted list the creation loop processed (0 when made = 0)                                      */
  int32_t n_created;
  int32_t reserved;
  /* caller-allocated, any may be NULL */
  uint8_t* created;                 /* [nt] 1 where a MapPoint was made                                                                              */
  int32_t* new_id;                  /* [nt] its id, -1 where none                                                                                    */
  float*   x3d;                     /* [nt][3] its position, 0 where none                                                                            */
  int32_t* kp_point_id;             /* [nt] what the frame holds on exit: id of mvpMapPoints[k] or -1                                                */
  int32_t* order;                   /* [nt] rank of the keypoint in the visiting order, -1 when it was not visited                                   */
} lld_frame_finish_result;
int  lld_frame_track_finish(lld_frame* frame, const lld_frame_finish_params* params, lld_frame_finish_result* out);
#define LLD_POINTS_LAST_FRAME     0
#define LLD_POINTS_INITIALIZATION 1
typedef struct {
  int32_t mode;                     /* LLD_POINTS_LAST_FRAME / LLD_POINTS_INITIALIZATION                                                             */
  float   th_depth;                 /* mThDepth                                                                                                      */
  int32_t first_new_id;             /* MapPoint::nNextId                                                                                             */
  int32_t reserved;
  const lld_track_params* params;   /* required with view, else may be NULL                                                                          */
  const lld_frame_view* view;       /* NULL: the frame's pose stays (LLD_POINTS_LAST_FRAME only)                                                     */
  const double* pose_qt;            /* [7] with view                                                                                                 */
  const float* depth;               /* as lld_frame_finish_params.depth                                                                              */
} lld_frame_points_params;
int  lld_frame_create_stereo_points(lld_frame* frame, const lld_frame_points_params* params, lld_frame_finish_result* out);
/* ORBmatcher::Fuse(KeyFrame*, vpMapPoints, th) (src/ORBmatcher.cc:825-958; the loop of LocalMapping::SearchInNeighbors) with the
 * projection loop (:841-890) on the device: cv::gemm transform, z >= 0, invz = 1/z, u = fx*(x*invz)+cx, KeyFrame::IsInImage
 * (upper bounds strict, src/KeyFrame.cc:633-636), ur = u - bf*invz, scale-invariance band, PO.dot(Pn) >= 0.5*dist3D, PredictScale;
 * then the window search with the level and reprojection-chi2 gates and `bestDist <= TH_LOW`.  `points`: as for
 * lld_orb_search_local_points; skip[i] = !pMP || isBad || IsInKeyFrame(pKF); has_obs is ignored (no occupancy in Fuse).
 * out->match[i] = bestIdx or -1, out->n_matches = nFused; the replace / add bookkeeping (:936-954) stays with the caller. */
int lld_orb_fuse_search(lld_ctx* ctx, const lld_orb_search* keyframe, const lld_frame_view* view, const lld_map_points* points,
                        float th, float* proj_uvr_or_null, lld_orb_search_result* out);
/* The matchers of relocalisation and loop closing WITH their projection loops on the device (round 3; before, the searches were
 * mirrored and the per-query projections stayed with the adapter).  One entry point, four routines:
 *   LLD_ORB_PROJ_KF_SIM3    ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)      src/ORBmatcher.cc:290-403
 *                           (LoopClosing::ComputeSim3): z >= 0, invz = 1/z, u = fx*(x*invz)+cx, KeyFrame::IsInImage, distance band,
 *                           PO.dot(Pn) >= 0.5*dist, PredictScale, radius = th*scale[level], levels [l-1, l], keypoints with
 *                           vpMatched[idx] skipped (frame->t_occupied) and taken ones blocking later points, bestDist <= TH_LOW.
 *   LLD_ORB_PROJ_RELOC      ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)  :1472-1599
 *                           (Tracking::Relocalization): NO depth test, invzc = float(1.0/z), u = fx*xc*invzc+cx, frame bounds
 *                           (u<min || u>max), distance band, PredictScale, radius = th*scale, levels [l-1, l+1], occupied keypoints
 *                           (CurrentFrame.mvpMapPoints[i2], frame->t_occupied) skipped and blocking, bestDist <= accept_max (ORBdist),
 *                           rotation histogram over `angle` (pKF->mvKeysUn[i].angle) when check_orientation.
 *   LLD_ORB_PROJ_FUSE_SIM3  ORBmatcher::Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint)                :977-1100
 *                           (LoopClosing::SearchAndFuse): projection as KF_SIM3, levels [l-1, l], no occupancy, bestDist <= TH_LOW;
 *                           match[i] = bestIdx, the replace / add bookkeeping (:1078-1093) stays with the caller.
 *   LLD_ORB_PROJ_SIM3_DIR   one direction of ORBmatcher::SearchBySim3                                     :1147-1224 / :1227-1304
 *                           p3Dc1 = R1w*p3Dw+t1w (view), p3Dc2 = sR*p3Dc1+t (second cv::gemm, `sR`, `t` below), z >= 0, IsInImage,
 *                           dist3D = cv::norm(p3Dc2), band, PredictScale, levels [l-1, l], bestDist <= TH_HIGH.  view->fx.. are pKF1's in
 *                           both directions (:1105-1108), the bounds and the scale pyramid those of the keyframe searched in.
 * `view` carries the DECOMPOSED transform (Rcw = sRcw/scw, tcw = Scw.col(3)/scw, Ow = -Rcw.t()*tcw, :298-303 - three OpenCV calls
 * that stay with the adapter) and the intrinsics / image bounds of the keyframe or frame searched in; `points`: as for
 * lld_orb_search_local_points (normal may be NULL for RELOC and SIM3_DIR; skip[i] = isBad / already found / vbAlreadyMatched;
 * has_obs is ignored).  proj_uv [n][2] and level [n] (either may be NULL) return u, v and nPredictedLevel of the points that reach
 * the window search.  Same OpenCV restatement as above (parity unpinned), bit-identical between device and oracle. */
#define LLD_ORB_PROJ_KF_SIM3   0
#define LLD_ORB_PROJ_RELOC     1
#define LLD_ORB_PROJ_FUSE_SIM3 2
#define LLD_ORB_PROJ_SIM3_DIR  3
typedef struct {
  int32_t routine;
  float   th;
  int32_t accept_max;         /* RELOC: ORBdist; ignored by the other routines (TH_LOW / TH_HIGH as listed) */
  int32_t check_orientation;  /* RELOC only */
  float   sR[9], t[3];        /* SIM3_DIR: sR21, t21 (KF1 -> KF2) or sR12, t12 (KF2 -> KF1), row-major */
} lld_orb_projection;
int lld_orb_search_projected(lld_ctx* ctx, const lld_orb_search* frame, const lld_frame_view* view, const lld_map_points* points,
                             const float* angle_or_null, const lld_orb_projection* proj, float* proj_uv_or_null, int32_t* level_or_null,
                             lld_orb_search_result* out);
/* ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1102-1326) as a whole: both directions (two LLD_ORB_PROJ_SIM3_DIR searches) and the
 * agreement check (:1306-1322).  kf1 / view1 / points1: KF1's keypoints, its pose (R1w, t1w) and its MapPoints per keypoint
 * (skip[i] = !pMP || vbAlreadyMatched1[i] || isBad), likewise KF2; sR12, t12, sR21, t21 as the reference forms them (:1121-1124).
 * match12[i1] = index of the KF2 keypoint whose MapPoint becomes vpMatches12[i1], or -1; returns nFound in *n_found. */
int lld_orb_search_by_sim3(lld_ctx* ctx, const lld_orb_search* kf1, const lld_frame_view* view1, const lld_map_points* points1,
                           const lld_orb_search* kf2, const lld_frame_view* view2, const lld_map_points* points2,
                           const float* sR12, const float* t12, const float* sR21, const float* t21, float th,
                           int32_t* match12 /* [points1->n] */, int32_t* n_found);
/* ------------------------------------------------------------------ Frame::ComputeStereoMatches, whole routine
 * src/Frame.cc:530-704: (1) the row-band Hamming search (:536-613, the ROWS problem of lld_orb_search_run with the level gate
 * octave +-1, disparity range [0, mbf/mb] and bestDist < (TH_HIGH+TH_LOW)/2), (2) the sub-pixel refinement (:615-688): 11x11
 * patch of the left pyramid level around the rounded scaled keypoint, centre pixel subtracted, L1 distance to the right patch slid
 * over incR = -5..5, first minimum (int bestDist, strict <), parabola through the three distances around it, |deltaR| <= 1,
 * bestuR = scale * (scaleduR0 + bestincR + deltaR), 0 <= disparity < mbf/mb (disparity <= 0 -> 0.01), (3) the outlier cut
 * (:690-703): median of the SAD distances, entries with dist >= 1.5f*1.4f*median are cleared.
 * All of it is integer / single-rounding float work: results are bit-exact against the CPU restatement.
 * Deviation: the reference slices cv::Mat ranges unchecked (OpenCV aborts when a patch leaves the image; ORB keeps keypoints
 * 19 px inside); here such a keypoint simply gets no stereo match.  Likewise unchecked in the reference: vRowIndices[kp.pt.y] (:569)
 * for a left keypoint whose row (long long)vL is not a row of level 0; here, on both routes (this call and lld_frame_build_stereo*),
 * such a keypoint has no candidate row: best_r = -1, no match. */
typedef struct {
  int32_t n;
  const float*    xy;           /* [n][2] mvKeys / mvKeysRight .pt */
  const int32_t*  octave;       /* [n]                              */
  const uint32_t* desc;         /* [n][8]                           */
} lld_keypoints;
typedef struct {
  int32_t n_levels;
  const uint8_t* const* left;   /* [n_levels] mpORBextractorLeft->mvImagePyramid[l].data (CV_8U)  */
  const uint8_t* const* right;  /* [n_levels] mpORBextractorRight->mvImagePyramid[l].data         */
  const int32_t* cols;          /* [n_levels]                                                       */
  const int32_t* rows;          /* [n_levels]                                                       */
  const int32_t* left_step;     /* [n_levels] bytes per image row (cv::Mat::step)                   */
  const int32_t* right_step;
  const float*   scale_factors;     /* [n_levels] mvScaleFactors    */
  const float*   inv_scale_factors; /* [n_levels] mvInvScaleFactors */
  int32_t on_device;            /* 1: the image pointers are HBM pointers (e.g. of a device ORB extractor), nothing is uploaded */
  int32_t reserved;
} lld_stereo_pyramids;
typedef struct {
  float*   u_right;             /* [n_left] mvuRight (-1 = none)                                   */
  float*   depth;               /* [n_left] mvDepth  (-1 = none)                                   */
  int32_t* best_r;              /* [n_left] or NULL: bestIdxR of the Hamming stage, -1 = none      */
  int32_t* sad;                 /* [n_left] or NULL: bestDist of the refinement as pushed into vDistIdx, -1 = not pushed */
  int32_t  n_matches;           /* entries of vDistIdx that survive the median cut                 */
  int32_t  reserved;
} lld_stereo_result;
int lld_compute_stereo_matches(lld_ctx* ctx, const lld_keypoints* left, const lld_keypoints* right, const lld_stereo_pyramids* pyr,
                               float mb, float mbf, lld_stereo_result* out);
/* `n` independent problems (e.g. one relocalisation / loop candidate keyframe each, or the searches of several frames) in one
 * launch: one workgroup per problem, all inputs moved in one host-to-device copy and all outputs in one copy back. */
int lld_orb_search_batch(lld_ctx* ctx, int n, const lld_orb_search* problems, lld_orb_search_result* outs);


/* ------------------------------------------------------------------ ORBextractor::operator(), whole routine
 * src/ORBextractor.cc:1043-1105 with what it calls: ComputePyramid (:1107-1132), ComputeKeyPointsOctTree (:765-852),
 * DistributeOctTree (:539-763, DivideNode :480-537), computeOrientation / IC_Angle (:77-104), the blur (:1085-1086) and
 * computeOrbDescriptor (:108-148).  A handle holds the level tables, the device buffers (sized once from max_cols / max_rows /
 * max_images) and the last pyramid, which lld_compute_stereo_matches can read in place (lld_orb_extractor_pyramids).
 * Everything is integer or single-rounding float work: results are bit-exact against the CPU restatement
 * (tests/orb_extract_ref.py).  OpenCV is restated as follows (parity with OpenCV itself unpinned):
 *   Level tables (:411-470): mvScaleFactor[l] = cumulative float products, inverse = 1.0f / factor, sigma2 = factor^2;
 *     nDesiredFeaturesPerScale = nfeatures*(1-f)/(1-(float)pow((double)f, n_levels)) in float (f = 1.0f/scale_factor),
 *     mnFeaturesPerLevel[l] = cvRound of it (then *= f), the remainder (>= 0) to the last level; umax as the constructor.
 *   Pyramid: level 0 is the image; level l = resize(level l-1) to cvRound((float)cols*inv[l]) x cvRound((float)rows*inv[l])
 *     (cvRound = round half to even).  Bilinear, 8-bit fixed point: per axis scale = 1.0/((double)dsize/ssize),
 *     f = (float)((d+0.5)*scale - 0.5) in double without contraction, s = floor(f), f -= s; s < 0 -> s = 0, f = 0;
 *     s >= ssize-1 -> s = ssize-1, f = 0; c1 = cvRound(f*2048), c0 = 2048-c1 (11-bit coefficients); horizontal pass
 *     h = c0*S[s] + c1*S[s+1] on the two source rows, vertical v = b0*h0 + b1*h1, pixel = (v + 2^21) >> 22.  The bordered copy
 *     (copyMakeBorder) is never read by the extractor or the stereo SAD and is not kept.
 *   FAST (:765-832): score(p) = (largest m such that 9 contiguous pixels of the 16-pixel Bresenham circle of radius 3 all differ
 *     from p by >= m in the same direction) - 1; p is a corner at threshold t iff score >= t (strict > p+t / < p-t).  Per 30-px
 *     cell (the reference's wCell / hCell, +6 overlap, asymmetric skips iniY >= maxBorderY-3 and iniX >= maxBorderX-6, clipping
 *     to maxBorder) detection and non-maximum suppression run INSIDE the cell's sub-image: only pixels >= 3 from its edges are
 *     tested, a neighbour outside that interior or not a corner at the cell's threshold counts as 0, a corner is kept iff its score
 *     is > all 8 neighbours.  Row-major within a cell, cells row-major; a pixel in the overlap of two cells appears twice (both
 *     kept).  min_th_fast is retried only in cells that found nothing at ini_th_fast.  response = (float)score.
 *   DistributeOctTree: the reference's list semantics (push_front of n1..n4, erasure of split nodes, bNoMore at size 1, stop at
 *     size >= N or unchanged size, sorted phase from the largest node down breaking at size >= N; each node keeps the first key of
 *     strictly greatest response in candidate order).  DEVIATION (the reference is not deterministic here): its sort of
 *     pair<size, ExtractorNode*> orders nodes of equal size by heap address; here a node created later counts as the larger, i.e.
 *     equal sizes are split in reverse creation (push) order.  A level returns up to max(N+3, 4*nIni) keypoints (no trimming;
 *     N+3 whenever 4*round(w/h) <= N+3, e.g. for every level of KITTI at nfeatures = 2000).
 *   IC_Angle: integer moments over the umax disc of the unblurred level; fastAtan2 as OpenCV's float polynomial (degrees, [0,360)):
 *     c = min/(max + (float)DBL_EPSILON), a = (((p7 c^2 + p5) c^2 + p3) c^2 + p1) c with p_k = (float)coef_k * (float)(180/pi),
 *     90-a when |y| > |x|, 180-a for x < 0, 360-a for y < 0; every float operation rounded separately.
 *   Blur: GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) restated as a documented integer filter (not OpenCV's own fixed point):
 *     separable Q8 kernel {18, 34, 49, 54, 49, 34, 18} (round(256*g_i) of the normalised Gaussian, the centre lowered by one so the
 *     taps sum to 256), horizontal then vertical in exact integers, pixel = (sum + 32768) >> 16, reflect-101 on the level's pixels.
 *   Descriptor: a = cosf(angle*factorPI), b = sinf(...) as glibc >= 2.28 computes them (restated in csrc/lld_glibc_sincosf.h,
 *     checked equal to this host's libm for every float angle in [0, 360): profiles/orb_sincosf_check.txt); offsets
 *     cvRound(x*b + y*a), cvRound(x*a - y*b) with every float operation rounded separately (no FMA).
 * Size limits: 62 <= each level's cols and rows (every level must give nCols, nRows and round(w/h) >= 1; checked on the host),
 * cols, rows <= max_cols, max_rows <= 16383; 1 <= n_levels <= LLD_ORB_MAX_LEVELS; thresholds in [1, 255]; 1 < scale_factor;
 * pattern coordinates |c| <= 13 (13*sqrt(2) rounds below EDGE_THRESHOLD = 19, so no descriptor read leaves the level).
 * No limit on the candidate count: every per-level buffer is sized at create time from the level's area, with room for the
 * cells' rounding (nCols * wCell may exceed the level's width). */
typedef struct lld_orb_extractor lld_orb_extractor;
typedef struct {
  int32_t nfeatures;
  float   scale_factor;
  int32_t n_levels;
  int32_t ini_th_fast;
  int32_t min_th_fast;
  int32_t max_cols, max_rows;     /* largest level-0 image a call may pass            */
  int32_t max_images;             /* images per lld_orb_extract call (e.g. 2: stereo) */
  const int32_t* pattern;         /* [512][2] = ORBextractor::pattern (256 point pairs, x then y), copied at create */
} lld_orb_extractor_params;
typedef struct {
  int32_t n_levels;
  int32_t max_keypoints;          /* capacity an lld_orb_features must have for an image of max_cols x max_rows:
                                     sum over levels of max(N_l + 3, 4*nIni_l); nfeatures + 3*n_levels for the usual sizes */
  float   scale_factor[LLD_ORB_MAX_LEVELS];       /* mvScaleFactor    */
  float   inv_scale_factor[LLD_ORB_MAX_LEVELS];   /* mvInvScaleFactor */
  float   level_sigma2[LLD_ORB_MAX_LEVELS];       /* mvLevelSigma2    */
  float   inv_level_sigma2[LLD_ORB_MAX_LEVELS];   /* mvInvLevelSigma2 */
  int32_t features_per_level[LLD_ORB_MAX_LEVELS]; /* mnFeaturesPerLevel */
  int32_t umax[16];                               /* HALF_PATCH_SIZE + 1 entries */
} lld_orb_extractor_levels;
typedef struct {
  const uint8_t* data;            /* CV_8UC1 pixels, host or (on_device = 1) HBM */
  int32_t cols, rows, step;       /* step: bytes per row                         */
  int32_t on_device;
} lld_orb_image;
typedef struct {                  /* per (image, level), optional */
  int32_t n_candidates;           /* FAST keypoints handed to DistributeOctTree  */
  int32_t cells_min_th;           /* cells that found nothing at ini_th_fast     */
  int32_t cells_empty;            /* cells that found nothing at min_th_fast too */
  int32_t iterations;             /* passes of the outer loop (`iteration`)      */
  int32_t sorted_rounds;          /* passes of the sorted-split loop (:673-738)  */
  int32_t finish_unchanged;       /* 1: the loop ended because the size did not change (not size >= N) */
  int32_t n_keypoints;            /* final node count = keypoints of the level   */
  int32_t features_wanted;        /* N = mnFeaturesPerLevel[level]               */
} lld_orb_level_stats;
typedef struct {
  int32_t  capacity;              /* in: entries the arrays hold (>= lld_orb_extractor_levels.max_keypoints)   */
  int32_t  n;                     /* out: keypoints, level by level, within a level in the final lNodes order   */
  float*   xy;                    /* [capacity][2] pt, scaled to level 0 by the float multiply of :1094-1101    */
  int32_t* octave;                /* [capacity]                                                                 */
  float*   angle;                 /* [capacity] degrees                                                         */
  float*   response;              /* [capacity]                                                                 */
  float*   size;                  /* [capacity] (float)(int)(PATCH_SIZE * mvScaleFactor[level])                 */
  uint32_t* desc;                 /* [capacity][8] rBRIEF, byte order of mDescriptors.data                      */
  lld_orb_level_stats* stats;     /* [n_levels] or NULL                                                         */
} lld_orb_features;
int  lld_orb_extractor_create(lld_ctx* ctx, const lld_orb_extractor_params* params, lld_orb_extractor** out);
void lld_orb_extractor_destroy(lld_orb_extractor* ex);
int  lld_orb_extractor_levels_get(const lld_orb_extractor* ex, lld_orb_extractor_levels* out);
/* Extracts n_images (1 <= n_images <= max_images) images in one sequence of launches on the context's stream; returns after the
 * results are on the host.  Invalid sizes, nulls, too many images or too small an output capacity return LLD_ERR_INVALID before
 * anything is queued.  A refused call leaves the handle as the last successful call left it: lld_orb_extractor_pyramids and
 * lld_orb_extractor_descriptors still describe that call's images, with its sizes and counts. */
int  lld_orb_extract(lld_orb_extractor* ex, int n_images, const lld_orb_image* images, lld_orb_features* outs);
/* The pyramid of image `image_index` of the last lld_orb_extract as device pointers: fills n_levels, cols, rows and steps and
 * sets on_device = 1.  `left` or `right` (whichever is non-NULL) receives the level pointers, `step` the matching step array, so
 * two calls (image 0 -> left, image 1 -> right) build the struct lld_compute_stereo_matches reads.  The arrays pointed to must
 * hold n_levels entries.  Valid until the next lld_orb_extract on the handle or lld_orb_extractor_destroy. */
int  lld_orb_extractor_pyramids(const lld_orb_extractor* ex, int image_index, const uint8_t** levels, int32_t* cols, int32_t* rows,
                                int32_t* step);
/* The rBRIEF descriptors of image `image_index` of the last lld_orb_extract as a device pointer: *desc = [n][8] u32 in HBM (the
 * byte order of mDescriptors.data), *n = that image's keypoint count.  Valid under the same rule as lld_orb_extractor_pyramids;
 * lld_bow_transform reads it with on_device = 1, so extract -> transform never leaves the device. */
int  lld_orb_extractor_descriptors(const lld_orb_extractor* ex, int image_index, const uint32_t** desc, int32_t* n);


/* ------------------------------------------------------------------ the stereo Frame, built on the device
 * Frame::Frame for a stereo pair (src/Frame.cc:77-170) runs, after the two ORBextractor calls (:101-106): UndistortKeyPoints (:111),
 * ComputeStereoMatches (:113), the level tables and grid constants (:92-98, :140-157) and AssignFeaturesToGrid (:159).  These calls do
 * that part on the device and hand back a resident lld_frame - the handle of lld_frame_create, on which lld_frame_search_last_frame,
 * lld_frame_search_local_points, lld_frame_set_lines, lld_frame_track_* and lld_frame_destroy work unchanged - whose mvuRight and
 * mvDepth were COMPUTED in HBM; the frame carries right coordinates, angles and mvInvLevelSigma2, so the whole chain may follow.
 *   stage 1  the row-band Hamming search of ComputeStereoMatches (:536-613): one wavefront per left keypoint, a lane per right
 *            keypoint; right keypoint iR is a candidate iff its octave is within +-1 of the left one, (int)vL lies in
 *            [floor(yR - r), ceil(yR + r)] with r = 2 * scale[octave_R], and uR lies in [uL - mbf/mb, uL]; a left keypoint with uL < 0
 *            is skipped; lowest distance, then lowest iR; accepted iff the distance is < (TH_HIGH + TH_LOW) / 2.  Bit-identical to
 *            the LLD_ORB_CAND_ROWS problem lld_compute_stereo_matches runs (which needs one workgroup and a trip through the host).
 *   stage 2, 3  the SAD refinement and the median cut of lld_compute_stereo_matches (same kernels), writing mvuRight / mvDepth into
 *            the frame's own arrays.
 * Scope: RECTIFIED stereo only - mvKeysUn = mvKeys, the `mDistCoef.at<float>(0)==0.0` branch of Frame::UndistortKeyPoints
 * (:468-474); the distorted branch, for the RGB-D and the monocular Frame, is lld_frame_build_mono* below (the reference rectifies a
 * stereo pair before it reaches the Frame).  Lines are added with
 * lld_frame_build_lines, which matches them on the device, or with lld_frame_set_lines when the caller has line_matches already (the
 * reference's line extractor is external and host-side: the KeyLines and descriptors themselves come from the host either way).
 * Both build calls queue their kernels on the context's stream and return WITHOUT synchronising; every later call on the frame is
 * ordered after them by that stream, and lld_frame_stereo_download is the one that waits.
 * Refusals, before anything is queued: LLD_ERR_INVALID for null pointers, mb not > 0, a grid outside lld_frame_create's limits,
 * n_levels outside [1, LLD_ORB_MAX_LEVELS] or different from pyr->n_levels, octaves outside [0, n_levels), an extractor without a
 * successful lld_orb_extract, image indices outside that call's n_images or equal to each other; LLD_ERR_UNSUPPORTED above
 * LLD_ORB_MAX_KEYPOINTS keypoints on either side.  A left image without keypoints gives an empty frame (nt = 0) and LLD_OK
 * (Frame.cc:108-109). */
typedef struct {
  float grid_min_x, grid_min_y, grid_width_inv, grid_height_inv;   /* mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv  */
  int32_t grid_cols, grid_rows;                                    /* 64, 48 (Frame.h:43-44); as lld_orb_search                       */
  float mb, mbf;                                                   /* mb = mbf / fx (Frame.cc:156), mbf: minZ = mb, maxD = mbf / mb   */
  const float* left_angle;      /* [left->n] mvKeysUn[k].angle, which searches with check_orientation read; required by
                                   lld_frame_build_stereo_keypoints (host or device like the keypoints); lld_frame_build_stereo reads
                                   the extractor's own                                                                               */
  const float* right_angle;     /* [right->n] or NULL; no routine reads mvKeysRight[k].angle, the frame does not keep it             */
  int32_t keypoints_on_device;  /* lld_frame_build_stereo_keypoints: 1 = xy, desc and the angles of both sides and right->octave are
                                   HBM pointers, read in place.  left->octave stays a HOST array on both routes: it becomes the
                                   frame's host copy of the octaves (query validation) and is the one array uploaded               */
  int32_t n_levels;             /* mnScaleLevels; must equal pyr->n_levels                                                           */
  const float* level_scale;       /* [n_levels] mvScaleFactors                                                                       */
  const float* level_sigma2;      /* [n_levels] mvLevelSigma2, or NULL (all 1)                                                       */
  const float* level_inv_sigma2;  /* [n_levels] mvInvLevelSigma2                                                                     */
} lld_frame_stereo_params;
/* The general form.  left / right: mvKeys / mvKeysRight with mDescriptors / mDescriptorsRight, on the host or (keypoints_on_device)
 * in HBM; pyr: the two image pyramids as for lld_compute_stereo_matches, on the host or (pyr->on_device) in HBM.  Everything that
 * starts on the host travels in ONE copy from a pinned buffer the frame owns; with device keypoints that copy is left->octave
 * (plus host pyramids).  Device inputs must stay valid until the queued work has run (e.g. until lld_frame_stereo_download). */
int  lld_frame_build_stereo_keypoints(lld_ctx* ctx, const lld_keypoints* left, const lld_keypoints* right, const lld_stereo_pyramids* pyr,
                                      const lld_frame_stereo_params* params, lld_frame** out);
/* The same build on images left_image / right_image of the handle's last lld_orb_extract, on the extractor's context: keypoints,
 * angles, descriptors and pyramids are read where the extractor left them, the level tables are the extractor's (params->n_levels,
 * level_*, left_angle, right_angle and keypoints_on_device are ignored), and nothing is uploaded.  The frame copies what it keeps
 * into its own allocation (device to device, inside the search kernel), so it survives the next lld_orb_extract on the handle and
 * the handle's destruction. */
int  lld_frame_build_stereo(lld_orb_extractor* ex, int left_image, int right_image, const lld_frame_stereo_params* params, lld_frame** out);
/* Waits for the frame's queued work and fetches mvuRight, mvDepth, optionally best_r / sad, and n_matches in one copy (the host
 * needs them for Frame::UnprojectStereo and for keyframe creation).  out->u_right and out->depth must hold the frame's nt entries.
 * LLD_ERR_INVALID on a frame made by lld_frame_create. */
int  lld_frame_stereo_download(lld_frame* frame, lld_stereo_result* out);


/* ------------------------------------------------------------------ the RGB-D and the monocular Frame, built on the device
 * The other two constructors of the reference: Frame::Frame(imGray, imDepth, ...) (src/Frame.cc:163-215) runs, after ExtractORB (:180),
 * UndistortKeyPoints (:187, :468-498) and ComputeStereoFromRGBD (:189, :707-728); Frame::Frame(imGray, ...) (:220-292) runs
 * UndistortKeyPoints (:248) and sets mvuRight = mvDepth = -1 (:255-256).  These calls do that on the device, in ONE launch with a lane
 * per keypoint (no atomics, no LDS), and hand back a resident lld_frame as lld_frame_build_stereo* does: its keypoints are mvKeysUn, it
 * carries mvuRight, angles and mvInvLevelSigma2, and lld_frame_search_*, lld_frame_compute_bow, lld_frame_set_lines and every
 * lld_frame_track_* call work on it unchanged (th_motion = 15 and th_local = 3 are the reference's thresholds for these sensors,
 * Tracking.cc:901, :1657).  The calls queue on the context's stream and return WITHOUT synchronising;
 * lld_frame_keypoints_download is the one that waits.
 *   undistortion  mvKeysUn[i].pt.  dist[0] == 0.0f: the distorted point, bit for bit, whatever the other coefficients hold (the
 *            reference's test, :470).  Otherwise the RESTATED cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) (:486) -
 *            OpenCV 3's cvUndistortPoints with R = I and P = K - in double, every operation rounded separately (no fused multiply-add):
 *              fx, fy, cx, cy, k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4] (0 when n_dist = 4) widened to double
 *              ifx = 1.0/fx; ify = 1.0/fy;  x0 = x = ((double)u - cx)*ifx;  y0 = y = ((double)v - cy)*ify
 *              5 times:  r2 = x*x + y*y;  icdist = 1.0/(1.0 + ((k3*r2 + k2)*r2 + k1)*r2)
 *                        dx = ((2.0*p1)*x)*y + p2*(r2 + (2.0*x)*x);  dy = p1*(r2 + (2.0*y)*y) + ((2.0*p2)*x)*y
 *                        x = (x0 - dx)*icdist;  y = (y0 - dy)*icdist
 *              u_un = (float)(fx*x + cx);  v_un = (float)(fy*y + cy)
 *            The five iterations are fixed, not run to convergence (up to 0.11 px is left at the corners of the TUM1 camera); that is
 *            the reference's behaviour.  Parity with OpenCV's own binary is unpinned, as everywhere in this project; every value is
 *            bit-exact against the numpy restatement tests/frame_mono_ref.py.  An undistorted keypoint may leave the grid; the searches
 *            drop such a keypoint as Frame::PosInGrid does (:446-456).
 *   depth    ComputeStereoFromRGBD: d = imDepth.at<float>(v, u) at the DISTORTED keypoint, row = (int)v, col = (int)u (truncation
 *            toward zero).  The reference indexes unchecked; here a keypoint whose u or v is not finite or lies outside (-1, cols) x
 *            (-1, rows) (compared in float, before the conversion) has no depth, so that no read leaves the image.  The depth image is
 *            the one GrabImageRGBD receives (Tracking.cc:252-253, imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor)) and only the
 *            sampled pixels are converted: LLD_DEPTH_U16 gives d = (float)raw * factor, always; LLD_DEPTH_F32 gives d = raw * factor
 *            when fabsf(factor - 1.0f) > 1e-5f and the raw value otherwise (one float multiply).  d > 0: mvDepth = d and
 *            mvuRight = u_un - mbf/d (a float division, then a float subtraction); +inf passes (depth inf, mvuRight = u_un); zero,
 *            negative and NaN leave both at -1.  factor is mDepthMapFactor as Tracking holds it, i.e. 1/DepthMapFactor of the
 *            settings file (Tracking.cc:155-159).
 *   no depth image (NULL): the monocular frame, mvuRight = mvDepth = -1 for every keypoint.
 * Refusals, before anything is allocated or queued: LLD_ERR_INVALID for null pointers, fx or fy not > 0, cx or cy not finite, n_dist
 * outside {4, 5}, a non-finite coefficient or mbf, a grid outside lld_frame_create's limits, n_levels outside [1, LLD_ORB_MAX_LEVELS], a host
 * octave outside [0, n_levels), a depth image with cols or rows outside [1, 16383], a step below the row's bytes or not a multiple of
 * the element size, an unknown type or a non-finite factor, an extractor without a successful lld_orb_extract, an image index outside
 * that call's n_images; LLD_ERR_UNSUPPORTED above LLD_ORB_MAX_KEYPOINTS.  No keypoints give an empty frame and LLD_OK (:184-185). */
#define LLD_DEPTH_F32 0        /* CV_32F  */
#define LLD_DEPTH_U16 1        /* CV_16U  */
typedef struct {
  float grid_min_x, grid_min_y, grid_width_inv, grid_height_inv;   /* mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv:
                                                                      from lld_frame_image_bounds (Frame.cc:197-200)                */
  int32_t grid_cols, grid_rows;                                    /* 64, 48 (Frame.h:43-44); as lld_orb_search                       */
  float fx, fy, cx, cy;                                            /* mK                                                              */
  float dist[5];                                                   /* mDistCoef: k1, k2, p1, p2, k3; dist[4] is ignored when n_dist = 4 */
  int32_t n_dist;                                                  /* 4 or 5 (mDistCoef.rows, Tracking.cc:85-87)                      */
  float mbf;                                                       /* mvuRight = u_un - mbf / depth                                   */
  int32_t keypoints_on_device;  /* lld_frame_build_mono_keypoints: 1 = kp->xy, kp->desc and left_angle are HBM pointers, read in place.
                                   kp->octave stays a HOST array (the frame's host copy of the octaves, and the one array uploaded)    */
  int32_t n_levels;             /* mnScaleLevels                                                                                       */
  int32_t reserved;
  const float* left_angle;      /* [kp->n] mvKeysUn[k].angle; required by lld_frame_build_mono_keypoints (host or device like the
                                   keypoints); lld_frame_build_mono reads the extractor's own                                          */
  const float* level_scale;       /* [n_levels] mvScaleFactors                                                                       */
  const float* level_sigma2;      /* [n_levels] mvLevelSigma2, or NULL (all 1)                                                       */
  const float* level_inv_sigma2;  /* [n_levels] mvInvLevelSigma2                                                                     */
} lld_frame_mono_params;
typedef struct {
  const void* data;             /* imDepth.data as the caller holds it BEFORE convertTo: float or uint16_t pixels                      */
  int32_t cols, rows;
  int32_t step;                 /* bytes per image row (cv::Mat::step)                                                                 */
  int32_t type;                 /* LLD_DEPTH_F32 or LLD_DEPTH_U16                                                                      */
  float   factor;               /* mDepthMapFactor                                                                                     */
  int32_t on_device;            /* 1: data is an HBM pointer, read in place; it must stay valid until the queued work has run          */
} lld_depth_image;
/* The general form.  kp: mvKeys with mDescriptors, on the host or (keypoints_on_device) in HBM; depth_or_null: the depth image on the
 * host or (on_device) in HBM, or NULL for a monocular frame.  Everything that starts on the host, the depth image included (rows
 * packed), travels in ONE copy from a pinned buffer the frame owns. */
int  lld_frame_build_mono_keypoints(lld_ctx* ctx, const lld_keypoints* kp, const lld_depth_image* depth_or_null,
                                    const lld_frame_mono_params* params, lld_frame** out);
/* The same build on image `image` of the handle's last lld_orb_extract, on the extractor's context: keypoints, angles, descriptors and
 * level tables are read where the extractor left them (params->n_levels, level_*, left_angle and keypoints_on_device are ignored);
 * only a host depth image is uploaded.  The frame copies what it keeps into its own allocation inside the kernel, so it survives the
 * next lld_orb_extract on the handle and the handle's destruction. */
int  lld_frame_build_mono(lld_orb_extractor* ex, int image, const lld_depth_image* depth_or_null, const lld_frame_mono_params* params,
                          lld_frame** out);
/* Waits for the frame's queued work and fetches mvKeysUn[i].pt (xy_un [nt][2]), mvuRight and mvDepth ([nt] each) in one copy; any of
 * the three may be NULL.  The host needs them for Frame::UnprojectStereo, the Initializer and keyframe creation.  LLD_ERR_INVALID on a
 * frame made by lld_frame_create or lld_frame_build_stereo* (and lld_frame_stereo_download stays LLD_ERR_INVALID on a frame made here). */
int  lld_frame_keypoints_download(lld_frame* frame, float* xy_un, float* u_right, float* depth);
/* Frame::ComputeImageBounds (Frame.cc:500-528), host only: bounds = mnMinX, mnMaxX, mnMinY, mnMaxY.  dist[0] == 0.0f gives 0, cols, 0,
 * rows; otherwise the undistortion above of the corners (0,0), (cols,0), (0,rows), (cols,rows) and the reference's min / max of them.
 * LLD_ERR_INVALID as the build calls refuse the camera, or cols / rows not > 0. */
int  lld_frame_image_bounds(int32_t cols, int32_t rows, float fx, float fy, float cx, float cy, const float* dist, int32_t n_dist,
                            float bounds[4]);


/* ------------------------------------------------------------------ DBoW2 vocabulary: load, transform, L1 score
 * Thirdparty/DBoW2/DBoW2/ of the reference, as ORB-SLAM2 uses it (ORBVocabulary = TemplatedVocabulary<FORB::TDescriptor, FORB>).
 * Every value is bit-exact against the CPU restatement tests/bow_ref.py.  Restated rules:
 *   Loader (TemplatedVocabulary.h:1338-1424, loadFromTextFile): line 1 is `k L scoring weighting`, refused unless 0 <= k <= 20,
 *     1 <= L <= 10, 0 <= scoring <= 5, 0 <= weighting <= 3 (:1358).  Every following line is one node `parent isLeaf d0 .. d31
 *     weight` and its node id is its line index (root = node 0, :1375-1381); the children of a node are its child lines in file
 *     order (:1384); word ids number the lines with isLeaf > 0 in file order (:1402-1409); a descriptor byte is (unsigned char)
 *     of the decimal int (FORB.cpp:120-135); weight is a double.  isLeaf() of a node means "has no children" (:328).
 *   Descent (:1218-1256): from the root, each level's children in order, distance = FORB::distance (FORB.cpp:81-101, the 256-bit
 *     Hamming distance), strict `<` (on equal distances the first child in order wins); the node reached at level m_L - levelsup
 *     is nid (m_L - levelsup <= 0: the root, :1227); the descent stops at the first node without children and returns its
 *     word_id and weight.
 *   Transform (:1127-1194, levelsup = 4 at every call site of ORB-SLAM2): features in index order; weight w > 0 goes into both
 *     vectors, anything else is a stop word and goes into neither.  TF / TF_IDF: BowVector::addWeight (BowVector.cpp:34-46), the
 *     repeated hits of a word add w again and again in feature order (repeated addition, not count*w); IDF / BINARY:
 *     addIfNotExist (:50-58).  FeatureVector::addFeature (FeatureVector.cpp:31-45): nodes ascending, feature indices ascending
 *     within a node.  Then normalize (BowVector.cpp:62-84), L1: norm = sequential sum of fabs(v) in ascending word id, then
 *     v /= norm for every word if norm > 0.  L1 scoring always normalises (ScoringObject.h:74), so the `/= nd` branch never runs.
 *   Score (ScoringObject.cpp:23-66, L1Scoring::score(v1 = query, v2 = candidate)): the common words in ascending id,
 *     score += fabs(vi - wi) - fabs(vi) - fabs(wi) left to right, then score = -score/2.0 (no common word: -0.0).
 * DEVIATIONS (the reference is undefined here):
 *   - nid is declared uninitialised per feature (:1151, :1179): a descent that reaches a leaf above level m_L - levelsup adds the
 *     feature under an indeterminate node.  Here it goes under the leaf's own node id.
 *   - A file ending in a newline makes the reference's `while(!f.eof())` parse one more, empty line: a childless non-word child of
 *     the root with weight 0 and a descriptor FORB::fromString leaves uninitialised (features that land on it are dropped).  This
 *     loader skips blank lines (whitespace only) and adds no such node.
 * Limits: lld_bow_vocab_create refuses (LLD_ERR_INVALID, nothing allocated) a tree where node 0 is not the root or parent[i] >= i,
 * a leaf flag that disagrees with "has no children", a node with more than LLD_BOW_MAX_CHILDREN children, a leaf deeper than
 * LLD_BOW_MAX_DEPTH, fewer than 2 nodes, or weighting outside 0..3; scoring other than L1_NORM returns LLD_ERR_UNSUPPORTED.
 * A vocabulary handle is driven by one host thread at a time (it runs on its context's stream). */
#define LLD_BOW_MAX_FEATURES 8192        /* descriptors per set of one lld_bow_transform call */
#define LLD_BOW_MAX_CHILDREN 64
#define LLD_BOW_MAX_DEPTH 16
#define LLD_BOW_L1_NORM 0                /* DBoW2::ScoringType: L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT */
#define LLD_BOW_TF_IDF 0                 /* DBoW2::WeightingType: TF_IDF, TF, IDF, BINARY */
#define LLD_BOW_TF 1
#define LLD_BOW_IDF 2
#define LLD_BOW_BINARY 3
typedef struct lld_bow_vocab lld_bow_vocab;
typedef struct {
  int32_t k, L, scoring, weighting;      /* the header line                                     */
  int32_t n_nodes;                       /* root included                                       */
  int32_t n_words;                       /* lines with isLeaf > 0                               */
  int32_t* parent;                       /* [n_nodes]; parent[0] = -1 (the root has no line)    */
  uint8_t* is_leaf;                      /* [n_nodes] the file flag (> 0 -> 1); is_leaf[0] = 0  */
  uint32_t* desc;                        /* [n_nodes][8] u32, byte order of the text; root zero */
  double* weight;                        /* [n_nodes]; weight[0] = 0                            */
} lld_bow_vocab_desc;
typedef struct {
  int32_t k, L, scoring, weighting, n_nodes, n_words;
  int32_t min_leaf_depth;                /* shallowest word (root = depth 0)                    */
  int32_t max_depth;
  int32_t max_sets, max_features;        /* as created                                          */
} lld_bow_vocab_info;
typedef struct {
  const uint32_t* desc;                  /* [n][8] u32: host or (on_device = 1) HBM             */
  int32_t n;                             /* 0 <= n <= the vocabulary's max_features             */
  int32_t on_device;
  int32_t levelsup;                      /* 4 at every ORB-SLAM2 call site                      */
  int32_t reserved;
} lld_bow_set;
typedef struct {                         /* every array holds the set's n entries (node_start n + 1) */
  int32_t n_words;                       /* out: BowVector size                                  */
  int32_t* word;                         /* [n] ascending word ids                               */
  double* value;                         /* [n] L1-normalised values                             */
  int32_t n_nodes;                       /* out: FeatureVector size                              */
  int32_t* node;                         /* [n] ascending node ids                               */
  int32_t* node_start;                   /* [n + 1] CSR over `feature`                           */
  int32_t* feature;                      /* [n] feature indices, ascending within a node         */
  int32_t* feature_word;                 /* [n] or NULL: word id per feature, -1 = stop word     */
  int32_t* feature_nid;                  /* [n] or NULL: nid per feature (also for stop words)   */
} lld_bow_result;
typedef struct {
  int32_t n;                             /* words                                                */
  const int32_t* word;                   /* [n] strictly ascending, each in [0, n_words)         */
  const double* value;                   /* [n]                                                  */
} lld_bow_vector;
/* Host only (no context, no GPU): reads a DBoW2 text vocabulary in two calls.  With d->parent == NULL it fills k, L, scoring,
 * weighting, n_nodes and n_words; with all four arrays set (n_nodes entries each) it fills them.  Returns LLD_ERR_INVALID for a
 * missing file, a refused header, a malformed node line or a parent that is not an earlier node. */
int  lld_bow_vocab_read_text(const char* path, lld_bow_vocab_desc* d);
/* Validates the tree (see Limits) before anything is allocated, then uploads it into one device slab sized for max_sets sets of
 * up to max_features (1 <= max_features <= LLD_BOW_MAX_FEATURES) descriptors. */
int  lld_bow_vocab_create(lld_ctx* ctx, const lld_bow_vocab_desc* d, int max_sets, int max_features, lld_bow_vocab** out);
void lld_bow_vocab_destroy(lld_bow_vocab* v);
int  lld_bow_vocab_info_get(const lld_bow_vocab* v, lld_bow_vocab_info* out);
/* TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup) for n_sets (1..max_sets) sets in one sequence of
 * launches; returns with the results on the host.  Nulls, n outside 0..max_features or too many sets return LLD_ERR_INVALID
 * before anything is queued. */
int  lld_bow_transform(lld_bow_vocab* v, int n_sets, const lld_bow_set* sets, lld_bow_result* results);
/* Frame::ComputeBoW (src/Frame.cc) on a resident frame: the descent and the assembly of lld_bow_transform on the frame's own device
 * descriptors (no upload), after which the FeatureVector (node, node_start, feature and their counts) is copied device to device, on the
 * stream, into memory the frame owns: it survives every later lld_bow_transform / lld_frame_compute_bow on the vocabulary and is what
 * lld_frame_track_reference_keyframe matches against.  out_or_null != NULL: waits and returns BowVector and FeatureVector on the host
 * (arrays of nt entries, node_start nt + 1, as for lld_bow_transform; bit-identical to it on the same descriptors) - a frame that becomes a
 * keyframe needs them for lld_kfdb_add.  NULL: queues the work and returns without synchronising (the frame's first call allocates).
 * A frame without keypoints gives empty vectors and LLD_OK.  Works on frames of lld_frame_create and of lld_frame_build_stereo*.
 * LLD_ERR_INVALID before anything is queued: a NULL frame or vocabulary, a vocabulary of another context than the frame's, more keypoints
 * than the vocabulary's max_features, or out arrays missing as for lld_bow_transform. */
int  lld_frame_compute_bow(lld_frame* frame, lld_bow_vocab* voc, int levelsup, lld_bow_result* out_or_null);
/* L1Scoring::score(query, candidate c) for n_cand candidates given as CSR: candidate c holds the words
 * cand_word[cand_start[c] .. cand_start[c+1]) (strictly ascending, each in [0, n_words)) with cand_value.  One upload, one
 * launch, out[c] on return.  Malformed vectors return LLD_ERR_INVALID before anything is queued.  Staging uses the context's
 * grow-only device scratch. */
int  lld_bow_score(lld_bow_vocab* v, const lld_bow_vector* query, int n_cand, const int32_t* cand_start, const int32_t* cand_word,
                   const double* cand_value, double* out);

/* ------------------------------------------------------------------ KeyFrameDatabase: resident inverted file, loop and reloc candidates
 * src/KeyFrameDatabase.cc of the reference (ORB-SLAM2's), with the per-keyframe query registers of KeyFrame (mnLoopQuery,
 * mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore, include/KeyFrame.h) and the covisibility lists the queries read.
 * Keyframes are the caller's mnId.  Ids, counters and candidates are bit-exact against the CPU restatement tests/kfdb_ref.py.
 * Restated rules:
 *   add (:40-45) appends the keyframe to the list of every word of its BowVector.  erase (:47-67) removes the first occurrence
 *     from each of those lists: the other entries keep their order.  clear (:69-73) empties the lists and leaves every register
 *     of every keyframe as it is.
 *   Walk (:86-104 loop, :207-222 reloc): the query's words in ascending order, each word's list in list order.  Per encounter of a
 *     keyframe: if its stamp (mnLoopQuery / mnRelocQuery) != the query id, words = 0 and (loop path: unless the keyframe is in the
 *     connected set) it is stamped with the query id and appended to lKFsSharingWords; then words++.  Stamps start at 0
 *     (KeyFrame.cc:38) and the loop and reloc registers are separate, so a keyframe whose stamp already equals the query id (query
 *     id 0 on a fresh keyframe, a query id used again) is neither reset nor listed; a connected keyframe is never stamped, so its
 *     words are reset at every encounter (it ends at 1).
 *     List order = ascending (first query word the keyframe shares, add order): erase never reorders a list and the database
 *     never holds a keyframe twice.
 *   Thresholds (:111-138, :226-252): maxCommonWords = the largest words of the listed keyframes; minCommonWords =
 *     (int)(maxCommonWords * 0.8f), a float product truncated.  A listed keyframe with words > minCommonWords (strict) is scored
 *     (nscores++): si = (float)L1Scoring::score(query, keyframe), the double sum of lld_bow_score cast to float, stored in
 *     mLoopScore / mRelocScore.  lScoreAndMatch holds the scored ones in list order; the loop path only those with si >= minScore.
 *   Accumulation (:144-173, :258-287): per entry, over GetBestCovisibilityKeyFrames(10) (the first <= 10 of the ordered
 *     covisibles), in order: accScore starts at si, float, summed left to right; bestScore starts at si and pBestKF at the entry,
 *     replaced only on a strictly greater score (the first maximum wins).  A neighbour is admitted on the loop path when
 *     mnLoopQuery == id && mnLoopWords > minCommonWords; on the reloc path when mnRelocQuery == id, with no words test, so a
 *     neighbour listed but not scored in this query adds the mRelocScore of an earlier query.
 *   Retain (:175-196, :289-308): bestAccScore = the largest accScore, starting at minScore (loop) or 0 (reloc); an entry is kept
 *     when accScore > 0.75f*bestAccScore (strict, float); the output is its pBestKF, de-duplicated with the first occurrence kept,
 *     in list order.  An empty lKFsSharingWords or lScoreAndMatch returns nothing (the registers the walk and the scoring changed
 *     stay changed).
 * DEVIATION (the reference is undefined here): mRelocScore is never initialised by the reference, and the reloc path reads it
 *   for a keyframe it did not score.  Here every score register starts at 0.0f when the library first meets the keyframe; from
 *   then on it persists across queries exactly like the reference field.
 * Handles and limits: any id that is added or named by lld_kfdb_set_covisibles gets a slot with its own registers; slots are never
 * released (ORB-SLAM2 never frees a keyframe) and max_keyframes (<= LLD_KFDB_MAX_KEYFRAMES) bounds them.  max_words bounds the words
 * of the BowVectors in the database at one time; erase returns its space (an add that does not fit behind the last vector compacts
 * the pool).  These return LLD_ERR_INVALID before anything is queued and leave the database unchanged: nulls; query or keyframe
 * words not strictly ascending or outside [0, n_words); adding an id that is in the database (or twice in one call); more slots
 * than max_keyframes or more words than max_words.  Erasing an id that is not in the database does nothing and returns LLD_OK.
 * A query always runs to completion and updates the registers, even when capacity is smaller than the result.  A handle is driven
 * by one host thread at a time, on its vocabulary's context stream. */
#define LLD_KFDB_MAX_KEYFRAMES 8192      /* slots of one database                                */
#define LLD_KFDB_MAX_COVISIBLES 10       /* GetBestCovisibilityKeyFrames(10)                     */
typedef struct lld_kfdb lld_kfdb;
typedef struct {
  int32_t capacity;                      /* entries of kf_id / acc_score                          */
  int32_t n_candidates;                  /* out: the full count; at most capacity ids are written */
  uint64_t* kf_id;                       /* out: the reference's return order                    */
  float* acc_score;                      /* out or NULL: accScore of the entry that produced each */
  int32_t n_sharing;                     /* out: lKFsSharingWords.size()                          */
  int32_t max_common_words;              /* out: maxCommonWords (0 when nothing is listed)        */
  int32_t min_common_words;              /* out: minCommonWords                                   */
  int32_t n_scored;                      /* out: nscores                                          */
} lld_kfdb_result;
/* KeyFrameDatabase(voc): an empty database on the vocabulary's context, for word ids in [0, voc's n_words). */
int  lld_kfdb_create(lld_bow_vocab* voc, int32_t max_keyframes, int64_t max_words, lld_kfdb** out);
void lld_kfdb_destroy(lld_kfdb* db);
/* n add() calls, in order: keyframe kf_id[i] with BowVector vecs[i]. */
int  lld_kfdb_add(lld_kfdb* db, int32_t n, const uint64_t* kf_id, const lld_bow_vector* vecs);
/* n erase() calls (KeyFrame::SetBadFlag, src/KeyFrame.cc:567). */
int  lld_kfdb_erase(lld_kfdb* db, int32_t n, const uint64_t* kf_id);
int  lld_kfdb_clear(lld_kfdb* db);
/* KeyFrame::UpdateBestCovisibles for n keyframes: the ordered covisibles of kf_id[i] are neighbour[start[i] .. start[i+1]) (start
 * holds n + 1 entries); the first LLD_KFDB_MAX_COVISIBLES are kept.  Neighbours not yet in the database get a slot and count once
 * they are added. */
int  lld_kfdb_set_covisibles(lld_kfdb* db, int32_t n, const uint64_t* kf_id, const int32_t* start, const uint64_t* neighbour);
/* DetectLoopCandidates(pKF, minScore) with pKF->mnId = query_id, pKF->mBowVec = q, GetConnectedKeyFrames() = connected (ids the
 * database has never met are ignored).  Uploads the query, downloads the candidates. */
int  lld_kfdb_detect_loop_candidates(lld_kfdb* db, uint64_t query_id, const lld_bow_vector* q, int32_t n_connected,
                                     const uint64_t* connected, float min_score, lld_kfdb_result* out);
/* DetectRelocalizationCandidates(F) with F->mnId = query_id, F->mBowVec = q. */
int  lld_kfdb_detect_relocalization_candidates(lld_kfdb* db, uint64_t query_id, const lld_bow_vector* q, lld_kfdb_result* out);

/* ================================================================== PnPsolver (src/PnPsolver.cc), Tracking::Relocalization's RANSAC
 * A batch of independent PnPsolvers, one per relocalisation candidate, whose RANSAC state stays in HBM between iterate() calls.
 * The interface is the reference's: the constructor (lld_pnp_problem), SetRansacParameters (lld_pnp_params), iterate(n, bNoMore,
 * vbInliers, nInliers) (lld_pnp_batch_iterate + _download) and find() (lld_pnp_batch_find).  Restated literally:
 *   PnPsolver(F, vpMapPointMatches) (:66-110): the caller skips NULL and isBad() points; correspondence i carries GetWorldPos()
 *     (float xyz), mvKeysUn[kp].pt (float uv), mvLevelSigma2[octave] (float sigma2) and kp = mvKeyPointIndices[i]; fu, fv, uc, vc
 *     = F.fx, fy, cx, cy.  adapters/lld_pnp_adapter.cc does this on live objects.
 *   SetRansacParameters (:121-157), computed on the host by lld_pnp_batch_create: nMinInliers = N*epsilon (a float product,
 *     truncated), raised to minInliers and to minSet; epsilon raised to (float)nMinInliers/N; nIterations = 1 when nMinInliers == N,
 *     else ceil(log(1-p)/log(1-pow(epsilon,3))) (the exponent is 3, not minSet); mRansacMaxIts = max(1, min(nIterations,
 *     maxIterations)); mvMaxError[i] = sigma2[i]*th2 in float.  Relocalization's values (Tracking.cc:1882) are the defaults.
 *   iterate (:165-258): outputs reset; N < mRansacMinInliers -> bNoMore, no draws, no pose.  The loop runs while mnIterations <
 *     mRansacMaxIts || nCurrentIterations < n (a call after the budget is spent still runs n iterations).  Each iteration draws
 *     4 indices (RandomInt over the remaining vAvailableIndices, the back swapped into the taken place), runs EPnP and
 *     CheckInliers; a hypothesis with mnInliersi >= mRansacMinInliers is eligible; an eligible one with a strictly greater count
 *     than mnBestInliers becomes the best (mBestTcw = R|t converted to float); every eligible one calls Refine on the best set,
 *     and a Refine that succeeds returns the refined pose at once.  When the budget is spent: bNoMore, and the best hypothesis
 *     (not refined) when mnBestInliers >= mRansacMinInliers.  vbInliers has n_keypoints entries, set at mvKeyPointIndices.
 *   Refine (:260-306): EPnP on every best inlier in ascending index order, CheckInliers; success only when the count is strictly
 *     greater than mRansacMinInliers.  A best set of exactly 4 (min_inliers <= 4 with N <= 9) takes the minimal-set basis below.
 *   CheckInliers (:308-340): Xc, Yc, invZc float, ue / ve double, distX, distY, error2 float; inlier when error2 < mvMaxError[i].
 *     The kernels are compiled without FMA contraction, so every in/out decision is the reference's expression.
 *   EPnP compute_pose (:477-525) in fp64: PCA control points (:375-409), barycentric coordinates (:411-434), M, L_6x10 and rho,
 *     the three beta approximations (:667-758) each with 5 Gauss-Newton steps through the reference's own Householder qr_solve
 *     (:840-952; where it returns early without writing X, X keeps its previous value, 0 at the start), compute_R_and_t with
 *     solve_for_sign on the first point's z only (:636-665), estimate_R_and_t with its determinant flip of R's third row
 *     (:569-627), and the lowest reprojection error with ties going to the lower index (:518-520).
 * DEVIATION 1 (the sample stream): DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) draws from the
 *   process-global rand(), which the stereo path never seeds and the LoopClosing thread shares.  Here every solver has its own
 *   stream: glibc's rand() after srand(seed) (the TYPE_3 additive generator: r[i] = r[i-3] + r[i-31] mod 2^32, output r >> 1,
 *   310 warm-up values discarded; seed 0 acts as 1), turned into indices by RandomInt's int(rand()/(RAND_MAX+1.0)*d).  With one
 *   stream each the solvers are independent, so one batched round (iterate(5) on every live candidate) gives exactly what the
 *   reference's sequential round robin (Tracking.cc:1894-1987) gives for every candidate it reaches.
 * DEVIATION 2 (numerics left to OpenCV): with 4 correspondences M^T M has an exactly 4-dimensional null space and the basis
 *   cvSVD returns (:491) is an artefact of its Jacobi sweeps, which the beta approximations (and so the result) depend on.  For a
 *   minimal set the basis is columns 9..12 of Q of a Householder QR of M^T (12 x 8), as ut rows 11, 10, 9, 8.  Refine (N > 4)
 *   takes the eigenvectors of the 4 smallest |eigenvalues| of M^T M from a cyclic Jacobi (at most 40 sweeps, stopping when the
 *   squared off-diagonal sum is <= 1e-36 of the squared diagonal sum); the 3x3 PCA uses the same routine, and the SVD of ABt is
 *   V from the Jacobi of ABt^T ABt with u_k = ABt v_k / s_k (a cut third column completed as u0 x u1).  Every eigenvector's sign
 *   is canonical (its first largest-magnitude component positive).  cvInvert(CV_SVD) and cvSolve(CV_SVD) become (A^T A)^+ A^T
 *   with eigenvalues of A^T A at or below 1e-14 of the largest dropped (singular values below about 1e-7 of the largest); this
 *   cutoff is this library's choice, not OpenCV's.  Non-finite values follow IEEE with no special case (a NaN pose has 0 inliers).
 * Limits: LLD_ERR_INVALID / LLD_ERR_UNSUPPORTED with nothing allocated: nulls; n < 1 or more than LLD_PNP_MAX_SOLVERS solvers;
 *   more than LLD_PNP_MAX_CORRESPONDENCES correspondences or LLD_PNP_MAX_KEYPOINTS keypoints; a kp_index out of range or repeated;
 *   fx or fy not > 0; min_set other than 4 (UNSUPPORTED); max_iterations outside 1..LLD_PNP_MAX_ITERATIONS, probability outside
 *   (0, 1), epsilon outside (0, 1], th2 not > 0.  lld_pnp_batch_iterate: n_iterations < 1 (INVALID) or above
 *   LLD_PNP_MAX_ITERATIONS (UNSUPPORTED).  A handle is driven by one host thread at a time, on its context's stream. */
#define LLD_PNP_MAX_CORRESPONDENCES 8192  /* per solver                                        */
#define LLD_PNP_MAX_KEYPOINTS 8192        /* per frame (length of vbInliers)                   */
#define LLD_PNP_MAX_SOLVERS 256           /* per batch                                         */
#define LLD_PNP_MAX_ITERATIONS 65536      /* mRansacMaxIts and iterate()'s n                   */
typedef struct {
  double probability;                    /* 0.99                                                  */
  int32_t min_inliers;                   /* 10                                                    */
  int32_t max_iterations;                /* 300                                                   */
  int32_t min_set;                       /* 4 (the only one supported)                            */
  float epsilon;                         /* 0.5                                                   */
  float th2;                             /* 5.991                                                 */
} lld_pnp_params;
void lld_pnp_params_default(lld_pnp_params* p);    /* SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) (Tracking.cc:1882) */
typedef struct {
  int32_t n;                             /* correspondences                                       */
  const float* xyz;                      /* [3n] GetWorldPos()                                    */
  const float* uv;                       /* [2n] mvKeysUn[kp].pt                                  */
  const float* sigma2;                   /* [n]  mvLevelSigma2[octave]                            */
  const int32_t* kp_index;               /* [n]  mvKeyPointIndices: distinct, in [0, n_keypoints) */
  int32_t n_keypoints;                   /* vpMapPointMatches.size()                              */
  float fx, fy, cx, cy;
  uint32_t seed;                         /* srand(seed) of this solver's stream (DEVIATION 1)     */
} lld_pnp_problem;
typedef struct {
  float Tcw[12];                         /* 3x4 row-major [R | t], float as the reference's cv::Mat */
  int32_t has_pose;                      /* iterate() returned a non-empty Mat                    */
  int32_t n_inliers;                     /* nInliers                                              */
  int32_t no_more;                       /* bNoMore                                               */
  int32_t iterations;                    /* mnIterations                                          */
  int32_t best_inliers;                  /* mnBestInliers                                         */
  int32_t n_keypoints;                   /* out: entries written to inlier                        */
  uint8_t* inlier;                       /* [n_keypoints] vbInliers, caller-allocated, or NULL    */
} lld_pnp_result;
typedef struct {                          /* diagnostic: one hypothesis of the last iterate call   */
  int32_t n_inliers;                     /* mnInliersi                                            */
  int32_t record;                        /* 1: a new best                                         */
  int32_t refine;                        /* -1 not eligible; else the Refine of its best-so-far set: 0 failed, 1 succeeded */
  int32_t refined_inliers;               /* that Refine's count                                   */
  double R[9], t[3];                     /* mRi, mti                                              */
} lld_pnp_hypothesis;
typedef struct lld_pnp_batch lld_pnp_batch;
/* n PnPsolvers with SetRansacParameters(params): uploads one slab of all correspondences and the RANSAC constants. */
int  lld_pnp_batch_create(lld_ctx* ctx, int32_t n, const lld_pnp_problem* problems, const lld_pnp_params* params, lld_pnp_batch** out);
/* iterate(n_iterations) on every solver with active[s] != 0 (active NULL: all), on the device, with no host trip between the
 * kernels; queued on the context's stream.  Inactive solvers keep their state and last results. */
int  lld_pnp_batch_iterate(lld_pnp_batch* b, int32_t n_iterations, const uint8_t* active);
/* find() (:159-163) on every active solver: iterate(mRansacMaxIts) of each, continuing its state like the reference's find(). */
int  lld_pnp_batch_find(lld_pnp_batch* b, const uint8_t* active);
/* The last iterate's outputs of every solver (outs[n]); waits for the stream. */
int  lld_pnp_batch_download(lld_pnp_batch* b, lld_pnp_result* outs);
/* Diagnostic (tests): the hypotheses drawn by the last iterate call of `solver`.  n_window: hypotheses evaluated (the window
 * max(n, budget - mnIterations), speculative ones past a successful Refine included); n_run: the iterations iterate() made.
 * The first min(capacity, n_window) are written.  An inactive solver reports 0 / 0. */
int  lld_pnp_batch_hypotheses(lld_pnp_batch* b, int32_t solver, int32_t capacity, lld_pnp_hypothesis* out, int32_t* n_window,
                              int32_t* n_run);
void lld_pnp_batch_destroy(lld_pnp_batch* b);
/* find() (:159-163) on one freshly constructed solver: create, lld_pnp_batch_find, download, destroy. */
int  lld_pnp_find(lld_ctx* ctx, const lld_pnp_problem* problem, const lld_pnp_params* params, lld_pnp_result* out);

/* ------------------------------------------------------------------ Tracking::Relocalization as a stage of the frame chain
 * Stage 1 by Tracking::Relocalization (src/Tracking.cc:1837-1998), the fourth entry into the chain of lld_frame_track_* (declared here
 * because it takes lld_pnp_params): ONE call for ORBmatcher(0.75, true).SearchByBoW against every candidate (:1873), the PnPsolvers
 * (:1881-1883), the rounds of iterate(5) (:1894-1915) and, for every candidate a round gives a pose, the ladder PoseOptimization ->
 * discard -> SearchByProjection(F, pKF, sFound, 10, 100) -> PoseOptimization -> SearchByProjection(.., 3, 64) -> PoseOptimization -> discard
 * (:1917-1976).  One upload of the candidates; the K match counts come back once (the host applies `nmatches < 15` and isBad and computes
 * SetRansacParameters, whose log / ceil stay the host's fp64 expression); after that the host reads ONE status word per round and nothing
 * else until `out` is fetched.
 *   - SearchByBoW runs for all candidates in one launch: one wavefront per (candidate, keyframe node), the rotation histogram per candidate,
 *     into a per-candidate match table instead of the frame's own (vvpMapPointMatches[i]).
 *   - The PnPsolver constructor (:66-110) is a kernel: a candidate's matches in ascending keypoint order, xyz = the candidate's world
 *     positions, uv / sigma2 from the resident keypoints and the frame's level table.
 *   - Each solver owns its rand() stream (DEVIATION 1 above) and a candidate's ladder touches only its own copy of the frame's
 *     mvpMapPoints / mvbOutlier / mTcw, so the reference's sequential round robin equals: evaluate every live candidate of a round side by
 *     side, then take the first in candidate order whose ladder ends with nGood >= 50.  The ladder's rungs are predicated on device flags.
 *   - sFound is a set of MapPoint ids: a candidate's MapPoint is skipped by the projected search when its id is among the ids the
 *     candidate's copy of the frame holds (at :1930 the inliers, at :1958-1961 everything held).
 * On success (out->matched = 1) the frame is left as the other stage-1 entries leave it - the pose (mTcw of the winning attempt), the
 * MapPoints it holds with ids / world positions / Observations() > 0, mvbOutlier of those, no lines, nothing marked seen (Relocalization
 * sets no mnLastFrameSeen) - so lld_frame_track_local_map can follow with no lld_frame_track_set_state.  The reference's quirk is kept:
 * when the second PoseOptimization lifts nGood to >= 50, the points it flagged stay in mvpMapPoints with mvbOutlier set (:1952-1956
 * discard nothing).  lld_frame_track_download's stage-1 record then carries that state: pose_qt and chi2 of the winner's last
 * PoseOptimization, n_inliers = nGood, kp_point_id / kp_outlier, n_points / n_points_map of what the frame holds, n_search_first =
 * n_search = the winner's SearchByBoW count, zeros elsewhere (on failure: all zeros, every id -1).
 * DEVIATIONS: (a) on failure (matched = 0) the frame holds nothing and keeps the pose handed in; the reference leaves the residue of the
 * last attempt in a frame nobody reads.  (b) mvbOutlier of a keypoint WITHOUT a MapPoint reads 0; the reference keeps there the flag of
 * whichever earlier attempt last held a point on it, which nothing reads before PoseOptimization resets it.  (c) the candidates after the
 * winner are iterated speculatively in the winning round; their records report the state before that round, as the reference leaves them.
 * `view` / `pose_qt`: the image bounds, scale constants and intrinsics of the frame as for lld_frame_track_motion_model, and the pose the
 * frame keeps when nothing matches.  candidates[i] = vpCandidateKFs[i] as lld_ref_keyframe describes a keyframe (ids distinct inside one
 * keyframe); extra[i] what the projected search and the solver need beyond it.
 * LLD_ERR_INVALID before anything is queued, the frame unchanged: no lld_frame_compute_bow on this frame yet, a NULL argument, n_candidates
 * outside [1, LLD_PNP_MAX_SOLVERS], any per-candidate condition lld_frame_track_reference_keyframe refuses, a candidate with keypoints but
 * no max_distance / min_distance, cam.fx or cam.fy not > 0, a frame without level_inv_sigma2 or (nt > 0) angles, pnp parameters
 * lld_pnp_batch_create refuses (min_set other than 4: LLD_ERR_UNSUPPORTED).  All candidates discarded before PnP (isBad, or fewer than 15
 * matches): matched = 0, no round queued (nCandidates == 0, :1894).  Synchronous: returns when the routine has ended.
 * Any other error (LLD_ERR_ALLOC, LLD_ERR_HIP) may arrive after the frame was emptied for the routine: it then holds nothing, at the pose handed in. */
#define LLD_RELOC_RUNG_POSE1   1         /* PoseOptimization on the PnP inliers (:1936)                                          */
#define LLD_RELOC_RUNG_SEARCH1 2         /* nGood < 50: SearchByProjection(.., 10, 100) (:1948)                                  */
#define LLD_RELOC_RUNG_POSE2   4         /* nadditional + nGood >= 50: PoseOptimization (:1952)                                  */
#define LLD_RELOC_RUNG_SEARCH2 8         /* 30 < nGood < 50: SearchByProjection(.., 3, 64) (:1962)                               */
#define LLD_RELOC_RUNG_POSE3   16        /* nGood + nadditional >= 50: PoseOptimization and discard (:1967-1971)                 */
typedef struct {
  const float*    max_distance;          /* [n] mfMaxDistance of GetMapPointMatches()[k] (ignored where point_id is -1)          */
  const float*    min_distance;          /* [n] mfMinDistance                                                                    */
  const uint32_t* point_desc;            /* [n][8] pMP->GetDescriptor() (ORBmatcher.cc:1530), or NULL: the keyframe's own desc   */
  int32_t  is_bad;                       /* pKF->isBad() (:1869)                                                                 */
  uint32_t seed;                         /* srand(seed) of this candidate's PnPsolver                                            */
} lld_reloc_candidate;
typedef struct {
  int32_t matched;                       /* bMatch                                                                               */
  int32_t winner;                        /* index into candidates, -1                                                            */
  int32_t round;                         /* 1-based round of the while loop (:1894) in which it won, 0                           */
  int32_t n_good;                        /* the winner's nGood, 0                                                                */
  int32_t n_rounds;                      /* rounds run                                                                           */
  int32_t n_kept;                        /* nCandidates after the BoW gate (:1884)                                               */
  float   Tcw[16];                       /* mCurrentFrame.mTcw at return (matched = 0: the pose handed in)                       */
  /* per candidate, caller-allocated [n_candidates], any may be NULL */
  int32_t* n_bow;                        /* SearchByBoW's return value (0 for an isBad keyframe: the reference does not search)  */
  uint8_t* discarded;                    /* vbDiscarded[i] at return                                                             */
  int32_t* rounds;                       /* iterate(5) calls the candidate received                                              */
  int32_t* n_good_last;                  /* nGood at the end of its last attempt (a round that gave it a pose), -1: none         */
  int32_t* rungs;                        /* OR of LLD_RELOC_RUNG_* its last attempt took                                         */
  int32_t* n_additional1;                /* nadditional of the (10, 100) search of that attempt, 0 when not run                  */
  int32_t* n_additional2;                /* ... of the (3, 64) search                                                            */
} lld_reloc_result;
int  lld_frame_relocalize(lld_frame* frame, const lld_track_params* params, const lld_frame_view* view, const double* pose_qt,
                          int32_t n_candidates, const lld_ref_keyframe* candidates, const lld_reloc_candidate* extra, const lld_pnp_params* pnp,
                          lld_reloc_result* out);

/* ================================================================== Sim3Solver (src/Sim3Solver.cc), LoopClosing::ComputeSim3's RANSAC
 * A batch of independent Sim3Solvers, one per loop candidate, whose RANSAC state stays in HBM between iterate() calls.  The prefix
 * is lld_sim3solver_ (lld_sim3_ is OptimizeSim3 above).  The interface is the reference's: the constructor (lld_sim3solver_problem),
 * SetRansacParameters (lld_sim3solver_params), iterate(n, bNoMore, vbInliers, nInliers) (lld_sim3solver_batch_iterate + _download),
 * find() (lld_sim3solver_batch_find) and GetEstimatedRotation / Translation / Scale (the best hypothesis, in the result).
 * Restated literally:
 *   Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) (:37-112): the caller walks vpMatched12 (length mN1 = n1) and skips an entry
 *     whose vpMatched12[i1] or pKF1->GetMapPointMatches()[i1] is NULL, either point isBad(), or either GetIndexInKeyFrame < 0;
 *     correspondence i carries both GetWorldPos() (float xyz), mvLevelSigma2[kp.octave] of both keypoints and index1 = i1.
 *     adapters/lld_sim3_adapter.cc does this on live objects.  lld_sim3solver_batch_create then computes, on the host:
 *     mvX3Dc1/2 = Rcw*Xw + tcw (float), mvP1im1 / mvP2im2 by FromCameraToImage (float: invz = 1/z, x = X*invz, u = fx*x + cx),
 *     mvnMaxError1/2 = 9.210*sigma2 in double TRUNCATED to an integer (std::vector<size_t>, include/Sim3Solver.h:78-79: sigma2
 *     1 -> 9, 1.44 -> 13, 2.0736 -> 19, 2.986 -> 27), compared as err < (float)maxErr.
 *   SetRansacParameters (:114-138): epsilon = (float)minInliers/N; nIterations = 1 when minInliers == N, else
 *     ceil(log(1-p)/log(1-pow(epsilon,3))); mRansacMaxIts = max(1, min(nIterations, maxIterations)).  LoopClosing's values
 *     (0.99, 20, 300, LoopClosing.cc:277) are the defaults here, not the header's minInliers = 6.
 *   iterate (:140-207): outputs reset (vbInliers: n1 entries, false); N < mRansacMinInliers -> bNoMore, no draws, no pose.  The
 *     loop runs while mnIterations < mRansacMaxIts AND nCurrentIterations < n (PnPsolver has OR: here a call after the budget is
 *     spent draws nothing and returns bNoMore).  Each iteration draws 3 indices (RandomInt over a fresh copy of mvAllIndices, the
 *     back swapped into the taken place), runs ComputeSim3 and CheckInliers.  A hypothesis with mnInliersi >= mnBestInliers
 *     becomes the best (ties replace it; the first one becomes the best even with 0 inliers); a best with mnInliersi >
 *     mRansacMinInliers returns T12 at once, before the bNoMore test (a success on the budget's last iteration has bNoMore false),
 *     with vbInliers set at index1 of its inliers.  Otherwise bNoMore = mnIterations >= mRansacMaxIts and no pose.
 *   find() (:209-213) is iterate(mRansacMaxIts), continuing the solver's state.
 *   ComputeSim3 (:226-337), Horn's closed form on the 3 sampled points in float: centroids O1, O2 and Pr = P - O; M = Pr2*Pr1^T;
 *     the 10 entries of N from M's floats (float sums, stored in double, then into a float 4x4); the eigenvector q of N's largest
 *     eigenvalue; ang = atan2(||q.xyz||, q.w); vec = 2*ang*q.xyz/||q.xyz||; R12 = Rodrigues(vec); P3 = R12*Pr2; s = (float)(nom/den)
 *     with nom = Pr1.dot(P3) and den = sum of P3's squares (floats) both in double, or 1 under fix_scale; t = O1 - (s*R)*O2;
 *     T12 = [sR | t]; T21 = [(1/s)R^T | -((1/s)R^T) t].
 *   CheckInliers (:340-364): X3Dc2 through T12 into K1 and X3Dc1 through T21 into K2 (Project: P3Dc = R*X + t, then as
 *     FromCameraToImage); err = dist.dot(dist) as float; an inlier when both errors are below their thresholds.  No depth test.
 *   Non-finite values follow IEEE with no special case: a sample whose rotation is exactly the identity has ||q.xyz|| = 0, so vec,
 *   R, T12 and T21 are NaN and the hypothesis has 0 inliers (and becomes the best if it is the first).
 * DEVIATION 1 (the sample stream): as lld_pnp's DEVIATION 1.  RandomInt draws from the process-global rand(), which the
 *   LoopClosing thread shares with Tracking.  Here every solver owns a glibc TYPE_3 rand() stream after srand(seed), so one batched
 *   round (iterate(5) on every live candidate, LoopClosing.cc:289-342) gives exactly what the sequential round robin gives for
 *   every candidate it reaches.
 * DEVIATION 2 (numerics left to OpenCV): these choices are this library's, restated identically in tests/sim3solver_ref.py.
 *   Products and dot products of float matrices (Rcw*X, Pr2*Pr1^T, R*Pr2, (s*R)*O2, sRinv*t, Project's R*X, Mat::dot, cv::norm):
 *   the float products summed in double in index order, starting from the first, rounded to float once, then the float + t.
 *   Centroids: the float sum of the three columns in order, divided by 3.0f.  s*R: the float product; (1/s)*R^T: the double
 *   quotient times the widened float, rounded.  vec: alpha = (2*ang)/||q.xyz|| in double, vec_i = (float)(q_i*alpha).
 *   cv::eigen(N): lld_pnp's cyclic Jacobi in fp64 on the widened N (same sweeps and tolerance); the largest eigenvalue, the lowest
 *   index on a tie; canonical sign (the first largest-magnitude component positive); rounded to float.  cv::Rodrigues: theta =
 *   ||vec|| in double; theta < DBL_EPSILON gives the identity; else r = vec/theta and R_ij = (cos*d_ij + (1-cos)*(r_i*r_j)) +
 *   sin*[r]x_ij in double, rounded to float.  Device atan2 / sin / cos may differ from glibc by an ulp of double; R, t and s
 *   hold to the restatement within 1 float ulp.  The kernels are compiled without FMA contraction.
 * Limits: LLD_ERR_INVALID / LLD_ERR_UNSUPPORTED with nothing allocated: nulls; n < 1 or more than LLD_SIM3S_MAX_SOLVERS solvers;
 *   more than LLD_SIM3S_MAX_CORRESPONDENCES correspondences or LLD_SIM3S_MAX_KEYPOINTS keypoints (n1); an index1 out of range or
 *   repeated; a sigma2 that is negative, not finite or 9.210*sigma2 >= 2^32; fx or fy of either keyframe not > 0; min_inliers < 3
 *   (UNSUPPORTED: a draw needs 3 correspondences); max_iterations outside 1..LLD_SIM3S_MAX_ITERATIONS, probability outside (0, 1).
 *   lld_sim3solver_batch_iterate: n_iterations < 1 (INVALID) or above LLD_SIM3S_MAX_ITERATIONS (UNSUPPORTED).  A handle is driven
 *   by one host thread at a time, on its context's stream. */
#define LLD_SIM3S_MAX_CORRESPONDENCES 8192  /* per solver                                      */
#define LLD_SIM3S_MAX_KEYPOINTS 8192        /* mN1 (length of vbInliers)                       */
#define LLD_SIM3S_MAX_SOLVERS 256           /* per batch                                       */
#define LLD_SIM3S_MAX_ITERATIONS 65536      /* maxIterations and iterate()'s n                 */
typedef struct {
  double probability;                    /* 0.99                                                  */
  int32_t min_inliers;                   /* 20                                                    */
  int32_t max_iterations;                /* 300                                                   */
} lld_sim3solver_params;
void lld_sim3solver_params_default(lld_sim3solver_params* p);   /* SetRansacParameters(0.99, 20, 300) (LoopClosing.cc:277) */
typedef struct {
  int32_t n;                             /* correspondences                                       */
  const float* xyz1;                     /* [3n] pMP1->GetWorldPos()                              */
  const float* xyz2;                     /* [3n] pMP2->GetWorldPos()                              */
  const float* sigma2_1;                 /* [n]  pKF1->mvLevelSigma2[kp1.octave]                  */
  const float* sigma2_2;                 /* [n]  pKF2->mvLevelSigma2[kp2.octave]                  */
  const int32_t* index1;                 /* [n]  mvnIndices1: distinct, in [0, n1)                */
  int32_t n1;                            /* mN1 = vpMatched12.size()                              */
  float Rcw1[9], tcw1[3];                /* pKF1->GetRotation() (row-major), GetTranslation()     */
  float Rcw2[9], tcw2[3];
  float fx1, fy1, cx1, cy1;              /* pKF1->mK                                              */
  float fx2, fy2, cx2, cy2;              /* pKF2->mK                                              */
  int32_t fix_scale;                     /* bFixScale                                             */
  uint32_t seed;                         /* srand(seed) of this solver's stream (DEVIATION 1)     */
} lld_sim3solver_problem;
typedef struct {
  float T12[12];                         /* 3x4 row-major [sR | t] iterate() returned, or zeros   */
  float R[9], t[3], s;                   /* GetEstimatedRotation / Translation / Scale (the best; zeros before any hypothesis) */
  int32_t has_pose;                      /* iterate() returned a non-empty Mat                    */
  int32_t n_inliers;                     /* nInliers                                              */
  int32_t no_more;                       /* bNoMore                                               */
  int32_t iterations;                    /* mnIterations                                          */
  int32_t best_inliers;                  /* mnBestInliers                                         */
  int32_t n1;                            /* out: entries written to inlier                        */
  uint8_t* inlier;                       /* [n1] vbInliers, caller-allocated, or NULL             */
} lld_sim3solver_result;
typedef struct {                          /* diagnostic: one hypothesis of the last iterate call   */
  int32_t n_inliers;                     /* mnInliersi                                            */
  int32_t record;                        /* 1: it became the best (>= mnBestInliers)              */
  int32_t idx[3];                        /* the sampled correspondences                           */
  float s;                               /* ms12i                                                 */
  float R[9], t[3];                      /* mR12i, mt12i                                          */
  float T12[12];                         /* mT12i rows 0..2                                       */
} lld_sim3solver_hypothesis;
typedef struct lld_sim3solver_batch lld_sim3solver_batch;
/* n Sim3Solvers with SetRansacParameters(params): the constructor's camera points, projections and thresholds, then one upload. */
int  lld_sim3solver_batch_create(lld_ctx* ctx, int32_t n, const lld_sim3solver_problem* problems, const lld_sim3solver_params* params,
                                 lld_sim3solver_batch** out);
/* iterate(n_iterations) on every solver with active[s] != 0 (active NULL: all), on the device, with no host trip between the
 * kernels; queued on the context's stream.  Inactive solvers keep their state and last results. */
int  lld_sim3solver_batch_iterate(lld_sim3solver_batch* b, int32_t n_iterations, const uint8_t* active);
/* find() (:209-213) on every active solver: iterate(mRansacMaxIts) of each, continuing its state like the reference's find(). */
int  lld_sim3solver_batch_find(lld_sim3solver_batch* b, const uint8_t* active);
/* The last iterate's outputs of every solver (outs[n]); waits for the stream. */
int  lld_sim3solver_batch_download(lld_sim3solver_batch* b, lld_sim3solver_result* outs);
/* Diagnostic (tests): the hypotheses drawn by the last iterate call of `solver`.  n_window: hypotheses evaluated (min(n,
 * mRansacMaxIts - mnIterations), speculative ones past a returned pose included); n_run: the iterations iterate() made.  The
 * first min(capacity, n_window) are written.  An inactive solver reports 0 / 0. */
int  lld_sim3solver_batch_hypotheses(lld_sim3solver_batch* b, int32_t solver, int32_t capacity, lld_sim3solver_hypothesis* out,
                                     int32_t* n_window, int32_t* n_run);
void lld_sim3solver_batch_destroy(lld_sim3solver_batch* b);
/* find() on one freshly constructed solver: create, lld_sim3solver_batch_find, download, destroy. */
int  lld_sim3solver_find(lld_ctx* ctx, const lld_sim3solver_problem* problem, const lld_sim3solver_params* params,
                         lld_sim3solver_result* out);

/* ================================================================== Initializer (src/Initializer.cc), the monocular bootstrap
 * Tracking::MonocularInitialization (src/Tracking.cc:579-640) builds Initializer(mCurrentFrame, 1.0, 200) on the reference frame
 * and calls Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated) on every later frame until it succeeds;
 * mvIniMatches comes from ORBmatcher::SearchForInitialization (lld_search_for_initialization above).  A handle lives as long as
 * the reference's object: lld_initializer_create is the constructor (:33-42; mvKeys1 stays in HBM), lld_initializer_initialize
 * is Initialize() (:44-121).  One call queues its whole sequence on the context's stream with no host trip between the kernels.
 * Restated literally:
 *   Match list (:51-63): mvMatches12 = (i, vMatches12[i]) for every vMatches12[i] >= 0, in index order; N = its length.
 *   Sets (:78-97): all iterations x 8 draws come from one stream, in order; each draw is RandomInt(0, size-1) over a fresh copy
 *     of 0..N-1 per iteration, the back swapped into the taken place.  Built on the host inside the call, before its one upload.
 *   Normalize (:749-795) over ALL keypoints of a frame, not only the matched: float means summed in index order, mean = sum/N,
 *     float mean absolute deviations summed in index order, sX = (float)(1.0/meanDevX); point = (x - meanX)*sX in float;
 *     T = [sX 0 -meanX*sX; 0 sY -meanY*sY; 0 0 1].  On the host (create for frame 1, initialize for frame 2).
 *   ComputeH21 (:226-266): rows 2i = (0 0 0 -u1 -v1 -1 v2*u1 v2*v1 v2), 2i+1 = (u1 v1 1 0 0 0 -u2*u1 -u2*v1 -u2), float entries;
 *     Hn = the null vector of the 16x9 system.  ComputeF21 (:268-303): rows (u2*u1 u2*v1 u2 v2*u1 v2*v1 v2 u1 v1 1); Fpre = the
 *     null vector of the 8x9 system; its full SVD with w[2] = 0; Fn = u*diag(w)*vt.
 *   Composition (:159-161, :210-212): H21i = T2inv*Hn*T1, H12i = H21i.inv(); F21i = T2t*Fn*T1, products left to right.
 *   CheckHomography (:305-388) / CheckFundamental (:390-468) in float, operation by operation as written there (1.0/x is the
 *     double quotient rounded to float): th = 5.991; th = 3.841 with thScore = 5.991; the test is `>`; a one-sided score term is
 *     added even when the other side fails; score is the sequential float sum in match order, bit for bit.
 *   Best hypothesis (:165, :216): replaced on strict `>`, starting from score 0.  When every hypothesis scores 0 (or NaN) the
 *     model has no winner: its matrix, inlier count and mask are zeros and win_H / win_F is -1.
 *   Model (:112-118): RH = SH/(SH+SF) in float; RH > 0.40 selects ReconstructH, otherwise (a 0/0 NaN included) ReconstructF.
 *     The chosen model having no winner (both scores 0) gives success = 0 with no motion hypothesis run; the reference would
 *     pass an empty Mat on.
 *   ReconstructF (:470-570): N = the winner's inliers; E21 = K.t()*F21*K; DecomposeE (:909-929): t = u.col(2)/norm, R1 = u*W*vt,
 *     R2 = u*W.t()*vt, each negated when its determinant < 0; CheckRT on (R1,t) (R2,t) (R1,-t) (R2,-t) in this order;
 *     nMinGood = max(int(0.9*N), minTriangulated); nsimilar counts nGood > 0.7*maxGood in double; maxGood < nMinGood or
 *     nsimilar > 1 fails; then the if / else-if chain on maxGood == nGood_k: the first equal one is examined and its
 *     parallax > minParallax decides, the next is not tried.
 *   ReconstructH (:572-732): A = K.inv()*H21*K, its full SVD, s = det(U)*det(Vt); d1/d2 < 1.00001 || d2/d3 < 1.00001 fails with
 *     no hypothesis run; aux1, aux3, aux_stheta, ctheta, aux_sphi, cphi in float; the eight hypotheses in the reference's order
 *     and signs (x1 = {a,a,-a,-a}, x3 = {b,-b,b,-b}, stheta / sphi = {c,-c,-c,c}); R = s*U*Rp*Vt, t = U*tp over its norm.  vn is
 *     computed by the reference (n flipped when n.z < 0) but never read, and is not computed here.  nGood > bestGood moves best to
 *     second, else nGood > secondBestGood; success when secondBestGood < 0.75*bestGood && bestParallax >= minParallax &&
 *     bestGood > minTriangulated && bestGood > 0.9*N.
 *   CheckRT (:798-907): vbGood and vP3D have n1 entries indexed by match.first.  P1 = K[I|0], P2 = K*[R|t], O2 = -R.t()*t.  Per
 *     inlier match: Triangulate (:734-747: rows x*P.row(2)-P.row(0), y*P.row(2)-P.row(1) of both cameras in float, the null
 *     vector of the 4x4, x3D = xyz/w); a non-finite coordinate skips the match; cosParallax = normal1.dot(normal2)/(dist1*dist2)
 *     as float; z1 <= 0 && cosParallax < 0.99998 skips; p3dC2 = R*p3dC1+t, z2 <= 0 && cosParallax < 0.99998 skips; the two
 *     reprojection errors in float against th2 = 4*sigma^2 (`>` skips); then cosParallax is pushed, vP3D written and nGood
 *     counted BEFORE vbGood is set only when cosParallax < 0.99998.  parallax = acos(sorted[min(50, size-1)])*180/pi, 0 when
 *     nGood == 0.  The selection here is exact (equal to sort-then-index; a NaN cosine orders by its bit pattern, where
 *     std::sort is undefined).
 *   Non-finite values follow IEEE with no special case beyond the reference's own isfinite test.
 * Outputs when success = 0: R21, t21, p3d and triangulated are zeros (the reference leaves its arguments untouched).
 *   best_index is the motion hypothesis the final rule examined (F: the first with nGood == maxGood once the count tests passed;
 *   H: bestSolutionIdx), -1 when there was none; n_good / parallax hold every hypothesis run (four for F), zeros otherwise.
 * DEVIATION 1 (the sample stream): the reference draws from the process-global rand(), seeded once per process by
 *   SeedRandOnce(0), so only a process's first Initialize is reproducible.  Here EVERY initialize call draws from a fresh glibc
 *   TYPE_3 stream after srand(seed); seed 0 equals srand(1), as in lld_pnp / lld_sim3solver.
 * DEVIATION 2 (numerics left to OpenCV): these choices are this library's, restated identically in tests/initializer_ref.py.
 *   Matrix products (also Mat::dot, R*p3dC1): the float products summed in double in index order from the first, rounded to float
 *   once; then the float + t.  A chain A*B*C is (A*B)*C.  u*diag(w) is the float product u_ik*w_k.  s*U is the float product.
 *   cv::norm: the square root of that double sum, in double; v/norm(v): the double reciprocal times the widened float, rounded;
 *   x3D/w likewise.  cv::determinant (3x3): (a0*(a4*a8-a5*a7) - a1*(a3*a8-a5*a6)) + a2*(a3*a7-a4*a6) in double on the widened
 *   entries.  Mat::inv (3x3): the cofactors in double times 1/det, rounded; det == 0 gives the zero matrix.  sqrt of a float: the
 *   double square root rounded to float.
 *   Null vector of the 16x9 / 8x9 / 4x4 systems: A^T A in double from the widened floats (each entry summed over the rows in order
 *   from 0.0), lld_pnp's cyclic Jacobi in fp64 (same sweeps and tolerance), the eigenvector of the smallest eigenvalue, the
 *   HIGHEST index on a tie, canonical sign (the first largest-magnitude component positive), rounded to float.
 *   Full 3x3 SVDs (rank-2 step of F, DecomposeE, ReconstructH): the same Jacobi on A^T A; eigenvalues ordered descending (the
 *   largest: lowest index on a tie; the smallest of the other two: highest index on a tie); v_k canonical; w_k = ||A v_k|| in
 *   double; u_k = A v_k / w_k.  U is completed when a singular value is (near) zero: u_0 = e_0 when w_0 = 0; u_1, when not
 *   w_1 > 1e-9*w_0, is the axis along which |u_0| is smallest (lowest index on a tie) made orthogonal to u_0 and normalised;
 *   u_2, when not w_2 > 1e-9*w_0, is u_0 x u_1.  So A = U*diag(w)*Vt holds to rounding, U's columns are orthonormal to 1e-7 or
 *   better, and s*U*Rp*Vt is a proper rotation whenever det(U)*det(Vt) = +-1 is, as in the reference.  U, w, Vt are then floats.
 *   Device acos may differ from glibc's by an ulp of double; nothing else differs.  No FMA contraction in the kernels.
 * Limits: LLD_ERR_INVALID / LLD_ERR_UNSUPPORTED with nothing allocated: nulls; n1, n2 or n12 below 1 (INVALID) or above
 *   LLD_INIT_MAX_KEYPOINTS (UNSUPPORTED); n12 != n1; a match value >= n2; fewer than 8 matches (the reference would draw from an
 *   empty vector); iterations outside 1..LLD_INIT_MAX_ITERATIONS; sigma not > 0 or not finite; fx or fy not > 0 or K not finite;
 *   non-finite keypoints.  A handle is driven by one host thread at a time, on its context's stream. */
#define LLD_INIT_MAX_KEYPOINTS 8192         /* n1, n2 and the length of vMatches12             */
#define LLD_INIT_MAX_ITERATIONS 4096        /* mMaxIterations                                  */
typedef struct {
  float sigma;                           /* 1.0 (Tracking.cc:596)                                 */
  int32_t iterations;                    /* 200 (Tracking.cc:596)                                 */
  float min_parallax;                    /* 1.0 (Initializer.cc:116-118)                          */
  int32_t min_triangulated;              /* 50  (Initializer.cc:116-118)                          */
  uint32_t seed;                         /* srand(seed) of every call's stream (DEVIATION 1)      */
} lld_initializer_params;
void lld_initializer_params_default(lld_initializer_params* p);   /* (1.0, 200, 1.0, 50, 0) */
typedef struct {
  int32_t success;                       /* Initialize()'s return                                 */
  int32_t model;                         /* 0: ReconstructH ran (RH > 0.40), 1: ReconstructF      */
  float SH, SF, RH;
  float H21[9], F21[9];                  /* the winners, row-major; zeros without a winner        */
  int32_t n_inliers_H, n_inliers_F;
  float R21[9], t21[3];                  /* zeros unless success                                  */
  int32_t n_good[8];                     /* nGood of every motion hypothesis (four for F)         */
  float parallax[8];
  int32_t best_index;                    /* the motion hypothesis examined, or -1                 */
  int32_t n_matches;                     /* N = mvMatches12.size()                                */
  int32_t win_H, win_F;                  /* the winning iteration of each model, or -1            */
  uint8_t* inlier_H;                     /* [N]  vbMatchesInliersH (room for n1), or NULL         */
  uint8_t* inlier_F;                     /* [N]  vbMatchesInliersF (room for n1), or NULL         */
  float* p3d;                            /* [3*n1] vP3D, or NULL                                  */
  uint8_t* triangulated;                 /* [n1] vbTriangulated, or NULL                          */
} lld_initializer_result;
typedef struct {                          /* diagnostic: one hypothesis of the last initialize call */
  int32_t idx[8];                        /* mvSets[it]                                            */
  float M[9];                            /* H21i or F21i                                          */
  float score;                           /* currentScore                                          */
  int32_t n_inliers;                     /* true entries of vbCurrentInliers                      */
} lld_initializer_hypothesis;
typedef struct lld_initializer lld_initializer;
/* Initializer(ReferenceFrame, sigma, iterations) (:33-42): K row-major 3x3, keys1_xy = mvKeysUn[i].pt of the reference frame. */
int  lld_initializer_create(lld_ctx* ctx, const float* K, int32_t n1, const float* keys1_xy, const lld_initializer_params* params,
                            lld_initializer** out);
/* Initialize(CurrentFrame, vMatches12, ...) (:44-121): keys2_xy = mvKeysUn of the current frame, matches12[n12 = n1] = the index
 * in frame 2 matched to keypoint i of frame 1, or negative.  The caller sets the four pointers of `result` (each may be NULL)
 * before the call.  Waits for the stream. */
int  lld_initializer_initialize(lld_initializer* h, int32_t n2, const float* keys2_xy, int32_t n12, const int32_t* matches12,
                                lld_initializer_result* result);
/* Diagnostic (tests): the hypotheses of the last initialize call, model 0 = H, 1 = F, in iteration order.  *n: the iterations
 * run (0 before any call); the first min(capacity, *n) are written. */
int  lld_initializer_hypotheses(lld_initializer* h, int32_t model, int32_t capacity, lld_initializer_hypothesis* out, int32_t* n);
void lld_initializer_destroy(lld_initializer* h);
/* One shot: create, initialize, destroy. */
int  lld_initializer_find(lld_ctx* ctx, const float* K, int32_t n1, const float* keys1_xy, int32_t n2, const float* keys2_xy,
                          int32_t n12, const int32_t* matches12, const lld_initializer_params* params, lld_initializer_result* result);

/* ---- Landmark refresh: MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307), MapPoint::UpdateNormalAndDepth
 * (src/MapPoint.cc:330-371) and MapLine::ComputeDistinctiveDescriptors (src/MapLine.cc:133-201) for a batch of landmarks.
 * The reference runs them one object at a time in LocalMapping::ProcessNewKeyFrame / SearchInNeighbors (src/LocalMapping.cc:
 * 141-162, :518-531), CreateNewMapPoints, at the end of every Local / GlobalBundleAdjustment and in LoopClosing::CorrectLoop /
 * SearchAndFuse; what they write (mDescriptor, mNormalVector, mfMinDistance, mfMaxDistance) is what lld_orb_search_local_points
 * and lld_frame_track_local_map read.  Each call makes one upload, queues its kernels on the context's stream with no host trip
 * between them, makes one download and waits for the stream.
 * Input: the observations of landmark i are entries obs_start[i] .. obs_start[i+1]-1 (CSR), LISTED IN THE ORDER IN WHICH THE
 *   REFERENCE'S std::map<KeyFrame*,size_t> ITERATES (pointer order): that order decides ties and the float sum.  obs_kf[o] indexes a
 *   keyframe table of n_kf entries (kf_ow = GetCameraCenter(), kf_bad = isBad()); obs_desc[o] is the row the caller gathered from
 *   pKF->mDescriptors (pKF->mDescriptorsLines for lines).
 * Descriptor rule (MapPoint.cc):
 *   :251-252 mbBad returns; :256-257 no observations returns; :261-267 vDescriptors = the rows of the keyframes that are not bad,
 *     in order; :269-270 none left returns.  Such a point is left alone: desc[i] keeps what the caller passed in, best_obs[i] =
 *     best_median[i] = -1, bit 0 of updated[i] is clear.
 *   :273-285 Distances[i][j] = DescriptorDistance of every pair (the popcount of the XOR of the 256 bits), diagonal 0.
 *   :290-294 per row: the row sorted, median = element (size_t)(0.5*(N-1)), the diagonal zero included.  N = 1 and N = 2 give
 *     index 0, i.e. median 0 and winner 0.  Computed here without a sort (the smallest v with count(d <= v) > index): equal.
 *   :296-300 `median < BestMedian` from INT_MAX in row order: the first row with the strictly smallest median wins.
 *   :305 mDescriptor = the winner's row.  best_obs[i] is the winner's position in the point's OWN observation list, bad keyframes
 *     counted (so obs_start[i] + best_obs[i] is its entry); best_median[i] its median.
 * Normal / depth rule (MapPoint.cc):
 *   :338-339 mbBad returns; :345-346 no observations returns (bit 1 of updated[i] clear, outputs kept).  Bad keyframes are NOT
 *     skipped: the reference does not test isBad() here, and n counts every observation.
 *   :348-357 normal = 0; per observation in order: normali = mWorldPos - Owi (float subtraction), normal = normal +
 *     normali/cv::norm(normali) (float additions in observation order).
 *   :359-363 PC = Pos - Ow[ref_kf]; dist = (float)cv::norm(PC); level = ref_level[i], which the caller reads as
 *     pRefKF->mvKeysUn[observations[pRefKF]].octave - observations[pRefKF] is std::map::operator[], so a reference keyframe that is
 *     absent from the map yields keypoint 0 (the adapter reproduces this).
 *   :367-369 mfMaxDistance = dist*level_scale[level]; mfMinDistance = mfMaxDistance/level_scale[n_levels-1] (float product and
 *     quotient); mNormalVector = normal/n.
 *   Numerics, as lld_orb_search_local_points states them for isInFrustum: float subtraction; cv::norm sums the squares in double in
 *     index order and takes the double square root.  The one new choice is Mat / double (normali/norm, normal/n): OpenCV turns it
 *     into convertTo with alpha = 1/s, whose CV_32F -> CV_32F path works in float, so x/s here is x * (float)(1.0/s): the double
 *     reciprocal rounded to float, then one float product.  (Its `+ 0` shift is not performed: it could only turn a -0 into +0, and
 *     the sum starts from +0.)  The device's double division, double square root and float division are correctly rounded, so
 *     every output is bit for bit the restatement's.
 *   DEVIATION (scales): one level_scale table serves all keyframes; the reference reads pRefKF->mvScaleFactors and
 *     pRefKF->mnScaleLevels of each point's own reference keyframe (all equal in the reference's configurations: one extractor).
 * Line rule (MapLine.cc:133-201): the same selection with obs_desc[n_obs][dim] in float (dim = 72 for LBD).
 *   :175-177 distij = cv::norm(a - b) in the form lld_match_l2f32 fixes (float difference, squares summed in double in ascending
 *     index order, double square root), then STORED AS FLOAT in Distances.
 *   :186-188 QUIRK (int median): the row is sorted as floats, but the element is assigned to `int median`, so it is truncated
 *     toward zero BEFORE the `median<BestMedian` test.  With unit-norm LBD rows almost every median truncates to 0 or 1 and the
 *     first kept row wins.  best_median[i] is that int.  The sorted element is found by rank count, equal to sort-then-index for
 *     finite distances; non-finite descriptors or a distance of 2^31 or more are outside the contract (std::sort and the
 *     conversion are undefined there).
 *   There is no normal / depth part for lines.  updated[i] is 1 when the descriptor was written.
 * flags: LLD_LANDMARK_DESCRIPTOR, LLD_LANDMARK_NORMAL_DEPTH or both (LocalBundleAdjustment's tail and CorrectLoop want only the
 *   second).  Inputs and outputs of the part not selected are neither read nor written and may be NULL; updated[] is always written.
 * Limits: the reference's stack table `float Distances[N][N]` bounds N in practice (8 MiB of stack: N < 1449).  A point with more
 *   than LLD_LANDMARK_MAX_OBS observations, a line with more than LLD_LANDMARK_MAX_LINE_OBS, or dim above
 *   LLD_LANDMARK_MAX_LINE_DIM returns LLD_ERR_UNSUPPORTED before anything is queued.  LLD_ERR_INVALID, also before anything is
 *   queued: a NULL required pointer; negative sizes; flags zero or with unknown bits; obs_start[0] != 0, obs_start not
 *   non-decreasing or obs_start[n] != n_obs; an obs_kf outside [0, n_kf); with the normal part, n_levels outside
 *   [1, LLD_ORB_MAX_LEVELS], or ref_kf outside [0, n_kf) / ref_level outside [0, n_levels) for a point the rule does not skip; dim
 *   below 1.  n_points = 0 (n_lines = 0) is LLD_OK and touches nothing. */
#define LLD_LANDMARK_MAX_OBS 1024          /* observations of one MapPoint                          */
#define LLD_LANDMARK_MAX_LINE_OBS 64       /* observations of one MapLine                           */
#define LLD_LANDMARK_MAX_LINE_DIM 128      /* floats of one line descriptor                         */
#define LLD_LANDMARK_DESCRIPTOR   1u       /* flags / updated bit 0: ComputeDistinctiveDescriptors  */
#define LLD_LANDMARK_NORMAL_DEPTH 2u       /* flags / updated bit 1: UpdateNormalAndDepth           */
typedef struct {
  int32_t n_points, n_obs, n_kf, n_levels;
  uint32_t flags;
  const int32_t*  obs_start;             /* [n_points+1]                                          */
  const int32_t*  obs_kf;                /* [n_obs] index into the keyframe table                 */
  const uint32_t* obs_desc;              /* [n_obs][8] pKF->mDescriptors.row(mit->second)         */
  const float*    kf_ow;                 /* [n_kf][3] GetCameraCenter()                           */
  const uint8_t*  kf_bad;                /* [n_kf] isBad()                                        */
  const float*    pos;                   /* [n_points][3] mWorldPos                               */
  const uint8_t*  bad;                   /* [n_points] mbBad                                      */
  const int32_t*  ref_kf;                /* [n_points] mpRefKF in the keyframe table              */
  const int32_t*  ref_level;             /* [n_points] pRefKF->mvKeysUn[observations[pRefKF]].octave */
  const float*    level_scale;           /* [n_levels] mvScaleFactors                             */
} lld_mappoint_refresh_in;
typedef struct {                          /* in / out: an entry the rule leaves alone keeps its value */
  uint32_t* desc;                        /* [n_points][8] mDescriptor                             */
  int32_t*  best_obs;                    /* [n_points] BestIdx in the point's own list, or -1     */
  int32_t*  best_median;                 /* [n_points] BestMedian, or -1                          */
  float*    normal;                      /* [n_points][3] mNormalVector                           */
  float*    min_distance;                /* [n_points] mfMinDistance                              */
  float*    max_distance;                /* [n_points] mfMaxDistance                              */
  uint8_t*  updated;                     /* [n_points] bit 0 descriptor, bit 1 normal / depth     */
} lld_mappoint_refresh_out;
int lld_mappoint_refresh(lld_ctx* ctx, const lld_mappoint_refresh_in* in, lld_mappoint_refresh_out* out);
typedef struct {
  int32_t n_lines, n_obs, n_kf, dim;
  const int32_t* obs_start;              /* [n_lines+1]                                           */
  const int32_t* obs_kf;                 /* [n_obs]                                               */
  const float*   obs_desc;               /* [n_obs][dim] pKF->mDescriptorsLines.row(mit->second)  */
  const uint8_t* kf_bad;                 /* [n_kf]                                                */
  const uint8_t* bad;                    /* [n_lines] mbBad                                       */
} lld_mapline_distinctive_in;
typedef struct {
  float*   desc;                         /* [n_lines][dim] mDescriptor                            */
  int32_t* best_obs;                     /* [n_lines] or -1                                       */
  int32_t* best_median;                  /* [n_lines] the int of the QUIRK, or -1                 */
  uint8_t* updated;                      /* [n_lines] 1 when the descriptor was written           */
} lld_mapline_distinctive_out;
int lld_mapline_distinctive(lld_ctx* ctx, const lld_mapline_distinctive_in* in, lld_mapline_distinctive_out* out);

/* ================================================================== LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:208-453), the loop body
 * For the current keyframe (keyframe 1) and n_pairs covisible neighbours (keyframe 2 of each pair), every epipolar match that
 * ORBmatcher::SearchForTriangulation returned goes through the parallax test, the linear triangulation or the stereo
 * un-projection, the two depth tests, the two reprojection gates and the scale-consistency gate.  One call makes one upload,
 * queues its two kernels on the context's stream with no host trip between them, makes one download and waits for the stream.
 * What stays with the caller: the neighbour loop, ComputeF12, the search, ComputeSceneMedianDepth(2) (median_depth) and the
 * object bookkeeping (new MapPoint, AddObservation, AddMapPoint, lld_mappoint_refresh for the new points).
 * Restated literally:
 *   Derived per keyframe: Rwc = Rcw.t(); Ow = -Rwc*tcw (src/KeyFrame.cc:85); invfx = 1.0f/fx, invfy = 1.0f/fy (src/Frame.cc:150).
 *   Baseline gate (:245-262): baseline = (float)cv::norm(Ow2-Ow1) of the float difference.  Stereo: baseline < pKF2->mb skips the
 *     pair.  Mono: ratioBaselineDepth = baseline/median_depth (float quotient); ratioBaselineDepth < 0.01 (the double constant)
 *     skips it.  A skipped pair has pair_status 1, n_new 0 and every match LLD_NEWPTS_PAIR_SKIPPED.
 *   Per match (idx1, idx2) (:287-451): bStereo1 = ur1[idx1] >= 0, bStereo2 = ur2[idx2] >= 0 (:294, :298).
 *   :301-306 xn = ((x-cx)*invfx, (y-cy)*invfy, 1) in float from mvKeysUn; ray = Rwc*xn;
 *     cosParallaxRays = ray1.dot(ray2)/(cv::norm(ray1)*cv::norm(ray2)), a double expression stored in a float.
 *   :308-317 cosParallaxStereo1 = cosParallaxStereo2 = cosParallaxRays+1 (float).  QUIRK: `if(bStereo1) .. else if(bStereo2)` -
 *     with BOTH keypoints stereo only cosParallaxStereo1 is computed, the other stays cosParallaxRays+1.  cosParallaxStereo =
 *     min(cosParallaxStereo1, cosParallaxStereo2) (std::min: the second when it is strictly smaller).
 *   :320 cosParallaxRays<cosParallaxStereo && cosParallaxRays>0 && (bStereo1 || bStereo2 || cosParallaxRays<0.9998): two float
 *     tests and one against the double constant, all strict.  Then (:323-338) A.row(0) = xn1.x*Tcw1.row(2)-Tcw1.row(0), row(1)
 *     with xn1.y and Tcw1.row(1), rows 2 and 3 likewise from keyframe 2 (float product, float difference); x3D = the null vector
 *     of A; x3D[3] == 0 is W_ZERO (:334); x3D = x3D[0..2]/x3D[3].  source 0.
 *   :341 else if(bStereo1 && cosParallaxStereo1<cosParallaxStereo2): x3D = keyframe 1's UnprojectStereo(idx1), source 1.
 *   :345 else if(bStereo2 && cosParallaxStereo2<cosParallaxStereo1): x3D = keyframe 2's UnprojectStereo(idx2), source 2.
 *   :349-350 else LOW_PARALLAX.
 *   UnprojectStereo (src/KeyFrame.cc:638-654): z = mvDepth[i]; u, v from mvKeys - the RAW keypoint, not mvKeysUn (:643) -
 *     x = (u-cx)*z*invfx, y = (v-cy)*z*invfy in float, left to right; Rwc*(x,y,z)+Ow.  z > 0 failing returns an empty Mat, which
 *     the reference would fault on: here it is NO_DEPTH.
 *   :355-360 z1 = Rcw1.row(2).dot(x3D)+tcw1[2]; z1 <= 0 is Z1; z2 likewise, Z2.
 *   :364-388 x1, y1 like z1; invz1 = 1.0/z1, the double quotient rounded to float; u1 = fx1*x1*invz1+cx1, v1 = fy1*y1*invz1+cy1,
 *     errX1 = u1-kp1.x, errY1 = v1-kp1.y in float.  Mono keypoint: (errX1*errX1+errY1*errY1) > 5.991*sigmaSquare1; stereo:
 *     u1_r = u1-mbf*invz1, errX1_r = u1_r-kp1_ur, (errX1*errX1+errY1*errY1+errX1_r*errX1_r) > 7.8*sigmaSquare1.  The float sum
 *     is widened and compared with the DOUBLE product 5.991*sigma2 / 7.8*sigma2; the test is `>`.  REPROJ1.
 *   :391-414 the same for keyframe 2 with its own intrinsics and sigma2.  QUIRK: u2_r = u2 - mpCurrentKeyFrame->mbf*invz2 (:407),
 *     the CURRENT keyframe's mbf.  REPROJ2.
 *   :417-423 dist1 = (float)cv::norm(x3D-Ow1), dist2 = (float)cv::norm(x3D-Ow2); dist1 == 0 || dist2 == 0 is DIST_ZERO.
 *   :426-432 ratioDist = dist2/dist1; ratioOctave = mvScaleFactors1[octave1]/mvScaleFactors2[octave2]; ratioFactor =
 *     1.5f*mfScaleFactor; ratioDist*ratioFactor<ratioOctave || ratioDist>ratioOctave*ratioFactor, all in float, is SCALE.
 *   Otherwise the point is created: status NEW.  Non-finite values follow IEEE with no special case (a NaN fails every test,
 *     so a NaN point can come out NEW, as in the reference).
 * Numerics left to OpenCV and libm: DEVIATION 2 of the Initializer section, unchanged.  Rwc*xn, Rwc*tcw, Rwc*x3Dc: the float
 *   products summed in double in index order, rounded to float once; then the float + Ow.  Mat::dot is that double sum, and the
 *   C++ expression it stands in (dot/(norm*norm), dot+t) is evaluated in double and rounded where it is assigned to a float.
 *   cv::norm: the double square root of the double sum.  The 4x4 null vector: A^T A in double from the widened floats, the shared
 *   cyclic Jacobi, the eigenvector of the smallest eigenvalue (the highest index on a tie), canonical sign, rounded to float.
 *   x3D/w: the double reciprocal times the widened float, rounded.  No FMA contraction.
 * DEVIATION (stereo parallax): cos(2*atan2(mb/2, depth)) (:313, :315) is evaluated as (d*d-a*a)/(d*d+a*a) in double on the widened
 *   floats d = depth and a = mb/2 (a float), rounded to float.  The reference's chain of float libm calls cannot be reproduced bit
 *   for bit; the closed form is the exact value correctly rounded, the same on host and device.  It differs from the float chain
 *   by a few ulp, which matters only where cosParallaxRays is that close to it.
 * Outputs (each pointer may be NULL): status / source / x3d per match (x3d zeros unless NEW; source names the branch taken, 0
 *   where none was: LOW_PARALLAX and PAIR_SKIPPED); pair_status / n_new per pair; new_match = the global match indices with status
 *   NEW in the reference's creation order (pair-major, match order within a pair; room for the number of matches);
 *   n_new_total is always written.
 * Limits, refused before anything is allocated: LLD_ERR_INVALID for a NULL required pointer (ctx, in, out, kf2, key_start and
 *   match_start always; with at least one match also matches, keys1_xy, ur1, depth1, octave1, keys2_xy, ur2, depth2 and octave2 -
 *   without a match none of these is read and each may be NULL; keys*_raw_xy may always be NULL), n_pairs < 1, a negative count, a
 *   *_start array that does not begin at 0 or decreases, an idx1 / idx2 outside its keyframe, an octave of a matched keypoint
 *   outside its level table, n_levels outside 1..LLD_ORB_MAX_LEVELS, a non-finite pose / intrinsic / mb / mbf / scale_factor
 *   (median_depth too when monocular), fx or fy not > 0; LLD_ERR_UNSUPPORTED for n_pairs > LLD_NEWPTS_MAX_PAIRS or more than
 *   LLD_NEWPTS_MAX_MATCHES matches in all.  No match in a pair, or in the whole call, is valid. */
#define LLD_NEWPTS_MAX_PAIRS 64
#define LLD_NEWPTS_MAX_MATCHES 65536
#define LLD_NEWPTS_NEW           0         /* the point is created                                  */
#define LLD_NEWPTS_LOW_PARALLAX  1         /* :349-350                                              */
#define LLD_NEWPTS_W_ZERO        2         /* :334                                                  */
#define LLD_NEWPTS_Z1            3         /* :356                                                  */
#define LLD_NEWPTS_Z2            4         /* :360                                                  */
#define LLD_NEWPTS_REPROJ1       5         /* :375-376, :386-387                                    */
#define LLD_NEWPTS_REPROJ2       6         /* :401-402, :412-413                                    */
#define LLD_NEWPTS_DIST_ZERO     7         /* :423                                                  */
#define LLD_NEWPTS_SCALE         8         /* :431                                                  */
#define LLD_NEWPTS_NO_DEPTH      9         /* UnprojectStereo with depth <= 0                       */
#define LLD_NEWPTS_PAIR_SKIPPED 10         /* the baseline gate skipped the pair                    */
#define LLD_NEWPTS_SRC_TRIANGULATED 0
#define LLD_NEWPTS_SRC_STEREO1      1
#define LLD_NEWPTS_SRC_STEREO2      2
typedef struct {
  float Rcw[9], tcw[3];                  /* GetRotation() row-major, GetTranslation()             */
  float fx, fy, cx, cy;
  float mb, mbf;                         /* mbf is read from keyframe 1 only (:381, :407)         */
  float scale_factor;                    /* mfScaleFactor, read from keyframe 1 only (:233)       */
  float median_depth;                    /* ComputeSceneMedianDepth(2): neighbours, monocular only */
  int32_t n_levels;
  float scale_factors[LLD_ORB_MAX_LEVELS];   /* mvScaleFactors                                    */
  float level_sigma2[LLD_ORB_MAX_LEVELS];    /* mvLevelSigma2                                     */
} lld_new_points_kf;
typedef struct {
  lld_new_points_kf kf1;                 /* mpCurrentKeyFrame                                     */
  int32_t monocular;                     /* mbMonocular (0 / 1)                                   */
  int32_t n_keys1;
  const float*   keys1_xy;               /* [n_keys1][2] mvKeysUn[i].pt                           */
  const float*   keys1_raw_xy;           /* [n_keys1][2] mvKeys[i].pt, NULL: equal to keys1_xy    */
  const float*   ur1;                    /* [n_keys1] mvuRight                                    */
  const float*   depth1;                 /* [n_keys1] mvDepth                                     */
  const int32_t* octave1;                /* [n_keys1] mvKeysUn[i].octave                          */
  int32_t n_pairs;
  int32_t reserved;
  const lld_new_points_kf* kf2;          /* [n_pairs] the neighbours                              */
  const int32_t* key_start;              /* [n_pairs+1] the neighbours' keypoints, concatenated   */
  const float*   keys2_xy;
  const float*   keys2_raw_xy;           /* NULL: equal to keys2_xy                               */
  const float*   ur2;
  const float*   depth2;
  const int32_t* octave2;
  const int32_t* match_start;            /* [n_pairs+1] vMatchedIndices of each pair, concatenated */
  const int32_t* matches;                /* [n_matches][2] (idx1, idx2 within the pair's keyframe) */
} lld_new_points_in;
typedef struct {                          /* every pointer may be NULL                             */
  uint8_t* status;                       /* [n_matches] LLD_NEWPTS_*                              */
  uint8_t* source;                       /* [n_matches] LLD_NEWPTS_SRC_*                          */
  float*   x3d;                          /* [n_matches][3] zeros unless NEW                       */
  uint8_t* pair_status;                  /* [n_pairs] 0 run, 1 skipped by the baseline gate       */
  int32_t* n_new;                        /* [n_pairs]                                             */
  int32_t* new_match;                    /* [n_matches] the first n_new_total entries are written */
  int32_t  n_new_total;
} lld_new_points_out;
int lld_new_points_triangulate(lld_ctx* ctx, const lld_new_points_in* in, lld_new_points_out* out);

/* ---- Covisibility counting: KeyFrame::UpdateConnections (src/KeyFrame.cc:312-402), the vote of Tracking::UpdateLocalKeyFrames and
 * the redundancy count of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:633-697) for a batch of keyframes ("queries") in one
 * call.  The reference runs them one keyframe at a time over copies of MapPoint::mObservations: in LocalMapping::
 * ProcessNewKeyFrame (:165) and SearchInNeighbors (:534), in Tracking (:696-697, :1358) and once per keyframe of the corrected
 * neighbourhood in LoopClosing::CorrectLoop (:434, :517, :556).  What UpdateConnections writes is what lld_kfdb_set_covisibles,
 * GetBestCovisibilityKeyFrames and the local-BA window builder consume.  Every result is an integer, so the call is exact and
 * bit-reproducible.  Each call makes one upload, queues its kernels on the context's stream with no host trip between them,
 * makes one download and waits for the stream once.
 * Keyframe table: n_kf slots, no per-slot data.  THE CALLER NUMBERS THE KEYFRAMES IN THE ORDER IN WHICH THE REFERENCE'S
 *   std::map<KeyFrame*, ...> ITERATES THEM (pointer order, std::less<KeyFrame*>): THAT ORDER DECIDES EVERY TIE BELOW.
 * Map points: the observations of point p are entries obs_start[p] .. obs_start[p+1]-1 (the CSR layout of lld_mappoint_refresh);
 *   obs_kf[o] is the observing keyframe's slot, obs_octave[o] = pKFi->mvKeysUn[mit->second].octave (culling only), point_bad[p] =
 *   isBad(), point_nobs[p] = MapPoint::Observations(), i.e. the stereo-weighted nObs and not the list length (culling only).
 * Queries: query_kf[q] is the slot of the keyframe itself, or -1 to exclude nobody (a Frame's vote in UpdateLocalKeyFrames,
 *   Tracking.cc).  Entries q_start[q] .. q_start[q+1]-1 of q_point are the entries of mvpMapPoints that are not NULL, in keypoint
 *   order; a point listed twice counts twice, as the reference's walk over the vector counts it.  For culling, q_octave[e] =
 *   pKF->mvKeysUn[i].octave and q_depth[e] = pKF->mvDepth[i] per entry, q_th_depth[q] = pKF->mThDepth per query, and `monocular`.
 * Connections rule (KeyFrame.cc):
 *   :329-333 a NULL entry and a bad point are skipped (the caller lists no NULL entries).
 *   :335-342 for every observation whose slot differs from query_kf[q]: counter[slot]++.
 *   :346-347 an empty counter returns: updated[q] = 0, the query owns no entries of either list, n_max[q] = 0, kf_max[q] = -1.
 *   :390     mConnectedKeyFrameWeights = KFcounter: entries conn_start[q] .. conn_start[q+1]-1 of conn_kf / conn_weight are every
 *            non-zero counter in ascending slot order (map order).
 *   :359-363 nmax / pKFmax: the first `>` in map order, so kf_max[q] is the LOWEST slot that holds the maximum; n_max[q] and
 *            kf_max[q] are always written.
 *   :364-368 the counters >= th are the pairs (weight, keyframe).
 *   :371-375 if there is none, the single pair (nmax, pKFmax).
 *   :377-384 sort of pair<int,KeyFrame*> ascending, then push_front: ordered_kf / ordered_weight (entries ordered_start[q] ..)
 *            are by DESCENDING weight, equal weights by DESCENDING slot.
 *   The AddConnection calls on the neighbours (:367, :374) and the first-connection parent (:394-399) belong to the caller
 *   (adapters/lld_covisibility_adapter.cc applies them).
 *   Capacities: conn_capacity / ordered_capacity are the entries the caller's conn_* / ordered_* arrays hold over all queries.
 *   The totals needed are always written to n_conn / n_ordered.  If either capacity is short the call returns LLD_ERR_INVALID
 *   with only those two totals written.  sum over q of min(n_kf, observations of q's entries) always suffices for both.
 * Culling rule (LocalMapping.cc), per query:
 *   :655-657 a bad point is skipped.
 *   :659-663 unless `monocular`, an entry with q_depth > q_th_depth || q_depth < 0 is skipped (float compares, exactly these two:
 *            depth == th_depth is kept).
 *   :665     n_mps++.
 *   :666     only if point_nobs > th_obs:
 *   :668-684 count the point's observations with slot != query_kf[q] and obs_octave <= q_octave + 1.  The reference breaks at
 *            th_obs, so its test is "count >= th_obs", which does not depend on the order of the observations.
 *   :685-688 if it holds, n_redundant++.
 *   :694     redundant[q] = (n_redundant > redundant_ratio * n_mps): the int against the double product, as written there.
 *   The mnId==0 skip (:644-645) and SetBadFlag (:695) belong to the caller.  SetBadFlag erases observations, so the counts of the
 *   keyframes after a culled one change: the adapter calls again for the rest.
 * flags: LLD_COVIS_CONNECTIONS, LLD_COVIS_CULLING or both.  Arrays of the part not selected are neither read nor written and may
 *   be NULL.  phase_ms may be NULL; otherwise it receives the HIP-event times of the upload, the kernels and the download.
 * Limits: n_kf above LLD_COVIS_MAX_KF (64 KB of LDS counters) returns LLD_ERR_UNSUPPORTED before anything is queued.
 *   LLD_ERR_INVALID, also before anything is queued: a NULL required pointer; a negative size or capacity; flags zero or with
 *   unknown bits; obs_start / q_start not starting at 0, not non-decreasing or not ending at n_obs / n_entries; an obs_kf outside
 *   [0, n_kf); a query_kf outside [-1, n_kf); a q_point outside [0, n_points).  n_queries = 0 is LLD_OK and touches nothing. */
#define LLD_COVIS_MAX_KF 16384             /* keyframe slots of one call                            */
#define LLD_COVIS_CONNECTIONS 1u           /* flags bit 0: UpdateConnections / the local-keyframe vote */
#define LLD_COVIS_CULLING     2u           /* flags bit 1: KeyFrameCulling's redundancy count       */
typedef struct {
  int32_t th;                            /* 15  (KeyFrame.cc:353)                                 */
  int32_t th_obs;                        /* 3   (LocalMapping.cc:648)                             */
  double  redundant_ratio;               /* 0.9 (LocalMapping.cc:694)                             */
} lld_covisibility_params;
void lld_covisibility_params_default(lld_covisibility_params* p);
typedef struct {
  int32_t n_kf, n_points, n_obs, n_queries, n_entries;
  int32_t monocular;                     /* mbMonocular: no depth test in the culling part        */
  uint32_t flags;
  lld_covisibility_params params;
  const int32_t* obs_start;              /* [n_points+1]                                          */
  const int32_t* obs_kf;                 /* [n_obs] slot of the observing keyframe                */
  const int32_t* obs_octave;             /* [n_obs] culling only                                  */
  const uint8_t* point_bad;              /* [n_points]                                            */
  const int32_t* point_nobs;             /* [n_points] MapPoint::Observations(); culling only     */
  const int32_t* query_kf;               /* [n_queries] own slot, or -1                           */
  const int32_t* q_start;                /* [n_queries+1]                                         */
  const int32_t* q_point;                /* [n_entries] the non-NULL mvpMapPoints in keypoint order */
  const int32_t* q_octave;               /* [n_entries] culling only                              */
  const float*   q_depth;                /* [n_entries] culling only                              */
  const float*   q_th_depth;             /* [n_queries] culling only                              */
} lld_covisibility_in;
typedef struct {
  int32_t  conn_capacity, ordered_capacity;   /* in: entries of conn_* / ordered_*               */
  int32_t  n_conn, n_ordered;            /* out: entries needed, always written                   */
  int32_t* conn_start;                   /* [n_queries+1]                                         */
  int32_t* conn_kf;                      /* [conn_capacity] ascending slot per query              */
  int32_t* conn_weight;                  /* [conn_capacity]                                       */
  int32_t* ordered_start;                /* [n_queries+1]                                         */
  int32_t* ordered_kf;                   /* [ordered_capacity] descending (weight, slot) per query */
  int32_t* ordered_weight;               /* [ordered_capacity]                                    */
  int32_t* n_max;                        /* [n_queries]                                           */
  int32_t* kf_max;                       /* [n_queries] or -1                                     */
  uint8_t* updated;                      /* [n_queries] 0: the early return of :346-347           */
  int32_t* n_mps;                        /* [n_queries] culling                                   */
  int32_t* n_redundant;                  /* [n_queries] culling                                   */
  uint8_t* redundant;                    /* [n_queries] culling                                   */
  float*   phase_ms;                     /* [3] upload, kernels, download; may be NULL            */
} lld_covisibility_out;
int lld_covisibility(lld_ctx* ctx, const lld_covisibility_in* in, lld_covisibility_out* out);

/* ================================================================== the loop-closing thread moves the map (lld_map_correct.hip)
 * Three entry points for the three host loops that run with Map::mMutexMapUpdate held: LoopClosing::CorrectLoop
 * (src/LoopClosing.cc:440-518), the write-back of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1601-1653) and the map update
 * of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:678-739).  Each call makes one upload, queues its kernels on the
 * context's stream with no host trip between them, makes one download and waits for the stream.  Every index and every parent link
 * is range-checked on the host first: LLD_ERR_INVALID / LLD_ERR_UNSUPPORTED are returned before anything is queued and leave the
 * outputs untouched.
 * Conventions: keyframe tables are numbered by the caller in std::less<KeyFrame*> order; the observations of a point are a CSR in
 * std::map iteration order (as in lld_mappoint_refresh); a Sim3 is 8 doubles (rotation x, y, z, w, translation, scale); a float pose is
 * Tcw[12], the rows of [R|t].  Float matrix products are cv::gemm products as this header fixes them everywhere: every entry the
 * double sum of its terms in index order, rounded to float once.
 * SetPose rule (src/KeyFrame.cc:82-89): Rwc = Rcw^T, Ow = -Rwc*tcw (one product), Twc = [Rwc | Ow].
 * UpdateNormalAndDepth (src/MapPoint.cc:330-371) has the numerics of lld_mappoint_refresh, bit for bit; level_scale is one table for
 * all keyframes (the DEVIATION stated there).  It runs in kernels sized for whole maps: eight points with at most 8 observations share
 * a wavefront, longer lists take a wavefront each.
 *
 * (a) lld_loop_correct, CorrectLoop :440-518.
 *   conn[n_conn]: the keyframe slots of mvpCurrentConnectedKFs plus mpCurrentKF IN THE ITERATION ORDER OF CorrectedSim3 (a
 *   std::map<KeyFrame*, ...>, so ascending slot when the table is in pointer order); cur = the position of mpCurrentKF in it.  Per
 *   connected keyframe r, kf_point[kf_start[r] .. kf_start[r+1]) = the point slots of the non-NULL GetMapPointMatches() in keypoint
 *   order (a slot may repeat).  The keyframe table holds every keyframe that observes a listed point.
 *   :442      Twc = mpCurrentKF->GetPoseInverse() by the SetPose rule.
 *   :457-463  Tic = Tiw*Twc, a full 4x4 float product (the translation column is the four-term sum too); g2oSic = Sim3(Ric, tic, 1.0);
 *             CorrectedSiw = g2oSic*mg2oScw (Eigen's Quaterniond(Matrix3d) and Sim3::operator*, no normalisation: sim3.h:64-67, :266-272);
 *             for cur it is mg2oScw itself.  :466-470 NonCorrectedSiw = Sim3(Riw, tiw, 1.0).
 *   :474-503  Owner of a point = the first rank in conn whose list holds it, points that are bad or `already` (mnCorrectedByKF ==
 *             mpCurrentKF->mnId on entry) skipped.  Corrected position = CorrectedSwi.map(Siw.map(P)) of the owner: P widened to double,
 *             Sim3::inverse and Sim3::map, rounded to float once (Converter::toCvMat).  corrected_by = the owner's rank, or -1.
 *   :506-514  Corrected pose = toCvSE3(R(q), t*(1./s)) (a reciprocal, then a product), Ow by the SetPose rule.
 *   :502      UpdateNormalAndDepth of a point owned by rank k reads, for an observing keyframe and for the reference keyframe alike, the
 *             CORRECTED centre when that keyframe is in conn at a rank strictly below k, and the centre on entry otherwise (rank k itself:
 *             its SetPose follows its points; keyframes outside conn never move).  This is what the interleaved loop computes.  A point
 *             with no observations is moved, and its normal and depth are left alone (bit 1 of updated clear).
 *   scw_f32 = Converter::toCvMat(Sim3) = [sR | t] in float (Converter.cc:55-61), what SearchAndFuse takes.  MapLines are not touched:
 *   the reference does not touch them.  UpdateConnections (:517) stays the batched lld_covisibility call after this one.
 * (b) lld_essential_graph_apply, Optimizer.cc:1601-1653.  sim3_before = vScw and sim3_after = the optimised CorrectedSiw: the sim3 array
 *   lld_optimize_essential_graph takes and the one it returns.  corr_kf[p] = the slot the caller chose at :1631-1639
 *   (mnCorrectedReference or pRefKF).  :1611-1619 every keyframe gets Tiw = toCvSE3(R, t*(1./s)) and its Ow; :1645-1650 every point that
 *   is not bad gets after[r]^-1.map(before[r].map(P)), rounded once; :1652 UpdateNormalAndDepth with ALL centres new.
 * (c) lld_global_ba_apply, LoopClosing.cc:678-739, all float cv::Mat arithmetic.  parent[k] = the slot of GetParent(), -1 for none.
 *   :679-702  the walk from origins[] over the children: a child that is not kf_in_gba (mnBAGlobalForKF != nLoopKF on entry) gets
 *             mTcwGBA = (Tchild*Twc_parent)*mTcwGBA_parent - two 4x4 products, Twc_parent the parent's [Rcw^T | Ow] BEFORE its update,
 *             Tchild the child's pose before its update - and counts as visited.  Every visited keyframe reports tcw_before (its pose
 *             on entry) and takes tcw_new = mTcwGBA with the SetPose-rule Ow.  A child reads only its parent, so the order among
 *             siblings does not matter; chains of keyframes that are not kf_in_gba are composed top-down.
 *   :705-739  a point that is not bad: in_gba takes pos_gba (moved 1); otherwise, when its reference keyframe was visited,
 *             Xc = Rcw_before*P + tcw_before (the product rounded, then the float sum), P' = Rwc_new*Xc + Ow_new (moved 2); otherwise
 *             it is untouched (moved 0).  There is no UpdateNormalAndDepth here: the reference has none.
 *   LLD_ERR_INVALID besides the common cases: a parent out of range, its own parent or on a cycle; an origin out of range, repeated,
 *   with a parent, or not kf_in_gba (the walk would read an mTcwGBA that was never set); a kf_in_gba keyframe the walk does not reach
 *   (its points would read an unset mTcwBefGBA); a point that is neither bad nor in_gba with ref_kf out of range.
 * Limits: n_kf above LLD_MAPCORR_MAX_KF, n_points above LLD_MAPCORR_MAX_POINTS, n_entries above LLD_MAPCORR_MAX_ENTRIES or a point with more than LLD_LANDMARK_MAX_OBS
 *   observations returns LLD_ERR_UNSUPPORTED.  n_points = 0 and n_conn = 1 are valid; n_kf is at least 1.  LLD_ERR_INVALID: a NULL
 *   required pointer; negative sizes; a CSR (kf_start, obs_start) that does not start at 0, decreases or does not end at its count;
 *   a keyframe or point slot out of range; cur outside conn; a slot repeated in conn; n_levels outside [1, LLD_ORB_MAX_LEVELS]; ref_kf
 *   or ref_level outside its table for a point the rule does not skip; a non-finite pose or Sim3, or a scale that is not > 0.
 * Outputs are in / out: an entry the rule leaves alone keeps the value the caller passed in. */
#define LLD_MAPCORR_MAX_KF 65536           /* keyframes of one call                                 */
#define LLD_MAPCORR_MAX_POINTS (1 << 23)   /* map points of one call                                */
#define LLD_MAPCORR_MAX_ENTRIES (1 << 24)  /* (connected keyframe, point) entries of lld_loop_correct */
#define LLD_MAPCORR_MOVED 1u               /* updated bit 0: the position was corrected; bit 1 is LLD_LANDMARK_NORMAL_DEPTH */
typedef struct {                          /* the point table of (a) and (b)                        */
  int32_t n_points, n_obs, n_levels, reserved;
  const float*    pos;                   /* [n_points][3] mWorldPos                               */
  const uint8_t*  bad;                   /* [n_points] isBad()                                    */
  const int32_t*  obs_start;             /* [n_points+1]                                          */
  const int32_t*  obs_kf;                /* [n_obs] slot of the observing keyframe                */
  const int32_t*  ref_kf;                /* [n_points] mpRefKF                                    */
  const int32_t*  ref_level;             /* [n_points] as in lld_mappoint_refresh_in              */
  const float*    level_scale;           /* [n_levels] mvScaleFactors                             */
} lld_mapcorr_points;
typedef struct {
  int32_t n_kf, n_conn, cur, n_entries;
  const float*    kf_tcw;                /* [n_kf][12] GetPose()                                  */
  const int32_t*  conn;                  /* [n_conn] keyframe slots in CorrectedSim3's order      */
  const double*   scw;                   /* [8] mg2oScw                                           */
  const int32_t*  kf_start;              /* [n_conn+1]                                            */
  const int32_t*  kf_point;              /* [n_entries] point slots per connected keyframe        */
  const uint8_t*  already;               /* [n_points] mnCorrectedByKF == mpCurrentKF->mnId       */
  lld_mapcorr_points  points;
} lld_loop_correct_in;
typedef struct {
  double*  corrected_sim3;               /* [n_conn][8] CorrectedSim3                             */
  double*  non_corrected_sim3;           /* [n_conn][8] NonCorrectedSim3                          */
  float*   tiw_corrected;                /* [n_conn][12] the pose SetPose takes                   */
  float*   ow_corrected;                 /* [n_conn][3] its camera centre                         */
  float*   scw_f32;                      /* [n_conn][12] toCvMat(CorrectedSiw) = [sR | t]         */
  float*   pos;                          /* [n_points][3]                                         */
  int32_t* corrected_by;                 /* [n_points] the owner's rank in conn, or -1            */
  float*   normal;                       /* [n_points][3]                                         */
  float*   min_distance;                 /* [n_points]                                            */
  float*   max_distance;                 /* [n_points]                                            */
  uint8_t* updated;                      /* [n_points] bit 0 moved, bit 1 normal / depth          */
} lld_loop_correct_out;
int lld_loop_correct(lld_ctx* ctx, const lld_loop_correct_in* in, lld_loop_correct_out* out);
typedef struct {
  int32_t n_kf, reserved;
  const double*   sim3_before;           /* [n_kf][8] vScw                                        */
  const double*   sim3_after;            /* [n_kf][8] the optimised CorrectedSiw                  */
  const int32_t*  corr_kf;               /* [n_points] mnCorrectedReference or pRefKF (:1631-1639) */
  lld_mapcorr_points  points;
} lld_essential_graph_apply_in;
typedef struct {
  float*   tiw;                          /* [n_kf][12]                                            */
  float*   ow;                           /* [n_kf][3]                                             */
  float*   pos;                          /* [n_points][3]                                         */
  float*   normal;                       /* [n_points][3]                                         */
  float*   min_distance;                 /* [n_points]                                            */
  float*   max_distance;                 /* [n_points]                                            */
  uint8_t* updated;                      /* [n_points] bit 0 moved, bit 1 normal / depth          */
} lld_essential_graph_apply_out;
int lld_essential_graph_apply(lld_ctx* ctx, const lld_essential_graph_apply_in* in, lld_essential_graph_apply_out* out);
typedef struct {
  int32_t n_kf, n_origins, n_points, reserved;
  const float*    kf_tcw;                /* [n_kf][12] GetPose()                                  */
  const uint8_t*  kf_in_gba;             /* [n_kf] mnBAGlobalForKF == nLoopKF on entry            */
  const float*    kf_tcw_gba;            /* [n_kf][12] mTcwGBA, read where kf_in_gba is set       */
  const int32_t*  parent;                /* [n_kf] slot of GetParent(), -1 for none               */
  const int32_t*  origins;               /* [n_origins] Map::mvpKeyFrameOrigins                   */
  const float*    pos;                   /* [n_points][3]                                         */
  const uint8_t*  bad;                   /* [n_points]                                            */
  const uint8_t*  in_gba;                /* [n_points] mnBAGlobalForKF == nLoopKF                 */
  const float*    pos_gba;               /* [n_points][3] mPosGBA, read where in_gba is set       */
  const int32_t*  ref_kf;                /* [n_points]                                            */
} lld_global_ba_apply_in;
typedef struct {
  uint8_t* visited;                      /* [n_kf] always written                                 */
  float*   tcw_new;                      /* [n_kf][12] mTcwGBA of a visited keyframe              */
  float*   tcw_before;                   /* [n_kf][12] mTcwBefGBA of a visited keyframe           */
  float*   ow_new;                       /* [n_kf][3]                                             */
  float*   pos;                          /* [n_points][3]                                         */
  uint8_t* moved;                        /* [n_points] 0 untouched, 1 pos_gba, 2 through ref_kf   */
} lld_global_ba_apply_out;
int lld_global_ba_apply(lld_ctx* ctx, const lld_global_ba_apply_in* in, lld_global_ba_apply_out* out);

/* ------------------------------------------------------------------ the resident map: Tracking::UpdateLocalMap between the tracking stages
 * Between its stage 1 (TrackWithMotionModel / TrackReferenceKeyFrame / Relocalization) and TrackLocalMap the reference runs
 * Tracking::UpdateLocalMap (src/Tracking.cc:1667-1835): the MapPoints stage 1 matched vote for the keyframes that observe them, the voted
 * keyframes and some of their neighbours, children and parents become mvpLocalKeyFrames, and the MapPoints / MapLines of those keyframes
 * become stage 2's input.  With the map on the host that is a download, a walk over std::maps, a gather of thousands of objects into arrays
 * and an upload, every frame.  An lld_map keeps what that walk reads as flat tables in HBM, so that the routine is a handful of kernels queued
 * between the two stages and stage 2 gathers its input from the tables by slot: one upload (stage 1's inputs) and one download per frame.
 *
 * Slots are caller-chosen dense integers, 0 <= slot < max_*.  On this route the ids the frame chain carries (last_point_id, kp_point_id,
 * the ids of lld_map_lines, what lld_frame_track_finish numbers) ARE point / line slots.  A point id outside [0, max_points), or a slot
 * lld_map_set_points never set, names a MapPoint the map does not hold - a temporal point of UpdateLastFrame (:840-883): it votes for
 * nothing and is not bad.  A keyframe or line slot never set counts as bad.
 * The handle belongs to one context and one host thread, like lld_frame. */
typedef struct lld_map lld_map;
typedef struct {
  int32_t max_keyframes;            /* <= 262144                                                                                                       */
  int32_t max_points, max_lines;
  int32_t line_dim;                 /* <= 128; a frame with lines must have the same dim                                                             */
  /* the most LIVE list entries, summed over all rows (the library reserves twice as much, so that rows can be replaced in any order) */
  int32_t max_observations;         /* MapPoint::mObservations                                                                                        */
  int32_t max_kf_points;            /* KeyFrame::mvpMapPoints (one entry per keypoint, -1 included)                                                  */
  int32_t max_kf_lines;             /* KeyFrame::mvpMapLines                                                                                          */
  int32_t max_children;             /* KeyFrame::mspChildrens                                                                                         */
  int32_t max_local_points;         /* mvpLocalMapPoints: also the number of queries stage 2 is sized for                                             */
  int32_t max_local_lines;          /* local_lines                                                                                                    */
} lld_map_limits;
int  lld_map_create(lld_ctx* ctx, const lld_map_limits* limits, lld_map** out);
void lld_map_destroy(lld_map* map);   /* waits for the context's stream */
int  lld_map_clear(lld_map* map);     /* Map::clear(): every slot never set, every list empty, no local map */
/* Updates.  Each replaces whole rows by slot from flat host arrays: one upload, queued on the context's stream, ordered before any later
 * track call; a row may be replaced any number of times, and no replacement fails while the live totals stay inside the limits.
 * Refused before anything is queued, the map unchanged: LLD_ERR_INVALID for a NULL map or required array, n < 0, a slot out of range or
 * named twice in one call, a referenced slot out of range, a start array that does not ascend from 0, order_key = UINT64_MAX;
 * LLD_ERR_UNSUPPORTED for a live total beyond its limit.  n = 0 is LLD_OK.  Uniqueness of order_key among live keyframes is NOT checked: with
 * two equal keys the order of those keyframes, and so the lists, are undefined (nothing is refused, nothing is read out of bounds).
 * A HIP failure (LLD_ERR_HIP / LLD_ERR_ALLOC) may arrive after a call's host bookkeeping moved: the map is then unusable - every later
 * lld_map_set_* and track call on it returns LLD_ERR_HIP - until lld_map_clear, after which it is filled again.
 *   lld_map_set_points        GetWorldPos, GetNormal, GetMinDistanceInvariance / GetMaxDistanceInvariance AS lld_map_points takes them, GetDescriptor, isBad
 *   lld_map_set_observations  mObservations of point slot[i] = kf_slot[start[i] .. start[i+1]); Observations() > 0 is "list not empty"
 *   lld_map_set_keyframes     order_key: the keyframe's position in std::map<KeyFrame*,int> / std::set<KeyFrame*> iteration - the pointer value,
 *                             or mnId for runs that repeat; unique among live keyframes.  parent: GetParent() or -1.  CSR lists per keyframe:
 *                             cov = GetBestCovisibilityKeyFrames(10) in its order (entries beyond 10 are ignored), child = GetChilds() in any order,
 *                             point = GetMapPointMatches() per keypoint (slot or -1), line = GetMapLineMatches() (slot or -1)
 *   lld_map_set_lines         GetMinimalPos (x0, dir), GetMainPoints3D (x1, x2), GetDescriptor [line_dim], isBad */
int  lld_map_set_points(lld_map* map, int32_t n, const int32_t* slot, const float* world_pos, const float* normal, const float* min_distance,
                        const float* max_distance, const uint32_t* desc, const uint8_t* bad);
int  lld_map_set_observations(lld_map* map, int32_t n, const int32_t* slot, const int32_t* start, const int32_t* kf_slot);
int  lld_map_set_keyframes(lld_map* map, int32_t n, const int32_t* slot, const uint64_t* order_key, const uint8_t* bad, const int32_t* parent,
                           const int32_t* cov_start, const int32_t* cov, const int32_t* child_start, const int32_t* child,
                           const int32_t* point_start, const int32_t* point, const int32_t* line_start, const int32_t* line);
int  lld_map_set_lines(lld_map* map, int32_t n, const int32_t* slot, const double* x0, const double* dir, const double* x1, const double* x2,
                       const float* desc, const uint8_t* bad);
/* Tracking::UpdateLocalMap on the frame's device state, queued behind whatever produced it (lld_frame_track_motion_model,
 * _reference_keyframe, lld_frame_relocalize or lld_frame_track_set_state): no upload, no synchronisation.  :1726-1835 and :1677-1723, quirks included:
 *   vote (:1730-1746)       a keypoint whose MapPoint is bad loses it (mvbOutlier stays); every observation of the others is one vote.
 *   empty vote (:1748)      the routine returns: the list of the previous call (it lives in the lld_map) and the reference keyframe stay,
 *                           UpdateLocalPoints still runs on that list with today's bad flags.
 *   voted (:1758-1774)      in ascending order_key; bad ones are neither listed nor marked nor candidates for pKFmax, which is the first
 *                           keyframe in that order with the strictly greatest count.
 *   extension (:1778-1828)  over the voted entries only; it stops before an entry when the list holds more than 80; per entry the first of its
 *                           cov list that is neither bad nor marked, the child of smallest order_key that is neither bad nor marked, and
 *                           the parent if unmarked (its bad flag is not read) - and appending a parent ends the WHOLE loop (:1824).
 *   points, lines (:1684-1722)  list order, then keypoint order; every non-bad one once.
 * Never a silently shortened local map: more than 1024 voted keyframes, more than max_local_points points or max_local_lines lines set the
 * status bits below, and lld_frame_track_local_map_resident then leaves the frame as it found it. */
#define LLD_LOCAL_MAP_KEYFRAME_OVERFLOW 1
#define LLD_LOCAL_MAP_POINT_OVERFLOW    2
#define LLD_LOCAL_MAP_LINE_OVERFLOW     4
#define LLD_MAP_MAX_LOCAL_KEYFRAMES  1280   /* 1024 voted, or at most 81 visited entries x 3 behind at most 81 */
int  lld_frame_track_update_local_map(lld_frame* frame, lld_map* map);
/* Stage 2 (lld_frame_track_local_map) on the lists the last lld_frame_track_update_local_map left: a kernel copies the listed rows into the
 * buffers lld_frame_track_local_map stages from the host (has_obs = observations not empty, id = slot), and the same kernels follow, sized
 * by max_local_points / max_local_lines; the entries behind the device-side counts are skipped entries.  Only the search's problem record
 * is uploaded.  After an overflow the decision is taken on the device: every entry is a skipped entry and the frame's MapPoint / MapLine
 * tables are set aside while the stage's kernels run and put back behind them, so the frame is left as stage 1 and the vote left it; the
 * stage-2 record then reads all zero and lld_local_map_result.stage2_ran is 0.  lld_frame_track_finish and lld_frame_new_map_lines follow as
 * after lld_frame_track_local_map.  LLD_ERR_INVALID before anything is queued: a NULL argument, a map of another context, no stage 1 on the
 * frame, no lld_frame_track_update_local_map on this frame and this map since that stage 1, or another
 * frame's update on the map since (the lists in the map are the last update's: frames share a map one after the other), a frame with lines whose dim differs from the map's line_dim. */
int  lld_frame_track_local_map_resident(lld_frame* frame, const lld_track_params* params, lld_map* map);
typedef struct {
  int32_t status;                   /* 0, or LLD_LOCAL_MAP_*_OVERFLOW bits                                                                            */
  int32_t n_voted;                  /* keyframeCounter.size()                                                                                         */
  int32_t n_local_keyframes, n_local_points, n_local_lines;   /* a count beyond its limit is the true count; its list was not written                */
  int32_t n_bad_cleared;            /* keypoints that lost a bad MapPoint (:1743)                                                                    */
  int32_t ref_keyframe;             /* slot of pKFmax -> mpReferenceKF, or -1: unchanged                                                              */
  int32_t vote_empty;               /* 1: the routine returned at :1748                                                                               */
  int32_t stage2_ran;               /* 1 after lld_frame_track_local_map_resident on a local map without overflow                                     */
  int32_t reserved;
  /* caller-allocated, any may be NULL */
  int32_t* local_keyframes;         /* [LLD_MAP_MAX_LOCAL_KEYFRAMES] mvpLocalKeyFrames as slots                                                       */
  int32_t* local_points;            /* [max_local_points] mvpLocalMapPoints                                                                           */
  int32_t* local_lines;             /* [max_local_lines]                                                                                              */
  uint8_t* mp_in_view;              /* [max_local_points] with stage2: lld_track_result.mp_in_view per local point (stage2->mp_in_view is not read); left
                                       alone when the frame's last stage 2 was lld_frame_track_local_map on more points than that                        */
  lld_track_result* stage1;         /* as lld_frame_track_download fills them, in the same synchronisation                                            */
  lld_track_result* stage2;
} lld_local_map_result;
int  lld_frame_local_map_download(lld_frame* frame, lld_map* map, lld_local_map_result* out);

/* ------------------------------------------------------------------ covisibility on the resident map (lld_map_covis.hip)
 * KeyFrame::UpdateConnections (src/KeyFrame.cc:312-402) and the redundancy count of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:646-694)
 * for a batch of keyframes, counted on the tables the map already holds: nothing of the map is gathered or uploaded, only the list of
 * query slots travels.  The rules are those of lld_covisibility above, restated on the map's tables; every result is an integer.
 *
 * Tables the culling part needs beyond lld_map_set_*.  They live in pools of their own (sized from max_observations and max_kf_points, twice
 * the limit like the others) that are allocated by the first call of one of the first two setters below - a map on which they are never
 * called allocates what it allocated before.  The setters follow the contract of lld_map_set_*: everything is validated first, a refusal
 * changes nothing, one block and one copy, a HIP failure behind the host bookkeeping poisons the map, lld_map_clear empties the new pools too.
 *   lld_map_set_observations_indexed  lld_map_set_observations, and with each observation kp_index = mObservations[pKF], the keypoint index
 *                             in the observing keyframe (>= 0), and per point n_obs[i] = MapPoint::Observations(), the stereo-weighted nObs
 *                             (>= 0), which is not the list length.  A row set through lld_map_set_observations carries no indices (an
 *                             earlier index row of that point is dropped) and keeps its n_obs.
 *   lld_map_set_keyframe_keypoints    per keyframe slot[i]: octave[start[i] .. start[i+1]) = mvKeysUn[k].octave, depth[..] = mvDepth[k] (a float
 *                             travels as its bit pattern), th_depth[i] = mThDepth.  LLD_ERR_INVALID also for a keyframe lld_map_set_keyframes
 *                             never set and for a row whose length differs from the keyframe's point row.  A point row replaced later by one
 *                             of another length leaves the keypoint row stale: the culling part says so (below) until the keypoints follow.
 *   lld_map_set_covisibles    replaces only the cov row (GetBestCovisibilityKeyFrames(10), entries beyond 10 are ignored) of keyframes that are
 *                             already set - for the neighbours on which UpdateConnections calls AddConnection (KeyFrame.cc:367, :374); key,
 *                             bad flag, parent and the point, line and child rows stay.  LLD_ERR_INVALID also for a keyframe never set.  It
 *                             allocates nothing. */
int  lld_map_set_observations_indexed(lld_map* map, int32_t n, const int32_t* slot, const int32_t* start, const int32_t* kf_slot,
                                      const int32_t* kp_index, const int32_t* n_obs);
int  lld_map_set_keyframe_keypoints(lld_map* map, int32_t n, const int32_t* slot, const int32_t* start, const int32_t* octave, const float* depth,
                                    const float* th_depth);
int  lld_map_set_covisibles(lld_map* map, int32_t n, const int32_t* slot, const int32_t* cov_start, const int32_t* cov);
/* What Tracking::UpdateLocalMap reads of a keyframe besides its points, read back from the device tables - for a caller that audits its
 * mirror (examples/map_covis_harness.cpp) and for the tests: parent[i] (slot or -1), n_cov[i] and cov[10 i ..] (the row as the device holds
 * it, written by lld_map_set_keyframes, lld_map_set_covisibles or LLD_MAP_COVIS_WRITE_COV; entries behind n_cov[i] are -1), and the child
 * rows as CSR: child_start [n + 1] is always written, child [child_capacity] only if the total fits - otherwise the call returns
 * LLD_ERR_INVALID with child_start alone written (child may be NULL with a capacity of 0).  One small upload, one kernel, one download, one
 * wait; cost follows n.  LLD_ERR_INVALID also for a NULL argument, n < 0, a slot out of range or never set; n = 0 is LLD_OK. */
int  lld_map_download_links(lld_map* map, int32_t n, const int32_t* slot, int32_t* parent, int32_t* n_cov, int32_t* cov, int32_t* child_start,
                            int32_t child_capacity, int32_t* child);
/* The call.  One upload (the query slots), kernels queued on the context's stream with no host trip between them, one download, one wait.
 * Every keyframe in the outputs is a SLOT.  "Map order" is ascending order_key, NOT slot order: order_key decides every tie.
 * Connections (LLD_COVIS_CONNECTIONS), per query kf_slot[q] (a slot may repeat; each listing is counted on its own):
 *   :329-333 the query walks its own point row (lld_map_set_keyframes); an entry -1, a bad point and a point slot lld_map_set_points never
 *            set (its row is empty) are skipped.
 *   :335-342 every observation of the others whose keyframe slot differs from the query's is one count for that slot; a point listed twice
 *            counts twice.  The observers' bad flags are not read (the reference does not read them).
 *   :346-347 an empty counter: updated[q] = 0, no entries of either list, n_max[q] = 0, kf_max[q] = -1.
 *   :390     conn_kf / conn_weight: every counted keyframe in ascending order_key.
 *   :359-363 kf_max[q]: the first keyframe in that order with the strictly greatest count, n_max[q] its count.
 *   :364-375 the counts >= th, or if there is none the single pair (n_max, kf_max).
 *   :377-384 ordered_kf / ordered_weight: by descending weight, equal weights by descending order_key.
 *   AddConnection on the neighbours and the first-connection parent belong to the caller (adapters/lld_map_adapter.cc).
 *   With LLD_MAP_COVIS_WRITE_COV (valid only together with LLD_COVIS_CONNECTIONS) a query with updated = 1 and status 0 also gets the first
 *   min(10, n) entries of its ordered list written into its cov row - GetBestCovisibilityKeyFrames(10) - on the stream, before any later
 *   lld_frame_track_update_local_map; every other query's row is left alone.
 * Culling (LLD_COVIS_CULLING), per query, over the same point row with the keyframe's keypoint row beside it:
 *   :655-657 an entry -1 and a bad point are skipped.  A point slot never set is not bad and has Observations() == 0.
 *   :659-663 unless `monocular`, an entry with depth > th_depth || depth < 0 is skipped (float compares; depth == th_depth is kept).
 *   :665     n_mps++.
 *   :666-688 only if the point's n_obs > th_obs: count its observations whose slot differs from the query's and whose octave - the observing
 *            keyframe's keypoint row at the stored index - is <= the entry's octave + 1; count >= th_obs: n_redundant++.
 *   :694     redundant[q] = (n_redundant > redundant_ratio * n_mps), the int against the double product.
 *   The mnId == 0 skip and SetBadFlag stay with the caller, who updates the rows a flagged keyframe changed and calls again for the rest.
 * Never a silently wrong answer - status[q], per query, and a bit of one query changes nothing for the others in the call:
 *   LLD_MAP_COVIS_CONN_OVERFLOW      more than LLD_MAP_COVIS_MAX_CONNECTED distinct covisible keyframes: the query's connection outputs are
 *                                    empty (no entries, n_max 0, kf_max -1), updated = 0, its cov row untouched.
 *   LLD_MAP_COVIS_NO_KEYPOINT_DATA   culling only: the query keyframe has no keypoint row of its point row's length, or the observation row
 *                                    of a point counted in n_mps has no index row of its length (it came through lld_map_set_observations,
 *                                    so its n_obs is not known either), or an index falls outside the observing keyframe's keypoint row.
 *                                    n_mps, n_redundant and redundant of the query are 0.  The device decides this from the row lengths
 *                                    before it reads; no read leaves a row.
 * Capacities as lld_covisibility: the totals needed are always written to lists.n_conn / lists.n_ordered; if either capacity is short the call
 * returns LLD_ERR_INVALID with only those two written (n_queries * LLD_MAP_COVIS_MAX_CONNECTED always suffices; the cov rows of
 * LLD_MAP_COVIS_WRITE_COV are written by that call all the same, and the repeated call writes the same rows again).  Arrays of a part not
 * selected are neither read nor written and may be NULL; status is always required; lists.phase_ms may be NULL, otherwise it receives the
 * HIP-event times of the upload of the query list, the kernels and the download.
 * LLD_ERR_INVALID before anything is queued: a NULL map, in, out, kf_slot, status or required output; n_queries < 0; a negative capacity;
 * flags zero, with unknown bits, or LLD_MAP_COVIS_WRITE_COV without LLD_COVIS_CONNECTIONS; a query slot out of range or never set.
 * LLD_ERR_HIP for a poisoned map, like every other call on it.  n_queries = 0 is LLD_OK and touches nothing. */
#define LLD_MAP_COVIS_MAX_CONNECTED    4096   /* distinct covisible keyframes of one query: half the 8192 cells of the counting table in LDS */
#define LLD_MAP_COVIS_WRITE_COV        4u     /* flags bit 2, beside LLD_COVIS_CONNECTIONS / LLD_COVIS_CULLING                              */
#define LLD_MAP_COVIS_CONN_OVERFLOW    1      /* status bits                                                                                */
#define LLD_MAP_COVIS_NO_KEYPOINT_DATA 2
typedef struct {
  int32_t n_queries;
  int32_t monocular;                /* mbMonocular: no depth test in the culling part */
  uint32_t flags;
  int32_t reserved;
  lld_covisibility_params params;
  const int32_t* kf_slot;           /* [n_queries] */
} lld_map_covisibility_in;
typedef struct {
  lld_covisibility_out lists;       /* the arrays and the capacity protocol of lld_covisibility; keyframes are slots */
  uint8_t* status;                  /* [n_queries] 0, or LLD_MAP_COVIS_CONN_OVERFLOW / LLD_MAP_COVIS_NO_KEYPOINT_DATA bits */
} lld_map_covisibility_out;
int  lld_map_covisibility(lld_map* map, const lld_map_covisibility_in* in, lld_map_covisibility_out* out);

/* ------------------------------------------------------------------ the local BA window from the resident map (lld_map_ba.hip)
 * The first third of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:938-1018 and the edge loops :1093-1218): local keyframes, local
 * points and lines, fixed cameras, and every observation flattened into a lld_ba_window - assembled on the map's tables.  Only the list
 * of local keyframe slots travels up; the window arrives in the layout lld_local_ba takes.
 *
 * Tables beyond the ones above, in pools of their own that the first of these three setters allocates (a map on which they are never
 * called allocates what it allocated before).  The contract is that of the other setters: everything is validated first, a refusal
 * changes nothing, one block and one copy per call, a HIP failure behind the host bookkeeping poisons the map, lld_map_clear empties them.
 *   lld_map_set_keyframe_features  per keyframe slot[i] (lld_map_set_keyframes must have set it): mn_id[i] = KeyFrame::mnId; Tcw [16 i ..] =
 *                             GetPose() row-major, stored as lld_se3_from_tcw_f32 of it (7 doubles, computed on the host); per keypoint
 *                             kp_uvr [3 k ..] = mvKeysUn[k].pt.x, .pt.y, mvuRight[k] - kp_start[i + 1] - kp_start[i] must equal the length
 *                             of the keyframe's point row; per left keyline kl_left [4 k ..] = startPointX, startPointY, endPointX,
 *                             endPointY, kl_right [4 k ..] the same of mvLinesRight[line_matches[k]] or four times -1.0f when
 *                             line_matches[k] < 0, kl_octave [2 k ..] = left octave, right octave (0 without a partner) - kl_start[i + 1] -
 *                             kl_start[i] must equal the length of the keyframe's line row.  Floats stay floats and are widened on the
 *                             device.  Keypoint octaves are those of lld_map_set_keyframe_keypoints.
 *   lld_map_set_keyframe_poses     Tcw alone, for keyframes that already have features (LLD_ERR_INVALID otherwise).
 *   lld_map_set_line_observations  per line slot[i]: kf_slot / line_index [start[i] .. start[i+1]) = MapLine::mObservations in
 *                             std::map<KeyFrame*, size_t> iteration order, n_obs[i] = MapLine::Observations() (stereo-weighted, not the
 *                             row length).  The live total of line observations is bounded by max_kf_lines (an observation is an entry of
 *                             a keyframe's line row).
 * LLD_ERR_UNSUPPORTED from the first setter when max_kf_points > 2^28 or max_kf_lines > 2^26 (the pools' offsets are int32). */
int  lld_map_set_keyframe_features(lld_map* map, int32_t n, const int32_t* slot, const uint64_t* mn_id, const float* Tcw, const int32_t* kp_start,
                                   const float* kp_uvr, const int32_t* kl_start, const float* kl_left, const float* kl_right, const int32_t* kl_octave);
int  lld_map_set_keyframe_poses(lld_map* map, int32_t n, const int32_t* slot, const float* Tcw);
int  lld_map_set_line_observations(lld_map* map, int32_t n, const int32_t* slot, const int32_t* start, const int32_t* kf_slot,
                                   const int32_t* line_index, const int32_t* n_obs);
/* The call.  One upload (the slot list and the level table), kernels on the context's stream with no host trip between them, one download,
 * one wait.  kf_slot[0] = pKF, kf_slot[1 .. n) = pKF->GetVectorCovisibleKeyFrames() in its order.  Rules, quirks included:
 *   :940-950   kf_slot[0] is a local keyframe whatever its bad flag; a bad neighbour is marked local but not listed (so it is never a fixed
 *              camera either).
 *   :955-984   local points in list order, then keypoint order: entries -1, bad points and point slots never set are skipped, the first
 *              occurrence counts.  Local lines likewise; a line slot never set is bad, and a line with n_obs < 4 is skipped without being marked.
 *   :990-1018  fixed cameras: the local points in list order, each observation row in stored order, then the lines the same way; an observer
 *              that is neither marked local nor marked fixed yet is marked fixed, and listed if it is not bad.
 *   cameras    the listed local keyframes with mn_id != 0 by ascending mn_id (n_free_cams of them), the listed local keyframes with
 *              mn_id == 0, then the fixed cameras in first-marked order.  [0, n_local_cams) are the local ones.  Uniqueness of mn_id is not
 *              checked: with equal ids the order of those is undefined, nothing is read out of bounds.
 *   :1093-1178 a point's run: its observations in stored order without the bad observers; u, v, uR widened from the observer's keypoint row
 *              at the stored index, inv_sigma2 = (double)inv_level_sigma2[octave of that keypoint].  A point whose run is empty stays.
 *   :1185-1218 a line's run: its non-bad observers in ascending mn_id, left and right end points widened, both octaves.
 *   pt_xyz is the widened float position; line_x0 / line_dir are the stored doubles.
 * Capacities: the seven counts are always written; if any capacity is short the call returns LLD_ERR_INVALID with only the counts (and
 * status = 0) written.  Arrays whose capacity is 0 may be NULL, except pt_obs_start and ln_obs_start (capacity + 1 entries each).
 * Never a silently wrong window - status, LLD_OK returned: LLD_MAP_BA_NO_FEATURE_DATA when a camera of the window has no feature rows
 * (lld_map_set_keyframe_features, lld_map_set_keyframe_keypoints) of its point and line rows' lengths, a local point's observation row has
 * no index row of its length, a local line that is not bad has no observation row, or a stored index falls outside the observer's row - or
 * an octave outside [0, n_levels).  The device decides this from the row lengths before it reads.  The counts are then 0 and no array is
 * written.
 * LLD_ERR_INVALID before anything is queued: a NULL argument; n_keyframes < 1 or > LLD_MAP_BA_MAX_LOCAL; a slot out of range, never set or
 * named twice; n_levels < 1 or a NULL level table; a negative capacity; a NULL array with a capacity above 0.  LLD_ERR_HIP for a poisoned map. */
#define LLD_MAP_BA_MAX_LOCAL        1024
#define LLD_MAP_BA_NO_FEATURE_DATA  1
typedef struct {
  int32_t n_keyframes;
  int32_t n_levels;
  const int32_t* kf_slot;           /* [n_keyframes]                                   */
  const float* inv_level_sigma2;    /* [n_levels] mvInvLevelSigma2                     */
  lld_camera cam;                   /* copied into the window: pKF's fx, fy, cx, cy, mbf */
} lld_map_ba_in;
typedef struct {
  int32_t cam_capacity, point_capacity, pt_obs_capacity, line_capacity, ln_obs_capacity;
  int32_t n_cams, n_free_cams, n_local_cams, n_points, n_pt_obs, n_lines, n_ln_obs;      /* always written */
  int32_t status;
  int32_t*  cam_slot;               /* [n_cams]                                         */
  double*   cam_qt;                 /* [n_cams][7]                                      */
  int32_t*  point_slot;             /* [n_points]                                       */
  double*   pt_xyz;                 /* [n_points][3]                                    */
  int32_t*  pt_obs_start;           /* [n_points + 1] (capacity + 1 entries are needed) */
  int32_t*  pt_obs_cam;             /* [n_pt_obs]                                       */
  double*   pt_obs_uvr;             /* [n_pt_obs][3]                                    */
  double*   pt_obs_inv_sigma2;      /* [n_pt_obs]                                       */
  int32_t*  line_slot;              /* [n_lines]                                        */
  double*   line_x0;                /* [n_lines][3]                                     */
  double*   line_dir;               /* [n_lines][3]                                     */
  int32_t*  ln_obs_start;           /* [n_lines + 1]                                    */
  int32_t*  ln_obs_cam;             /* [n_ln_obs]                                       */
  double*   ln_obs_left;            /* [n_ln_obs][4]                                    */
  double*   ln_obs_right;           /* [n_ln_obs][4]                                    */
  int32_t*  ln_obs_octave;          /* [n_ln_obs][2]                                    */
  float*    phase_ms;               /* NULL, or [3]: HIP-event times of upload, kernels, download */
} lld_map_ba_window_out;
int  lld_map_ba_window(lld_map* map, const lld_map_ba_in* in, lld_map_ba_window_out* out);
/* lld_map_ba_window into pinned buffers the map owns (grown on demand: a call that finds them short repeats the assembly once), then
 * lld_local_ba_stopflag on that window.  The map's tables are not changed (lld_map_ba_apply, below, does that).  Every pointer of `result` and `ids` is SET by the call and
 * points into memory of the map, valid until the next lld_map_local_ba or lld_map_destroy on it; ids->window is the window that was solved.
 * With ids->status != 0 nothing was solved and the counts are 0.  params = NULL: lld_ba_params_default; stop_flag may be NULL. */
typedef struct {
  int32_t status;                   /* 0 or LLD_MAP_BA_NO_FEATURE_DATA                  */
  int32_t n_local_cams;             /* cameras [0, n_local_cams) are the local keyframes: the adapter writes a pose back for each */
  const int32_t* cam_slot;          /* [window.n_cams]                                  */
  const int32_t* point_slot;        /* [window.n_points]                                */
  const int32_t* line_slot;         /* [window.n_lines]                                 */
  int32_t n_marked_bad;             /* keyframe slots the walk marks fixed (mnBAFixedForKF) although they are bad or were never set: */
  int32_t reserved;                 /* no cameras, in no order - for a caller that mirrors the reference's visit marks               */
  const int32_t* marked_bad_slot;   /* [n_marked_bad]                                   */
  lld_ba_window window;
} lld_map_ba_ids;
int  lld_map_local_ba(lld_map* map, const lld_map_ba_in* in, const lld_ba_params* params, volatile const unsigned char* stop_flag,
                      lld_ba_result* result, lld_map_ba_ids* ids);

/* ------------------------------------------------------------------ a local BA's result applied to the resident map (lld_map_apply.hip)
 * The last third of Optimizer::LocalBundleAdjustment, the part under mMutexMapUpdate (src/Optimizer.cc:1334-1386): the outlier
 * observations are erased, the local keyframes get their poses, every local point its position and UpdateNormalAndDepth, every line its
 * minimal position - on the map's tables, by the device.  It is the first call that lets the device change rows of the map; the host's
 * bookkeeping of the rows (lengths, live totals, the copy a repack is made from) follows every change, so the setters, the limits and
 * lld_map_covisibility go on as if the caller had sent the changed rows itself.
 *
 * Two tables beyond the ones above:
 *   lld_map_set_point_refs    MapPoint::mpRefKF of point slot[i] as a keyframe slot, or -1: unknown.  A pool of its own that the first call
 *                             allocates (every slot then -1).  The contract is that of the other setters: everything is validated first
 *                             (LLD_ERR_INVALID for a NULL array, n < 0, a slot out of range or named twice, a ref_kf outside
 *                             [-1, max_keyframes)), a refusal changes nothing, one block and one copy per call, lld_map_clear sets every
 *                             slot to -1 again.
 *   the camera centre         lld_map_set_keyframe_features and lld_map_set_keyframe_poses also store KeyFrame::SetPose's Ow of the float
 *                             Tcw they are given (float[3] per keyframe, computed on the host: -Rcw^T tcw, each entry one three-term sum in
 *                             double rounded once - the arithmetic of lld_loop_correct's centres).
 *
 * lld_map_ba_apply applies a result to THE WINDOW THIS MAP ASSEMBLED LAST (lld_map_ba_window or lld_map_local_ba): that window's index
 * arrays (point_slot, pt_obs_start, pt_obs_cam, cam_slot and the line twins) are still in the map's device staging, only the result
 * travels up.  The result is the caller's to pass (the arrays of lld_ba_result); the "returned before optimising" exit (:1220-1222) is the
 * caller's too - it does not call.  The map counts its mutations (every lld_map_set_* that is not refused, lld_map_clear,
 * LLD_MAP_COVIS_WRITE_COV and an apply itself).  LLD_ERR_INVALID before anything is queued, nothing changed: a NULL argument or array
 * (phase_ms may be NULL; arrays of a count of 0 may be NULL); n_levels < 1; no complete window is staged (the last assembly had a status
 * other than 0 or a short capacity, or there was none); the map changed since that window was assembled - so a second apply of one
 * window is refused too; n_cams, n_points, n_pt_obs, n_lines or n_ln_obs differ from that window's.  LLD_ERR_HIP for a poisoned map.
 * One upload, kernels on the context's stream with no host trip between them, one download, one wait; no allocation per call (the
 * staging grows only).  A HIP failure behind the first launch poisons the map.
 *
 * Cameras  [0, n_local_cams) of the window, the mn_id == 0 one included: T = lld_se3_to_tcw_f32(cam_qt[c]) on the host (out->tcw), the
 *          stored pose lld_se3_from_tcw_f32(T), the centre of T (out->ow is read back from the table).
 * Points   Every window point on its own.  Its erase list: its window observations with pt_obs_outlier = 1, the ones at a keypoint with
 *          uR < 0 (the mono edges) first, then the others, each in window order - the reference's order (:1282-1310).
 *          One erasure (MapPoint.cc:111-137, KeyFrame::EraseMapPointMatch before it): the observer cam_slot[pt_obs_cam[e]] is looked up in the
 *          stored row; the observer's point-row entry at the stored keypoint index is set to -1 whatever it holds; n_obs drops by 2 if
 *          uR >= 0 at that keypoint (a float compare on the stored bits), else by 1; the entry leaves the observation row and the index row
 *          (the order of the rest and the row's place are kept).  n_obs <= 2 after an erasure: the point goes bad (SetBadFlag, :151-168) -
 *          state isBad, EVERY remaining observer's point-row entry at its stored index set to -1 (by index, the observer is not looked
 *          at), both rows empty; the erasures behind that one do nothing, so n_obs stays where it went bad.
 *          A stored index outside the observer's point row (a bad or never-set observer met by the cascade; never a window camera) is
 *          not written: counted in n_index_skipped, flagged on the point.
 *          mpRefKF: of a surviving point whose reference keyframe was erased, the first entry of the final row (mObservations.begin()).
 *          Of a point that went bad the table gets -1; the reference leaves whatever begin() was at the erasure that took mpRefKF,
 *          a value that depends on its erase order.  Without lld_map_set_point_refs every reference is -1 and none is written.
 *          Position: p_pos = (float)pt_xyz for every window point, bad ones included (SetWorldPos does not look).
 *          UpdateNormalAndDepth (:330-371) for every window point that is not bad and whose row is not empty, with the numerics of
 *          lld_mappoint_refresh: the terms in row order, the centres from the table (the local cameras' are the new ones), the level =
 *          the octave of the reference keyframe's keypoint at the point's stored index there - keypoint 0 when the reference keyframe is
 *          no observer (observations[pRefKF] default-inserts 0); the reference keyframe's bad flag is not read.  Nothing is refreshed
 *          (normal and distances stay, LLD_MAP_APPLY_NO_REFERENCE) when the reference is -1, has no keypoint row reaching that index or
 *          no centre, when an observer has no centre, or when the octave is outside [0, n_levels).
 * Lines    A line with line_removed = 1 is skipped whole (:1320-1323).  Of the others an observation is erased when either of its two
 *          ln_edge_outlier flags is set, in window order (ascending mn_id).  One erasure (MapLine.cc:77-104): the observer's line-row
 *          entry at the stored keyline index set to -1; n_obs drops by 2 if that keyline's stored right end points are not four times
 *          -1.0f, else by 1; the entry leaves l_obs / l_idx.  n_obs <= 4: the line goes bad - and MapLine::SetBadFlag clears
 *          mObservations BEFORE it calls EraseMapLineMatch(this), which then finds no index: the remaining observers' line-row entries
 *          are NOT cleared, only the row is emptied and the line marked bad; later erasures of that line do nothing.  l_x0 / l_dir take
 *          the result for every line that was not removed; l_x1 / l_x2 stay.
 * Outputs  are read from the tables behind the writes, per window point and per window line, in window order. */
#define LLD_MAP_APPLY_WENT_BAD       1   /* pt_flags bits */
#define LLD_MAP_APPLY_REFRESHED      2   /* normal, min and max distance were recomputed */
#define LLD_MAP_APPLY_NO_REFERENCE   4
#define LLD_MAP_APPLY_INDEX_SKIPPED  8
typedef struct {
  int32_t n_cams, n_points, n_pt_obs, n_lines, n_ln_obs;   /* the counts of the window the result belongs to */
  int32_t n_levels;
  const double*  cam_qt;            /* [n_cams][7]; the local cameras' are read       */
  const double*  pt_xyz;            /* [n_points][3]                                  */
  const double*  line_x0;           /* [n_lines][3]                                   */
  const double*  line_dir;          /* [n_lines][3]                                   */
  const uint8_t* pt_obs_outlier;    /* [n_pt_obs]                                     */
  const uint8_t* ln_edge_outlier;   /* [n_ln_obs][2]                                  */
  const uint8_t* line_removed;      /* [n_lines]                                      */
  const float*   level_scale;       /* [n_levels] mvScaleFactors                      */
} lld_map_ba_apply_in;
typedef struct {
  int32_t n_local_cams;             /* written: the window's                          */
  int32_t n_pt_obs_erased, n_ln_obs_erased;   /* erasures that took effect            */
  int32_t n_points_bad, n_lines_bad;          /* went bad in this call                */
  int32_t n_index_skipped;
  float*   tcw;                     /* [n_local_cams][16] the poses as the keyframes get them (SetPose) */
  float*   ow;                      /* [n_local_cams][3]                              */
  float*   pt_pos;                  /* [n_points][3]                                  */
  float*   pt_normal;               /* [n_points][3]                                  */
  float*   pt_min_distance;         /* [n_points]                                     */
  float*   pt_max_distance;         /* [n_points]                                     */
  int32_t* pt_n_obs;                /* [n_points]                                     */
  int32_t* pt_ref_kf;               /* [n_points] -1 without lld_map_set_point_refs   */
  int32_t* pt_row_len;              /* [n_points]                                     */
  uint8_t* pt_flags;                /* [n_points] LLD_MAP_APPLY_* bits                */
  uint8_t* ln_bad;                  /* [n_lines]                                      */
  int32_t* ln_n_obs;                /* [n_lines]                                      */
  int32_t* ln_row_len;              /* [n_lines]                                      */
  float*   phase_ms;                /* NULL, or [3]: HIP-event times of upload, kernels, download */
} lld_map_ba_apply_out;
int  lld_map_set_point_refs(lld_map* map, int32_t n, const int32_t* slot, const int32_t* ref_kf);
int  lld_map_ba_apply(lld_map* map, const lld_map_ba_apply_in* in, lld_map_ba_apply_out* out);
/* The rows of one pool as the DEVICE holds them, for a caller that audits its mirror and for the tests: CSR with the capacity protocol of
 * lld_map_download_links - start [n + 1] is always written (from the host's lengths), data [capacity] only if the total fits, otherwise
 * LLD_ERR_INVALID with start alone written (data may be NULL with a capacity of 0).  LLD_ERR_HIP when a device row's length is not the
 * host's: never with a sound map.  A pool that was never allocated has empty rows.  One small upload, one kernel, one download, one wait.
 * LLD_ERR_INVALID also for a NULL argument, an unknown kind, n < 0, a slot out of the pool's range; n = 0 is LLD_OK. */
#define LLD_MAP_ROWS_POINT_OBS   0   /* per point slot: the observing keyframe slots                */
#define LLD_MAP_ROWS_POINT_IDX   1   /* per point slot: the keypoint indices, parallel to them      */
#define LLD_MAP_ROWS_KF_POINTS   2   /* per keyframe slot: the point slot per keypoint, or -1       */
#define LLD_MAP_ROWS_KF_LINES    3   /* per keyframe slot: the line slot per keyline, or -1         */
#define LLD_MAP_ROWS_LINE_OBS    4   /* per line slot: the observing keyframe slots                 */
#define LLD_MAP_ROWS_LINE_IDX    5   /* per line slot: the keyline indices                          */
int  lld_map_download_rows(lld_map* map, int32_t kind, int32_t n, const int32_t* slot, int32_t* start, int32_t capacity, int32_t* data);

/* ------------------------------------------------------------------ landmark refresh on the resident map (lld_map_refresh.hip)
 * MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth and MapLine::ComputeDistinctiveDescriptors - the rules of
 * lld_mappoint_refresh / lld_mapline_distinctive above, bit for bit - for the landmarks a list of slots names, read from and written to the
 * map's tables.  LocalMapping runs them in ProcessNewKeyFrame, after CreateNewMapPoints and twice in SearchInNeighbors; with the map
 * resident only the slot list (and the level table) travels up, and nothing has to be sent back into the map afterwards.
 *
 * Two row pools beyond the ones above, allocated by the first of these two setters (a map that never calls them allocates what it
 * allocated before).  The contract is that of the other setters: everything is validated first, a refusal changes nothing, one block and
 * one copy per call, the mutation count increments, a HIP failure behind the host bookkeeping poisons the map, lld_map_clear empties them.
 *   lld_map_set_keyframe_descriptors       desc[8 k ..] = mDescriptors.row(k) as eight uint32, for keypoints start[i] .. start[i+1] of keyframe
 *                                          slot[i].  LLD_ERR_INVALID also for a keyframe lld_map_set_keyframes never set or a row of another
 *                                          length than its point row.  The live total is bounded by 8 * max_kf_points words:
 *                                          LLD_ERR_UNSUPPORTED, nothing changed, when the call's rows would take it past that bound, and
 *                                          when twice that bound (or twice the line pool's) passes an int32 offset.
 *   lld_map_set_keyframe_line_descriptors  desc[dim k ..] = mDescriptorsLines.row(k), dim = the map's line_dim floats (they travel as bit
 *                                          patterns); the row length must be the keyframe's line row's; the bound is line_dim * max_kf_lines,
 *                                          with the same LLD_ERR_UNSUPPORTED past it.
 *
 * lld_map_refresh_points / lld_map_refresh_lines: n landmark slots, each at most once.  One small upload (the slots, the level table),
 * kernels on the context's stream with no host trip between them, one download, one wait; no allocation per call (the staging only grows).
 * Early return: a point whose state is isBad or never set, or whose observation row is empty, and a line that is bad, never set or without
 *   an observation row, is left alone: updated = 0, best_obs = best_median = -1.
 * Descriptor part (points with LLD_LANDMARK_DESCRIPTOR, every line): the stored row is in std::map order; observers whose keyframe is bad or
 *   never set are skipped; observer j contributes the row of its keyframe's descriptor pool at the index the landmark's index row stores
 *   for it; selection, median index and first-of-equal-medians are lld_mappoint_refresh's (for lines: lld_mapline_distinctive's float L2,
 *   rank count and `int median`).  The winner goes to the landmark's descriptor row; best_obs is its position in the stored row.
 * Normal part (points with LLD_LANDMARK_NORMAL_DEPTH): every stored observer counts, the centres are the keyframe table's, the reference is
 *   lld_map_set_point_refs', the level is the octave of the reference keyframe's keypoint at the point's stored index there (keypoint 0 when
 *   the reference is no observer) - the rules lld_map_ba_apply applies to a window's points, with the numerics of lld_mappoint_refresh.
 * No index is followed before it is held to the row it points into.  A landmark that fails one of these checks is NOT WRITTEN AT ALL (neither
 * part) and carries the bit in its updated byte; the call still returns LLD_OK:
 *   LLD_MAP_REFRESH_NO_INDEX       its index row is missing or of another length than its observation row
 *   LLD_MAP_REFRESH_NO_DESCRIPTOR  descriptor part: an observer that is not bad has no descriptor row reaching the stored index
 *   LLD_MAP_REFRESH_NO_REFERENCE   normal part: the conditions of LLD_MAP_APPLY_NO_REFERENCE
 * Refused before anything is queued, nothing changed.  LLD_ERR_INVALID: a NULL argument, slot or updated array; n < 0; a slot out of range or
 * named twice; flags zero or with unknown bits; with the normal part a NULL level_scale or n_levels outside [1, LLD_ORB_MAX_LEVELS].
 * LLD_ERR_UNSUPPORTED: a named point whose observation row is longer than LLD_LANDMARK_MAX_OBS, a named line whose row is longer than
 * LLD_LANDMARK_MAX_LINE_OBS.  LLD_ERR_HIP for a poisoned map.  n = 0 is LLD_OK and touches nothing.
 * A call that wrote a landmark counts as a mutation of the map: a BA window staged before it is stale, and lld_map_ba_apply refuses it, as
 * after any setter.  No row length changes.  A HIP failure behind the first launch poisons the map.
 * Outputs are per query, read from the tables behind the writes (so a landmark that was not written shows what the map holds); every
 * output array but updated may be NULL. */
#define LLD_MAP_REFRESH_NO_INDEX       4   /* updated bits, beside LLD_LANDMARK_DESCRIPTOR / LLD_LANDMARK_NORMAL_DEPTH */
#define LLD_MAP_REFRESH_NO_DESCRIPTOR  8
#define LLD_MAP_REFRESH_NO_REFERENCE   16
typedef struct {
  int32_t n;                        /* point slots named                                */
  uint32_t flags;                   /* LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH */
  int32_t n_levels, reserved;
  const int32_t* slot;              /* [n]                                              */
  const float*   level_scale;       /* [n_levels] mvScaleFactors; normal part only      */
} lld_map_refresh_points_in;
typedef struct {
  uint32_t* desc;                   /* [n][8] p_desc behind the call                    */
  int32_t*  best_obs;               /* [n] position in the stored row, or -1            */
  int32_t*  best_median;            /* [n] or -1                                        */
  float*    normal;                 /* [n][3]                                           */
  float*    min_distance;           /* [n]                                              */
  float*    max_distance;           /* [n]                                              */
  uint8_t*  updated;                /* [n] required                                     */
  float*    phase_ms;               /* NULL, or [3]: HIP-event times of upload, kernels, download */
} lld_map_refresh_points_out;
typedef struct {
  int32_t n, reserved;
  const int32_t* slot;              /* [n] line slots                                   */
} lld_map_refresh_lines_in;
typedef struct {
  float*   desc;                    /* [n][line_dim] l_desc behind the call             */
  int32_t* best_obs;                /* [n] or -1                                        */
  int32_t* best_median;             /* [n] the int of the QUIRK, or -1                  */
  uint8_t* updated;                 /* [n] required: LLD_LANDMARK_DESCRIPTOR, or LLD_MAP_REFRESH_* bits */
  float*   phase_ms;
} lld_map_refresh_lines_out;
int  lld_map_set_keyframe_descriptors(lld_map* map, int32_t n, const int32_t* slot, const int32_t* start, const uint32_t* desc);
int  lld_map_set_keyframe_line_descriptors(lld_map* map, int32_t n, const int32_t* slot, const int32_t* start, const float* desc);
int  lld_map_refresh_points(lld_map* map, const lld_map_refresh_points_in* in, lld_map_refresh_points_out* out);
int  lld_map_refresh_lines(lld_map* map, const lld_map_refresh_lines_in* in, lld_map_refresh_lines_out* out);
/* The fixed rows of point / line slots as the DEVICE holds them - the twins of lld_map_download_rows for an audit and for the tests.  One
 * small upload, one kernel, one download, one wait; any output array may be NULL; a slot may be named more than once.  state: 0 never set,
 * 1 live, 2 isBad; bad: 1 isBad or never set.  LLD_ERR_INVALID for a NULL map or slot array, n < 0, a slot out of range; LLD_ERR_HIP for a
 * poisoned map; n = 0 is LLD_OK. */
int  lld_map_download_points(lld_map* map, int32_t n, const int32_t* slot, float* pos, float* normal, float* min_distance, float* max_distance,
                             uint32_t* desc, uint8_t* state);
int  lld_map_download_lines(lld_map* map, int32_t n, const int32_t* slot, float* desc, uint8_t* bad);

/* ------------------------------------------------------------------ duplicate map points fused on the resident map
 * lld_map_fuse: one ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:825-958) on the map's tables, as LocalMapping::SearchInNeighbors
 * (src/LocalMapping.cc:455-535) calls it 10-30 times per keyframe.  Nothing is gathered: the target keyframe's keypoints, octaves and
 * descriptors are its rows of lld_map_set_keyframe_features / _keypoints / _descriptors, the candidates' positions, normals, distances,
 * descriptors, flags and observation rows are the points' rows, and the holders are the target's point row.  Two phases.
 *
 * Search (device).  Candidate i is skipped (:846-850) when its slot is -1, was never set, is bad, or holds the target in its observation
 * row.  Otherwise it is projected with the float operations of lld_orb_fuse_search (the pose, centre, intrinsics and bounds travel in
 * `view` and are NOT rebuilt from the map's stored pose, so that both routes see the same floats), and every keypoint k of the target is a
 * candidate match under the rules of LLD_ORB_CAND_GRID with the gates LEVEL | CHI2 above: |dx| < r && |dy| < r with r = th *
 * level_scale[level]; the keypoint's PosInGrid cell (rounded) lies inside the grid and inside GetFeaturesInArea's cell range of the window;
 * octave in [level - 1, level] (and inside the level tables); the 7.8 / 5.99 chi2 gate on level_inv_sigma2; DescriptorDistance against
 * the point's descriptor row.  match[i] = the FIRST minimum in GetFeaturesInArea's order (column outer, row inner, index within the cell)
 * if its distance is <= 50, else -1: what lld_orb_fuse_search returns for the same inputs, bit for bit.
 *
 * Walk (host, on the copies of the rows the map keeps, in list order over the matched candidates; :934-956 as adapters/
 * lld_matcher_adapter.cc restates it behind a finished search).  The candidate is tested again: bad by now, or attached to the target by an
 * earlier step -> action 5.  The holder is the target's point row at match[i]:
 *   none              AddObservation + AddMapPoint: the candidate's observation and index rows grow by (target, match[i]), its
 *                     Observations() by 2 if the keypoint's uR >= 0, else by 1, the target's entry is set.  action 1.
 *   bad or never set  counted, nothing done.  action 4.
 *   else              Observations(holder) > Observations(candidate): the candidate is replaced by the holder (action 2), else the holder by
 *                     the candidate (action 3; a tie replaces the holder).  MapPoint::Replace (src/MapPoint.cc:176-220) row-wise: the same slot
 *                     returns; the loser's entries in stored order - the survivor absent from that keyframe: its entry there becomes the
 *                     survivor, the survivor gains the observation (+2 / +1 by that keyframe's uR at that index); present: the entry is
 *                     cleared by index; the loser becomes bad with empty rows, its Observations() stays what it was; mpRefKF untouched.
 * A new observation enters a row in front of the first stored observer whose order key (lld_map_set_keyframes) is greater than the new
 * keyframe's: a row stored in std::map order stays in it.  An index beyond a keyframe's rows writes nothing there and counts as monocular.
 * mnFound / mnVisible are no tables of the map: the caller adds the loser's to the survivor's from action / other (MapPoint.cc:210-211).
 * Then one upload carries every changed row (through the pools' one placement machinery: in place, to the tail, or a repack) and the
 * changed counts and flags, and behind it on the stream ComputeDistinctiveDescriptors (MapPoint.cc:212) runs for every survivor, once, on
 * the rows the call leaves, with lld_map_refresh_points' kernels and guards.  QUIRK kept apart from the reference: a survivor that a later
 * step of the same call makes bad keeps the descriptor it had (the reference recomputed it before; a bad point's descriptor is never read).
 * survivor[]: the distinct survivors in walk order, n_survivors of them.
 *
 * Refused before anything is queued, map unchanged.  LLD_ERR_INVALID: a NULL argument or output array; a target out of range, never set, or
 * without feature, keypoint and descriptor rows of its point row's length; n_points < 0; both or neither of point_slot / source_keyframe
 * (with source_keyframe >= 0: a keyframe never set, or n_points other than its point row's length); a slot outside [-1, max_points);
 * th, fx or fy not > 0; n_levels outside [1, LLD_ORB_MAX_LEVELS] or other than view.n_levels; a NULL level table; grid_cols / grid_rows < 1;
 * a candidate or holder of the walk whose index row is not of its observation row's length; more survivors than survivor_capacity (then
 * n_survivors holds the number needed; the search has run by then, so a caller that retries pays for it twice - a capacity of n_points
 * never meets this).  LLD_ERR_UNSUPPORTED: a live total of a pool beyond its limit, a survivor row longer than
 * LLD_LANDMARK_MAX_OBS, a target of more than 2^24 keypoints or a grid of more than 2^24 cells.  LLD_ERR_HIP: a poisoned map.
 * n_points = 0 is LLD_OK and touches nothing.  A slot may be named twice: the second occurrence meets the re-test.
 * A call that changed anything counts as one mutation: a staged BA window is stale.  A HIP failure behind the first queued change, or a
 * row length on the device that is not the host's, poisons the map.  phase_ms (NULL or [4]): HIP-event times of the search's upload and
 * kernels, the host clock over walk + row upload + refresh, the HIP-event time of the search's download. */
typedef struct {
  int32_t target;                   /* keyframe slot of pKF                             */
  int32_t n_points;                 /* candidates, in vpMapPoints order                 */
  const int32_t* point_slot;        /* [n_points], -1 = a NULL entry; NULL with source_keyframe >= 0 */
  int32_t source_keyframe;          /* -1, or: the candidates are this keyframe's point row as the map holds it */
  float th;                         /* 3.0 in SearchInNeighbors                         */
  lld_frame_view view;              /* pKF's pose, Ow, intrinsics, bounds, log scale factor, levels */
  float grid_min_x, grid_min_y, grid_width_inv, grid_height_inv;
  int32_t grid_cols, grid_rows;
  int32_t n_levels, reserved;
  const float* level_scale;         /* [n_levels] mvScaleFactors                        */
  const float* level_inv_sigma2;    /* [n_levels] mvInvLevelSigma2                      */
} lld_map_fuse_in;
typedef struct {
  int32_t n_fused;                  /* nFused (:956)                                    */
  int32_t n_added, n_replaced;      /* actions 1; actions 2 and 3                       */
  int32_t reserved;
  int32_t* match;                   /* [n_points] bestIdx or -1: the search alone       */
  uint8_t* action;                  /* [n_points] 0 none, 1 added, 2 candidate replaced by holder, 3 holder replaced by candidate,
                                       4 holder bad, 5 skipped by the walk's re-test    */
  int32_t* other;                   /* [n_points] the holder's slot for 2 / 3 / 4, else -1 */
  int32_t survivor_capacity, n_survivors;
  int32_t* survivor;                /* [survivor_capacity]                              */
  float*   phase_ms;                /* NULL or [4]                                      */
} lld_map_fuse_out;
#define LLD_MAP_FUSE_NONE 0
#define LLD_MAP_FUSE_ADDED 1
#define LLD_MAP_FUSE_CANDIDATE_REPLACED 2
#define LLD_MAP_FUSE_HOLDER_REPLACED 3
#define LLD_MAP_FUSE_HOLDER_BAD 4
#define LLD_MAP_FUSE_SKIPPED 5
int  lld_map_fuse(lld_map* map, const lld_map_fuse_in* in, lld_map_fuse_out* out);
/* MapPoint::Observations() of point slots as the DEVICE holds it (0 before the first lld_map_set_observations_indexed): the twin of
 * lld_map_download_points for the one fixed value it does not carry.  Refusals as there. */
int  lld_map_download_point_counts(lld_map* map, int32_t n, const int32_t* slot, int32_t* n_obs);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* LLD_AMD_H */
