/*
 * tpamd.h -- C-ABI of the MI355X (gfx950) batched time-optimal path-timing engine.
 *
 * The reference (theteamatx/x-edr-trajectory-planning) has no FFI: its boundary
 * is the C++ class API of trajectory_planning/. Every entry point below names
 * the reference interface (file:line under trajectory_planning/) whose work it
 * performs for a BATCH of independent paths. The C++ mirror classes in
 * x-edr-trajectory-planning_amd/host/ call these with B = 1 (drop-in) or B >> 1
 * (BatchPathTiming); INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *  - All arithmetic is fp64 (time_optimal_path_timing.h:38-41).
 *  - "_device" entry points take DEVICE pointers, enqueue work on the given HIP
 *    stream (hipStream_t passed as void*) and return without synchronising.
 *    "_host" entry points take HOST pointers, copy in, run, copy out and
 *    synchronise before returning.
 *  - Return value: 0 on success, a negative TPAMD_E_* code for call-level errors
 *    (bad arguments, HIP failure). Per-path solver outcomes are written to the
 *    status[] array (TPAMD_PATH_*), in the reference's order of checks.
 *  - No exceptions cross this boundary. An engine handle is not thread-safe;
 *    distinct engines may be used from distinct threads.
 */
#ifndef TPAMD_H_
#define TPAMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPAMD_VERSION 200

/* call-level errors */
#define TPAMD_E_INVALID_ARGUMENT (-1)
#define TPAMD_E_HIP (-2)
#define TPAMD_E_UNSUPPORTED (-3)
#define TPAMD_E_NO_DEVICE (-4)
#define TPAMD_E_STALE (-5) /* engine-held state belongs to a different solve */

/* per-path status (status[b]); 0 = solved. Codes follow the reference's checks:
 * SetupProblem (time_optimal_path_timing.cc:165-193), IsSetupValid (:554-576),
 * OptimizePathParameter (:383-391, :400-403, :422-428). */
#define TPAMD_PATH_OK 0
#define TPAMD_PATH_INFEASIBLE_BOUNDS 2
#define TPAMD_PATH_S_RANGE 3
#define TPAMD_PATH_SD_START_NEGATIVE 4
#define TPAMD_PATH_LOWER_GE_UPPER 5
#define TPAMD_PATH_TOO_FEW_SAMPLES 6
#define TPAMD_PATH_NO_CONNECTION 7
#define TPAMD_PATH_NAN_SD2 8
#define TPAMD_PATH_NONZERO_END 9
#define TPAMD_PATH_CRIT_INDEX_ZERO 10 /* reference reads sd2_max[-1] here (.cc:361,:372) */
#define TPAMD_PATH_NO_WAYPOINTS 11 /* tpamd_time_waypoint_paths_*: a path without waypoints has no spline (timeable_path_joint_spline.cc:200-207) */
#define TPAMD_PATH_SWEEP_POLL_EXPIRED 12 /* internal error, never expected: a bounded wait between the two waves of a sweep workgroup ran out (csrc/tpamd_sweep_joint.h, "loop queue") */

typedef struct tpamd_engine tpamd_engine;

/* Engine lifetime. An engine owns a device workspace that grows on demand
 * (outside any timed region once warmed up) and is bound to one HIP device. */
int tpamd_engine_create(int device_ordinal, tpamd_engine **out);
void tpamd_engine_destroy(tpamd_engine *engine);
int tpamd_version(void);
const char *tpamd_error_string(int code);
/* HIP devices visible to the library (0: none, the engine has no CPU fallback). */
int tpamd_device_count(void);
/* Pre-size the workspace for batches up to (num_paths, num_samples, num_rows). */
int tpamd_engine_reserve(tpamd_engine *engine, int num_paths, int num_samples,
                         int num_rows);
/* Pipelined modes for streams of joint-space solves (tpamd_time_joint_paths_device). The engine
 * keeps two workspaces, used alternately.
 *   1: the front stage of a solve (set-up and the sampling / LP kernel, which also writes out->q)
 *      runs on a stream of the engine, so that it overlaps the extremal sweep of the PREVIOUS
 *      solve; the sweep and every other output stay on the caller's stream, in order.
 *   2: the sweep runs on one of two engine streams as well, ordered behind the call's position in
 *      the caller's stream and behind its own front stage, so that it can start while the slowest
 *      paths of the previous solve are still running. The caller's stream is ordered behind the
 *      PREVIOUS solve when a call returns; tpamd_engine_fence orders it behind all of them.
 * Contract while a mode is on: the inputs of a call (and its out->q buffer) must be ready when the
 * call is made -- the front stage is NOT ordered behind earlier work on the caller's stream -- and
 * must stay untouched until the caller's stream has passed the call (mode 2: the fence). Only
 * tpamd_time_joint_paths_device is pipelined: the _host entry points and every other solve
 * (rows, Cartesian, planning windows, joint groups) run in order on the caller's stream and are
 * ordered against the engine's streams where they share a workspace with pipelined solves. Calls
 * captured into a HIP graph run unpipelined; fence and synchronise the engine before capturing
 * (a captured stream cannot wait for work outside the capture). 0 = off (default); changing the
 * mode waits for the engine's streams. */
int tpamd_engine_set_pipelining(tpamd_engine *engine, int mode);
/* Make hip_stream wait for every solve issued so far (needed in mode 2 before the outputs of the
 * last solve are used; harmless otherwise). */
int tpamd_engine_fence(tpamd_engine *engine, void *hip_stream);
/* Bytes of device workspace currently held. */
size_t tpamd_engine_workspace_bytes(const tpamd_engine *engine);

/* ------------------------------------------------------------------------
 * Form (i): joint-space degree-2 B-spline paths.
 * Performs, per path, what PathTimingTrajectory::ComputeTimingProfile runs for a
 * TimeableJointSplinePath (path_timing_trajectory.cc:307-475):
 *   SamplePath          timeable_path_joint_spline.cc:294-318
 *                       (BSplineBase::KnotSpan bspline_base.cc:218-246,
 *                        UpdateBasisAndDerivatives :268-348,
 *                        BSplineT::EvalCurveAndDerivatives bspline.h:540-568)
 *   ConstraintSetup     timeable_path_joint_spline.cc:320-343 (C = 2D rows)
 *   InitSolver/SetupProblem/SetSetupDone  time_optimal_path_timing.cc:135-203,:535-576
 *                       with s_start = path_start, s_end = path_start + delta*(N-1)
 *   OptimizePathParameter                  time_optimal_path_timing.cc:287-490
 *   epilogue qd = q'*sd, qdd = clamp(q'*sdd + q''*sd^2, +-a_max)  path_timing_trajectory.cc:458-472
 * ------------------------------------------------------------------------ */
typedef struct tpamd_joint_batch {
  int32_t num_paths;        /* B */
  int32_t num_dofs;         /* D, 1..16 */
  int32_t num_samples;      /* N, 3..8192 (JointPathOptions::num_path_samples) */
  int32_t num_points;       /* P control points per path; P+3 knots */
  int32_t max_solver_loops; /* <=0: max(100, 10*N) as path_timing_trajectory.cc:398-400 */
  int32_t reserved;
  double constraint_safety; /* PathOptions::constraint_safety, timeable_path.h:80 */
} tpamd_joint_batch;

typedef struct tpamd_joint_inputs {
  const double *knots;          /* [B][P+3] */
  const double *control_points; /* [B][P][D] */
  const double *max_velocity;   /* [B][D]  TimeablePath::SetMaxJointVelocity */
  const double *max_acceleration; /* [B][D] TimeablePath::SetMaxJointAcceleration */
  const double *path_start;     /* [B]  SamplePath(path_start) */
  const double *delta;          /* [B]  PathOptions::delta_parameter */
  const double *sd_start;       /* [B]  SetupProblem sd_start */
  const double *sdd_start;      /* [B]  SetupProblem sdd_start; NULL = 0 */
  const double *time_start;     /* [B]  SetupProblem time_start */
  /* Ragged batches (BASELINE.json configs[4]): samples of each path, 3 <= n[b] <=
   * num_samples; NULL = every path has num_samples. All [B][N]-shaped arrays keep the
   * stride num_samples; entries beyond n[b] are not written. The sweep then takes the paths
   * longest first (a device-side counting sort), whatever their order in the batch. */
  const int32_t *num_samples_per_path; /* [B] or NULL */
} tpamd_joint_inputs;

typedef struct tpamd_path_outputs {
  double *time;  /* [B][N] GetTimeSamples()      */
  double *s;     /* [B][N] GetPathParameter()    */
  double *sd;    /* [B][N] GetPathVelocity()     */
  double *sdd;   /* [B][N] GetPathAcceleration() */
  double *q;     /* [B][N][D] GetPathPositionAt(i); may be NULL */
  double *qd;    /* [B][N][D] velocity_at_path_samples_; may be NULL */
  double *qdd;   /* [B][N][D] acceleration_at_path_samples_; may be NULL */
  int32_t *last_extremal_index; /* [B] GetLastExtremalIndex(); may be NULL */
  double *max_time_increment;   /* [B] GetMaxTimeIncrement(); may be NULL */
  int32_t *status;              /* [B] TPAMD_PATH_* */
  double *sd2;                  /* [B][N] squared path velocity sd2_ (sd = sqrt(sd2)); may be NULL */
} tpamd_path_outputs;

int tpamd_time_joint_paths_device(tpamd_engine *engine, const tpamd_joint_batch *batch,
                                  const tpamd_joint_inputs *in,
                                  const tpamd_path_outputs *out, void *hip_stream);
int tpamd_time_joint_paths_host(tpamd_engine *engine, const tpamd_joint_batch *batch,
                                const tpamd_joint_inputs *in,
                                const tpamd_path_outputs *out);

/* Several joint-space batches solved CONCURRENTLY (BASELINE.json configs[4]: a mixed 6/7/14-joint
 * batch with 500..4000 samples per path). The kernels are specialised on the joint count, and a
 * launch's LDS is sized by its sample stride, so a mixed batch is bucketed by the caller into
 * groups of one (num_dofs, num_points, stride) each -- BatchPathTiming buckets by
 * (D, P, ceil(N / 512)) -- and every group is what tpamd_time_joint_paths_* takes. Here the groups
 * of one call run side by side: the groups are taken heaviest first (stride x joints) and dealt
 * to the engine's lanes (a stream and a workspace of the engine's own each; four, the number of
 * hardware queues the runtime uses), the heaviest on the highest-priority lane; their sampling/LP
 * kernels run one after another in that order, their sweeps overlap. The
 * lanes fork from hip_stream's position at the call and hip_stream waits for all of them before it
 * goes on, so for the caller the call behaves like one solve on hip_stream. Within a ragged group
 * the sweep takes the paths longest first (as tpamd_time_joint_paths_* does). Never pipelined.
 * Same per-path results as separate calls, bit for bit. batches/inputs/outputs: [num_groups]. */
int tpamd_time_joint_groups_device(tpamd_engine *engine, int num_groups,
                                   const tpamd_joint_batch *batches,
                                   const tpamd_joint_inputs *inputs,
                                   const tpamd_path_outputs *outputs, void *hip_stream);
int tpamd_time_joint_groups_host(tpamd_engine *engine, int num_groups,
                                 const tpamd_joint_batch *batches, const tpamd_joint_inputs *inputs,
                                 const tpamd_path_outputs *outputs);

/* Stand-alone batched TimeableJointSplinePath::SamplePath
 * (timeable_path_joint_spline.cc:294-318): q, q' = dq/ds, q'' = d2q/ds2 at
 * path_start + i*delta, i < N, as [B][N][D] host arrays (GetPathPositionAt,
 * GetFirstPathDerivativeAt, GetSecondPathDerivativeAt). */
int tpamd_sample_joint_paths_host(tpamd_engine *engine, int num_paths, int num_dofs,
                                  int num_samples, int num_points, const double *knots,
                                  const double *control_points, const double *path_start,
                                  const double *delta, double *q, double *q1, double *q2);

/* ---- Waypoint batches: fit on the device, any waypoint count per path ------------------------
 * TimeableJointSplinePath::SetWaypoints / FitSplineToWaypoints
 * (timeable_path_joint_spline.cc:200-207, :252-292) for num_paths paths at once, the joint
 * counterpart of tpamd_fit_pose_waypoints_*. Path k takes waypoints waypoint_offsets[k] ..
 * waypoint_offsets[k + 1]) of waypoints [rows][D] and rounding[k] (rounding NULL: 0.2, the default
 * of PathOptions::rounding):
 *   - control points: PolyLineToBspline3Waypoints with the rounding radius (:253-254), P_k =
 *     max(3 W_k - 2, 4);
 *   - uniform degree-2 knots on [0, 1] (splines/bspline_base.cc:356-381), every knot multiplied by
 *     max(length of the control polygon, 0.1) (:271-285).
 * The outputs are packed raggedly, path k behind path k - 1, as tpamd_fit_pose_waypoints_* packs
 * them: knots (sum of P_k + 3 values), control_points [sum P_k][D]. Per path: num_points[k],
 * path_end[k] (the last knot) and status[k] TPAMD_PLAN_*. A path without waypoints gets
 * TPAMD_PLAN_INVALID_ARGUMENT, num_points 0 and path_end 0, occupies no slots and leaves the other
 * paths as they are without it. point_offsets [num_paths + 1] (may be NULL) receives the first
 * control point of every path; it is always a HOST array, computed from the waypoint counts before
 * the launch (path k's knots start at point_offsets[k] + 3 * (paths with waypoints before k)).
 * Knots and control points are bit-identical to the host mirror's fit.
 * Call-level errors write nothing: a NULL engine or required array, num_paths < 0, num_dofs
 * outside 1..16, waypoint_offsets[0] != 0 or decreasing offsets (TPAMD_E_INVALID_ARGUMENT); more
 * than 65535 paths (TPAMD_E_UNSUPPORTED). Host pointers; synchronises. */
int tpamd_fit_joint_waypoints_host(tpamd_engine *engine, int num_paths, int num_dofs,
                                   const int32_t *waypoint_offsets, const double *waypoints,
                                   const double *rounding, double *knots, double *control_points,
                                   int32_t *num_points, int32_t *point_offsets, double *path_end,
                                   int32_t *status);
/* The same with every array except waypoint_offsets and point_offsets a device pointer. Enqueues
 * on hip_stream (NULL: the null stream) and does not synchronise; the offsets go up on hip_stream
 * first, into the buffer of the engine that tpamd_fit_pose_waypoints_device documents (shared with
 * it: the next call of any of these _device entries waits on its stream for this one's kernel). */
int tpamd_fit_joint_waypoints_device(tpamd_engine *engine, int num_paths, int num_dofs,
                                     const int32_t *waypoint_offsets, const double *waypoints,
                                     const double *rounding, double *knots, double *control_points,
                                     int32_t *num_points, int32_t *point_offsets, double *path_end,
                                     int32_t *status, void *hip_stream);

/* Waypoints in, trajectories out: SetWaypoints (as above) and then, per path, what
 * tpamd_time_joint_paths_* computes (SamplePath .. OptimizePathParameter .. the epilogue, see Form
 * (i)) with path_start 0, in ONE call for paths of any waypoint count and any sample count. The
 * fit runs on the device into a scratch of the engine in which every path has a slot of
 * max_k P_k control points (it grows on demand and lives until tpamd_engine_destroy); the
 * sampling/LP kernel reads every path's own count from it, so nothing is bucketed by size. */
typedef struct tpamd_waypoint_batch {
  int32_t num_paths;        /* B */
  int32_t num_dofs;         /* D, 1..16 */
  int32_t num_samples;      /* N, 3..8192: stride of the [B][N] outputs and the largest per-path count */
  int32_t max_solver_loops; /* as tpamd_joint_batch */
  double constraint_safety; /* as tpamd_joint_batch */
} tpamd_waypoint_batch;

typedef struct tpamd_waypoint_inputs {
  const int32_t *waypoint_offsets;     /* [B+1] HOST array in both entries */
  const double *waypoints;             /* [rows][D] */
  const double *rounding;              /* [B] PathOptions::rounding; NULL = 0.2 */
  const double *max_velocity;          /* [B][D] */
  const double *max_acceleration;      /* [B][D] */
  const int32_t *num_samples_per_path; /* [B] n_k <= num_samples; NULL = every path has num_samples */
  /* [B] PathOptions::delta_parameter; NULL = every path is covered exactly by its samples:
   * delta_k = path_end_k / (n_k - 1), one IEEE division on the device, where the length is known */
  const double *delta;
  const double *sd_start;              /* [B]; NULL = 0 */
  const double *time_start;            /* [B]; NULL = 0 */
} tpamd_waypoint_inputs;

/* What the fit found, each array optional (a NULL struct: none). knots / control_points have one
 * slot of S = max(3 max_k W_k - 2, 4) control points per path -- [B][S + 3] and [B][S][D]; path k
 * uses the first num_points[k] + 3 and num_points[k] entries of its slot; what the rest of a slot
 * holds afterwards is unspecified. */
typedef struct tpamd_waypoint_fit_outputs {
  int32_t *num_points;    /* [B] P_k; 0 without waypoints */
  double *path_end;       /* [B] the last knot; 0 without waypoints */
  double *delta_used;     /* [B] the delta the path was sampled with */
  double *knots;          /* [B][S + 3] */
  double *control_points; /* [B][S][D] */
} tpamd_waypoint_fit_outputs;

/* `out` has the layout and meaning of tpamd_time_joint_paths_* (time, s, sd, sdd and status are
 * required). A path without waypoints gets status TPAMD_PATH_NO_WAYPOINTS whatever else is wrong
 * with it, none of its other outputs is written, and the other paths are what they are without it,
 * bit for bit. A count n_k outside [2, num_samples] fails path k alone (TPAMD_PATH_TOO_FEW_SAMPLES).
 * With per-path counts the sweep takes the paths longest first, as tpamd_time_joint_paths_* does.
 * Never pipelined (tpamd_engine_set_pipelining): the fit precedes the front stage on the caller's
 * stream. Call-level errors write nothing: a NULL engine, struct or required array, num_paths < 0,
 * waypoint_offsets[0] != 0 or decreasing offsets (TPAMD_E_INVALID_ARGUMENT); num_dofs outside
 * 1..16, num_samples outside 3..8192, more than 65535 paths, or a largest P_k whose knots and
 * control points do not fit the sampling/LP kernel's 160 KB of LDS (TPAMD_E_UNSUPPORTED); the
 * _host entry also refuses a per-path count above num_samples (TPAMD_E_INVALID_ARGUMENT). Host
 * pointers; synchronises. */
int tpamd_time_waypoint_paths_host(tpamd_engine *engine, const tpamd_waypoint_batch *batch,
                                   const tpamd_waypoint_inputs *in, const tpamd_path_outputs *out,
                                   const tpamd_waypoint_fit_outputs *fit);
/* The same with every array except waypoint_offsets a device pointer. Enqueues on hip_stream and
 * does not synchronise, except when the engine's scratch has to grow; the offsets go up as
 * tpamd_fit_joint_waypoints_device stages them. */
int tpamd_time_waypoint_paths_device(tpamd_engine *engine, const tpamd_waypoint_batch *batch,
                                     const tpamd_waypoint_inputs *in, const tpamd_path_outputs *out,
                                     const tpamd_waypoint_fit_outputs *fit, void *hip_stream);

/* ------------------------------------------------------------------------
 * Form (ii): explicit constraint rows  lower <= A*sdd + B*sd^2 <= upper.
 * Batched TimeOptimalPathProfile::InitSolver + SetupProblem +
 * OptimizePathParameter (time_optimal_path_timing.h:118-150). Row arrays are
 * [B][N][C] (sample-major, row-minor): Constraint::a_coefficient/b_coefficient/
 * lower/upper (time_optimal_path_timing.h:65-102). q/qd/qdd outputs are unused.
 * ------------------------------------------------------------------------ */
typedef struct tpamd_rows_batch {
  int32_t num_paths;        /* B */
  int32_t num_samples;      /* N */
  int32_t num_rows;         /* C, 1..64 */
  int32_t max_solver_loops; /* <=0: 100 (time_optimal_path_timing.h:339) */
} tpamd_rows_batch;

typedef struct tpamd_rows_inputs {
  const double *a;      /* [B][N][C] */
  const double *b;      /* [B][N][C] */
  const double *lower;  /* [B][N][C] */
  const double *upper;  /* [B][N][C] */
  const double *s_start, *s_end, *sd_start, *sdd_start, *time_start; /* [B] each */
} tpamd_rows_inputs;

int tpamd_optimize_rows_device(tpamd_engine *engine, const tpamd_rows_batch *batch,
                               const tpamd_rows_inputs *in,
                               const tpamd_path_outputs *out, void *hip_stream);
int tpamd_optimize_rows_host(tpamd_engine *engine, const tpamd_rows_batch *batch,
                             const tpamd_rows_inputs *in,
                             const tpamd_path_outputs *out);

/* Ragged rows batches: path b has n[b] = num_samples_per_path[b] samples, 3 <= n[b] <= num_samples,
 * and is solved exactly as a uniform call with num_samples = n[b] would solve it: ds = (s_end -
 * s_start) / (n[b] - 1), the last sample is n[b] - 1. The row arrays and every [B][N]-shaped
 * output keep the stride num_samples; rows at i >= n[b] are not read, outputs there are not
 * written. A count outside [2, num_samples] fails that path alone (TPAMD_PATH_TOO_FEW_SAMPLES, as a
 * joint batch reports it). For B > 1 the sweep takes the paths longest first.
 * num_samples_per_path [B] is a device array for _device, a host array for _host; NULL is
 * TPAMD_E_INVALID_ARGUMENT. The engine reads it until the stream has run the call. */
int tpamd_optimize_rows_ragged_device(tpamd_engine *engine, const tpamd_rows_batch *batch,
                                      const tpamd_rows_inputs *in, const int32_t *num_samples_per_path,
                                      const tpamd_path_outputs *out, void *hip_stream);
int tpamd_optimize_rows_ragged_host(tpamd_engine *engine, const tpamd_rows_batch *batch,
                                    const tpamd_rows_inputs *in, const int32_t *num_samples_per_path,
                                    const tpamd_path_outputs *out);

/* ------------------------------------------------------------------------
 * Form (iii): Cartesian-space paths after the IK callback (BASELINE.json configs[3]).
 * Replaces, for B paths at once, the arithmetic of TimeableCartesianSplinePath that
 * follows path_ik_func_: ComputePathDerivatives (timeable_path_cartesian_spline.cc:39-68,
 * called from SamplePath :541-542), ConstraintSetup (:551-595, C = 2D+2 rows), then
 * the solver and the planner epilogue as for joint paths. The pose-spline sampling, the
 * IK callback and the Jacobian callback are user std::functions (:508-510, :576) and stay
 * on the host: their results are the inputs here. J*q' is summed over the dofs in index
 * order. max_solver_loops <= 0: max(100, 10 N).
 * ------------------------------------------------------------------------ */
typedef struct tpamd_cartesian_batch {
  int32_t num_paths;        /* B */
  int32_t num_dofs;         /* D, 1..16 */
  int32_t num_samples;      /* N */
  int32_t max_solver_loops;
  double constraint_safety; /* CartesianPathOptions::constraint_safety */
} tpamd_cartesian_batch;

typedef struct tpamd_cartesian_inputs {
  const double *ik_positions;  /* [B][N][D]    path_position_ (IK solution per sample) */
  const double *jacobians;     /* [B][N][6][D] jacobian_func_(path_position_[i]), row-major */
  const double *max_velocity;      /* [B][D] */
  const double *max_acceleration;  /* [B][D] */
  const double *max_translational_velocity; /* [B] */
  const double *max_rotational_velocity;    /* [B] */
  const double *path_start, *delta, *sd_start, *sdd_start, *time_start; /* [B] each; sdd_start may be NULL */
} tpamd_cartesian_inputs;

/* out->q, if given, receives a copy of ik_positions. */
int tpamd_time_cartesian_paths_device(tpamd_engine *engine, const tpamd_cartesian_batch *batch,
                                      const tpamd_cartesian_inputs *in,
                                      const tpamd_path_outputs *out, void *hip_stream);
int tpamd_time_cartesian_paths_host(tpamd_engine *engine, const tpamd_cartesian_batch *batch,
                                    const tpamd_cartesian_inputs *in,
                                    const tpamd_path_outputs *out);

/* Ragged Cartesian batches: every path has its own sample count, and the IK rows may be packed.
 * Path b has n[b] = num_samples_per_path[b] samples, 3 <= n[b] <= batch->num_samples, and is timed
 * exactly as a uniform call with num_samples = n[b] would time it: s_end = path_start +
 * delta (n[b] - 1), the forward differences end at n[b] - 1 (q'[n[b]-1] = 0, q''[0] = q''[n[b]-1] =
 * 0), and max_solver_loops <= 0 means max(100, 10 n[b]). Same per-path results as separate uniform
 * calls, bit for bit.
 *   first_row == NULL  strided inputs: ik_positions [B][N][D] and jacobians [B][N][6][D] with
 *                      N = num_samples; path b's samples beyond n[b] are not read.
 *   first_row [B]      packed inputs: ik_positions [rows][D] and jacobians [rows][6][D] are row
 *                      tables, and path b reads rows first_row[b] .. first_row[b] + n[b] - 1: the
 *                      layout tpamd_sample_ik_targets_* writes, with first_row = row_offsets[0..B).
 *                      The paths' ranges may lie in any order and may overlap (they are only read).
 *                      rows < 2^31. num_rows tells the _host entry how many rows to stage.
 * Every [B][N]-shaped output keeps the stride num_samples; entries at i >= n[b] are not written
 * (the _host entry leaves the caller's memory there as it was). out->q, if given, receives path
 * b's rows at [b][0 .. n[b])[D] (a gather in the packed case).
 * A count outside [2, num_samples] fails that path alone with the status a ragged joint batch
 * gives such a path (TPAMD_PATH_S_RANGE below 2, where s_end <= s_start; TPAMD_PATH_TOO_FEW_SAMPLES
 * above num_samples); none of that path's rows is read, nothing but its per-path status entries
 * is written, and the other paths are unaffected. For B > 1 the sweep takes the paths longest first (the
 * device-side counting sort of ragged joint batches).
 * num_samples_per_path and first_row are device arrays for _device and host arrays for _host; the
 * engine reads them until the stream has run the call. Call-level errors as for the uniform entry;
 * a NULL num_samples_per_path (or, for _host with first_row, num_rows < 1 or >= 2^31) is
 * TPAMD_E_INVALID_ARGUMENT. Never pipelined. */
int tpamd_time_cartesian_paths_ragged_device(tpamd_engine *engine, const tpamd_cartesian_batch *batch,
                                             const tpamd_cartesian_inputs *in,
                                             const int32_t *num_samples_per_path, const int32_t *first_row,
                                             const tpamd_path_outputs *out, void *hip_stream);
int tpamd_time_cartesian_paths_ragged_host(tpamd_engine *engine, const tpamd_cartesian_batch *batch,
                                           const tpamd_cartesian_inputs *in,
                                           const int32_t *num_samples_per_path, const int32_t *first_row,
                                           int64_t num_rows, const tpamd_path_outputs *out);

/* Pose targets of Cartesian-space paths: what TimeableCartesianSplinePath::SamplePath evaluates
 * before it calls the IK callback (timeable_path_cartesian_spline.cc:484-503), for B paths at
 * once: the degree-2 translation spline (BSplineT::EvalCurve, splines/bspline.h:512-536) and the
 * degree-2 quaternion spline (BSplineQ::EvalCurve, splines/bsplineq.cc:223-244: cumulative basis
 * :309-317, QuatPower = exp(p log q) :112-146) on a shared knot vector, at
 * path_start[b] + i * delta[b], i < N; beyond knots.back() - delta the last control pose is
 * repeated. knots [B][P+3], translation_points [B][P][3], rotation_points [B][P][4] as
 * (w, x, y, z), poses [B][N][7] = (tx, ty, tz, qw, qx, qy, qz). The IK and Jacobian callbacks
 * stay with the caller; their results go to tpamd_time_cartesian_paths_*. */
int tpamd_sample_pose_splines_device(tpamd_engine *engine, int num_paths, int num_samples,
                                     int num_points, const double *knots,
                                     const double *translation_points,
                                     const double *rotation_points, const double *path_start,
                                     const double *delta, double *poses, void *hip_stream);
int tpamd_sample_pose_splines_host(tpamd_engine *engine, int num_paths, int num_samples,
                                   int num_points, const double *knots,
                                   const double *translation_points, const double *rotation_points,
                                   const double *path_start, const double *delta, double *poses);

/* ---- Cartesian goals: the two device stages around the caller's IK ------------------------
 * A Cartesian goal is pose waypoints plus joint seed waypoints. tpamd_fit_pose_waypoints_* turns
 * them into the pose spline and the joint seed spline; tpamd_sample_ik_targets_* turns both into
 * one pose target and one joint target per row of the IK table; the caller's IK (on the device)
 * turns the targets into the table tpamd_planner_set_upload_ik_tables_device takes. The IK stays
 * user code.
 *
 * Rows of a path's IK table as TimeableCartesianSplinePath::BuildIkTable counts them:
 * PathIkIndex(knots.back()) + N + 1 = round(path_end / delta) + num_samples + 1
 * (timeable_path_cartesian_spline.cc:671-674 with std::round). -1 for delta <= 0 or
 * num_samples < 1. Host arithmetic only. */
int tpamd_ik_table_rows(double path_end, double delta, int num_samples);
/* TimeableCartesianSplinePath::SetWaypoints / FitSplineToWaypoints
 * (timeable_path_cartesian_spline.cc:415-482) for num_paths paths at once. Path k takes waypoints
 * waypoint_offsets[k] .. waypoint_offsets[k + 1]) of pose_waypoints [rows][7] (tx, ty, tz, qw, qx,
 * qy, qz; quaternions are not normalised) and joint_waypoints [rows][D], with
 * translation_rounding[k] and rotation_rounding[k] (any value passes through; CornerOffset's 1e-6
 * rule is the only one):
 *   - joint control points: PolyLineToControlPoints with the rotation rounding as the radius
 *     (timeable_path_joint_spline.cc:252-292, the mirror passes options_.rounding());
 *   - pose control points: PolyLineToBspline3Waypoints on poses with CornerOffset
 *     (splines/spline_utils.cc:104-204);
 *   - uniform degree-2 knots on [0, 1] (splines/bspline_base.cc:356-381), every knot multiplied by
 *     max(L + L, 0.1) * 10, L the length of the translation control polygon (:436-438).
 * Path k has P_k = max(3 W_k - 2, 4) control points. The outputs are packed raggedly, path k behind
 * path k - 1, as tpamd_planner_set_upload_paths_ragged packs splines: knots (sum of P_k + 3 values),
 * translation_points [sum P_k][3], rotation_points [sum P_k][4] (w, x, y, z), joint_control_points
 * [sum P_k][D]. Per path: num_points[k], path_end[k] (the last knot) and status[k] TPAMD_PLAN_*. A
 * path without waypoints gets TPAMD_PLAN_INVALID_ARGUMENT, num_points 0 and path_end 0, occupies no
 * slots and leaves the other paths as they are without it. point_offsets [num_paths + 1] (may be
 * NULL) receives the first control point of every path; it is always a HOST array, computed from
 * the waypoint counts before the launch. The joint control points are bit-identical to the host
 * mirror; the pose control points and knots agree with it to rounding (atan2 / sin / cos of the
 * device math library).
 * Call-level errors write nothing: a NULL engine or required array, num_paths < 0, num_dofs
 * outside 1..16, waypoint_offsets[0] != 0 or decreasing offsets (TPAMD_E_INVALID_ARGUMENT); more
 * than 65535 paths (TPAMD_E_UNSUPPORTED). Host pointers; synchronises. */
int tpamd_fit_pose_waypoints_host(tpamd_engine *engine, int num_paths, int num_dofs,
                                  const int32_t *waypoint_offsets, const double *pose_waypoints,
                                  const double *joint_waypoints, const double *translation_rounding,
                                  const double *rotation_rounding, double *knots,
                                  double *translation_points, double *rotation_points,
                                  double *joint_control_points, int32_t *num_points,
                                  int32_t *point_offsets, double *path_end, int32_t *status);
/* The same with every array except waypoint_offsets and point_offsets a device pointer. Enqueues
 * on hip_stream (NULL: the null stream) and does not synchronise; the offsets go up on hip_stream
 * first, into a buffer of the engine that the next call of these _device entries reuses (that call
 * waits on its stream for this one's kernel). path_end lands in DEVICE memory: a caller that sizes
 * the target buffers copies num_paths doubles down and calls tpamd_ik_table_rows. */
int tpamd_fit_pose_waypoints_device(tpamd_engine *engine, int num_paths, int num_dofs,
                                    const int32_t *waypoint_offsets, const double *pose_waypoints,
                                    const double *joint_waypoints, const double *translation_rounding,
                                    const double *rotation_rounding, double *knots,
                                    double *translation_points, double *rotation_points,
                                    double *joint_control_points, int32_t *num_points,
                                    int32_t *point_offsets, double *path_end, int32_t *status,
                                    void *hip_stream);
/* The inputs of the IK callback as TimeableCartesianSplinePath::ExtendIkSolution evaluates them
 * (timeable_path_cartesian_spline.cc:484-526), for a ragged batch. Path k has num_points[k] >= 3
 * control points, packed as tpamd_fit_pose_waypoints_* packs them (no empty paths), and rows
 * row_offsets[k] .. row_offsets[k + 1]); row r belongs to parameter r * delta[k]. Below
 * knots.back() - delta the pose target is the translation spline (BSplineT::EvalCurve,
 * splines/bspline.h:512-536) and the quaternion spline (BSplineQ::EvalCurve,
 * splines/bsplineq.cc:223-244), exactly as tpamd_sample_pose_splines_* with path_start 0, and the
 * joint target the joint spline's EvalCurve; from there on (:488, :499-502) the last control pose
 * and the last joint control point, bit for bit. pose_targets [rows][7], joint_targets [rows][D].
 * Paths of any size are sampled (control points are read from global memory, not staged).
 * Call-level errors write nothing: a NULL engine or array, num_paths < 0, num_dofs outside 1..16,
 * num_points[k] < 3, row_offsets[0] != 0 or decreasing, delta[k] <= 0. Host pointers; synchronises. */
int tpamd_sample_ik_targets_host(tpamd_engine *engine, int num_paths, int num_dofs,
                                 const int32_t *num_points, const int32_t *row_offsets,
                                 const double *knots, const double *translation_points,
                                 const double *rotation_points, const double *joint_control_points,
                                 const double *delta, double *pose_targets, double *joint_targets);
/* The same with the four spline arrays, delta and the two outputs device pointers; num_points and
 * row_offsets stay HOST arrays. delta[k] cannot be checked on the host here: the kernel leaves the
 * rows of a path whose delta is not > 0 untouched. Enqueues on hip_stream and does not synchronise
 * (the staging of the offsets is that of tpamd_fit_pose_waypoints_device). */
int tpamd_sample_ik_targets_device(tpamd_engine *engine, int num_paths, int num_dofs,
                                   const int32_t *num_points, const int32_t *row_offsets,
                                   const double *knots, const double *translation_points,
                                   const double *rotation_points, const double *joint_control_points,
                                   const double *delta, double *pose_targets, double *joint_targets,
                                   void *hip_stream);
/* The same two entries for a part of every table: path k's output rows row_offsets[k] ..
 * row_offsets[k + 1]) are table rows first_row[k] .. first_row[k] + n_k - 1 (first_row is a HOST
 * array in both, >= 0). Table row r belongs to parameter r * delta[k], never to an accumulated
 * parameter, so the rows are bit-equal to the same rows of a whole-path sampling: the targets of
 * a streamed IK table (tpamd_planner_set_append_ik_rows*) do not depend on the chunking. */
int tpamd_sample_ik_target_rows_host(tpamd_engine *engine, int num_paths, int num_dofs,
                                     const int32_t *num_points, const int32_t *row_offsets,
                                     const int32_t *first_row, const double *knots,
                                     const double *translation_points, const double *rotation_points,
                                     const double *joint_control_points, const double *delta,
                                     double *pose_targets, double *joint_targets);
int tpamd_sample_ik_target_rows_device(tpamd_engine *engine, int num_paths, int num_dofs,
                                       const int32_t *num_points, const int32_t *row_offsets,
                                       const int32_t *first_row, const double *knots,
                                       const double *translation_points, const double *rotation_points,
                                       const double *joint_control_points, const double *delta,
                                       double *pose_targets, double *joint_targets, void *hip_stream);

/* ------------------------------------------------------------------------
 * Receding-horizon planning: the window loop of PathTimingTrajectory::Plan
 * (path_timing_trajectory.cc:628-660 around ComputeTimingProfile :307-475) for B planners with
 * TimeableJointSplinePath paths of one shape, CHAINED ON THE DEVICE. Per iteration and planner:
 * the window start is looked up in the planner's window history (the sample before the loop's
 * start time, :328-339; a new path starts at 0), the path is sampled and solved from there, the
 * start velocity of a new or modified path is projected on the start tangent (:360-393), the
 * window replaces the tail of the history (:418-472), and the loop continues from the start of
 * the final deceleration -- max(last_extremal_index, N/2) (:639-646), converted with the
 * nanosecond truncation of trajectory_planning/time.h:22-29 -- until the path's end is planned
 * (CloseToEnd, timeable_path_joint_spline.cc:142-144) or the time horizon is covered (:650-652).
 * Only the number of planners still looping crosses PCIe per iteration; histories and results
 * cross once per call. Host pointers; in/out arrays carry planner state between calls.
 * ------------------------------------------------------------------------ */
#define TPAMD_PLAN_OK 0
#define TPAMD_PLAN_FAILED_PRECONDITION 1 /* nothing to connect to (:324) */
#define TPAMD_PLAN_OUT_OF_RANGE 2
#define TPAMD_PLAN_INVALID_ARGUMENT 3    /* non-positive duration (:313-317), start velocity (:387-392) */
#define TPAMD_PLAN_INTERNAL 4            /* solver set-up / optimisation failed (:394-417) */
#define TPAMD_PLAN_DEADLINE_EXCEEDED 5   /* planning-loop limit (:655-658) */
#define TPAMD_PLAN_NOT_FOUND 6           /* stopping trajectories: no safe stop (trajectory_buffer.cc:333-349) */
#define TPAMD_PLAN_NEEDS_ROWS 7          /* Cartesian set, streaming Plan: the next window is not resident yet */
#define TPAMD_PLAN_RESOURCE_EXHAUSTED 8  /* tpamd_planner_set_plan_device: the history or trajectory buffer is full */
#define TPAMD_PLAN_MORE 100              /* history_capacity exhausted: call again with more room */

typedef struct tpamd_plan_args {
  int32_t num_planners, num_dofs, num_samples, num_points;
  int32_t history_capacity;        /* samples per planner the history arrays hold (their stride) */
  int32_t max_planning_iterations; /* PathTimingTrajectoryOptions::GetMaxPlanningIterations */
  double constraint_safety;        /* PathOptions::constraint_safety */
  double max_initial_velocity_error;
  const double *knots, *control_points;          /* [B][P+3], [B][P][D] */
  const double *max_velocity, *max_acceleration; /* [B][D] */
  const double *delta;                           /* [B] PathOptions::delta_parameter */
  const double *initial_velocity;                /* [B][D] TimeablePath::GetInitialVelocity */
  const int64_t *start_ns, *horizon_ns;          /* [B] Plan(start, time_horizon) */
  /* planner state, in/out */
  int32_t *path_state;      /* [B] 1 kNewPath, 2 kModifiedPath, 3 kPathWasSampled */
  int32_t *planned_to_end;  /* [B] in: planned_to_end_ after UpdatePathTrackingStatus */
  int32_t *history_count;   /* [B] size of time_at_path_samples_ */
  double *history_time, *history_s, *history_sd, *history_sdd; /* [B][capacity] *_at_path_samples_ */
  double *history_q, *history_qd, *history_qdd;                /* [B][capacity][D] */
  double *path_horizon;             /* [B] path_horizon_ */
  int64_t *final_decel_start_ns;    /* [B] final_decel_start_ as left by the loop (:645-646) */
  /* the last window each planner solved in this call: profile_ and the path's samples (out) */
  double *window_time, *window_s, *window_sd, *window_sdd, *window_sd2; /* [B][N] */
  double *window_q, *window_q1, *window_q2;                             /* [B][N][D] */
  double *window_path_start, *window_sd_start, *window_time_start;      /* [B] path_start_, path_start_velocity_, path_time_start_ */
  int32_t *window_last_extremal_index;  /* [B] */
  double *window_max_time_increment;    /* [B] */
  int32_t *status;   /* [B] TPAMD_PLAN_* */
  int32_t *windows;  /* [B] windows solved in this call (0: the outputs above are untouched) */
  /* Continuation after TPAMD_PLAN_MORE: the loop state of every planner, written by every call;
   * with resume != 0 it is read back in (call again with larger history arrays, same other
   * arguments), and only planners with looping[b] != 0 go on. */
  int32_t resume;
  int64_t *loop_start_ns;  /* [B] loop_start_time of the next window (:659) */
  int32_t *loop_count;     /* [B] windows counted by the loop so far (:633) */
  int32_t *looping;        /* [B] */
} tpamd_plan_args;

int tpamd_plan_joint_windows_host(tpamd_engine *engine, const tpamd_plan_args *args);

/* ------------------------------------------------------------------------
 * Planner sets: B PathTimingTrajectory planners (path_timing_trajectory.h:91-186) with
 * TimeableJointSplinePath paths of one shape whose WHOLE state lives on the device between Plan
 * calls -- the spline and limits, the window history (*_at_path_samples_), the planner scalars
 * (path_horizon_, planned_to_end_, final_decel_start_, start/end time, initial_plan_ ...), the
 * profile of the last window, and the resampled trajectory (time_, positions_, ...).
 * tpamd_planner_set_plan is Plan(start, time_horizon) (path_timing_trajectory.cc:579-684) for all
 * of them at once, entirely on the device: HandleTimeArguments :502-538, UpdatePathTrackingStatus
 * :477-500, the "planned enough" branch with EraseTrajectoryBefore :540-577 (both sampling
 * methods), the truncation at GetTimeOffsetAfter :604-621, the window loop :628-660 chained as in
 * tpamd_plan_joint_windows_host, ResampleTrajectory :755-836 and the bookkeeping of :662-684.
 * A Plan call moves 16 bytes per planner up (the two time arguments) and one status + summary
 * record down, plus a few words per window iteration; trajectories come down only when asked for
 * (tpamd_planner_set_download_trajectory). The mirror's PathTimingTrajectorySet wraps this.
 * History and trajectory buffers grow on the device when a planner needs more room.
 * ------------------------------------------------------------------------ */
typedef struct tpamd_planner_set tpamd_planner_set;

typedef struct tpamd_planner_set_config {
  int32_t num_planners, num_dofs, num_samples, num_points;
  int32_t history_capacity;        /* samples per planner to start with; <= 0: 8 * num_samples. It doubles
                                    * when a Plan fills it; neither sampling method bounds it */
  int32_t trajectory_capacity;     /* resampled samples per planner to start with; <= 0: 4096 */
  int32_t sampling_method;         /* 0 kUniformlyInTime, 1 kSkipSamplesCloserThanTimeStep */
  int32_t max_planning_iterations; /* PathTimingTrajectoryOptions::GetMaxPlanningIterations */
  double constraint_safety;        /* PathOptions::constraint_safety */
  double max_initial_velocity_error;
  int64_t time_step_ns;            /* TrajectoryPlannerOptions::GetTimeStep */
} tpamd_planner_set_config;

typedef struct tpamd_planner_summary {
  int64_t end_time_ns, final_decel_start_ns, start_time_ns; /* GetEndTime, GetFinalDecelStart, GetStartTime */
  int32_t num_samples;     /* GetNumTimeSamples */
  int32_t target_reached;  /* with path_state: IsTrajectoryAtEnd */
  int32_t planned_to_end;
  int32_t windows;         /* timing windows solved by this Plan call */
  int32_t path_state;      /* TimeablePath::State after the call (3 = kPathWasSampled) */
  int32_t history_count;   /* size of time_at_path_samples_ */
  int32_t status;          /* TPAMD_PLAN_* */
  int32_t reserved;
} tpamd_planner_summary;

int tpamd_planner_set_create(tpamd_engine *engine, const tpamd_planner_set_config *config,
                             tpamd_planner_set **out);
void tpamd_planner_set_destroy(tpamd_planner_set *set);
/* The paths of `count` planners (ids[count], or planners 0..count-1 if ids is NULL) after
 * SetWaypoints (path_state 1 = kNewPath) or SwitchToWaypointPath (2 = kModifiedPath), which stay on
 * the host (O(waypoints) spline edits): knots [count][P+3], control_points [count][P][D],
 * max_velocity / max_acceleration / initial_velocity [count][D], delta [count]. Host pointers. */
int tpamd_planner_set_upload_paths(tpamd_planner_set *set, int count, const int32_t *ids,
                                   const double *knots, const double *control_points,
                                   const double *max_velocity, const double *max_acceleration,
                                   const double *delta, const double *initial_velocity,
                                   const int32_t *path_state);
/* Paths of any size: planner k's path has num_points[k] >= 3 control points, its knots
 * (num_points[k] + 3) and control points (num_points[k] x D) packed behind those of planner k - 1
 * in `knots` / `control_points`; the other arrays as in tpamd_planner_set_upload_paths. The set's
 * per-planner capacity grows (by doubling) before anything changes; every id, state and size is
 * checked before the first copy. The fixed-size entry above takes paths of the config's
 * num_points. Host pointers; synchronises. */
int tpamd_planner_set_upload_paths_ragged(tpamd_planner_set *set, int count, const int32_t *ids,
                                          const int32_t *num_points, const double *knots,
                                          const double *control_points, const double *max_velocity,
                                          const double *max_acceleration, const double *delta,
                                          const double *initial_velocity, const int32_t *path_state);
/* The resident path of one planner: *num_points (0: no path) and, if the arrays are not NULL, its
 * knots [num_points + 3] and control points [num_points][D]. `capacity` is the number of control
 * points the arrays can hold; a larger path gives TPAMD_E_INVALID_ARGUMENT (*num_points is still
 * written). With both arrays NULL nothing crosses PCIe. */
int tpamd_planner_set_download_path(tpamd_planner_set *set, int planner, int32_t *num_points,
                                    double *knots, double *control_points, int capacity);
/* The online path switch (path_timing_trajectory_test.cc:298-420) for `count` planners of a set
 * (ids[count], each listed once, or planners 0..count-1 if ids is NULL), on the device:
 *   1. stop parameter: keep_path_until[k], or if keep_path_until is NULL the fastest-stop
 *      parameter GetPathStopParameter(time_ns[k]) (as tpamd_planner_set_stop_parameters);
 *   2. the velocity at time_ns[k] on the resident trajectory (TrajectoryBuffer::GetVelocityAtTime:
 *      TPAMD_PLAN_FAILED_PRECONDITION without a plan, TPAMD_PLAN_OUT_OF_RANGE outside it);
 *   3. TimeableJointSplinePath::SwitchToWaypointPath(stop, waypoints) with the new waypoints
 *      waypoints[waypoint_offsets[k] .. waypoint_offsets[k + 1])[D] (rounding radius 0.2, the
 *      PathOptions default), bit-identical to the host mirror;
 *   4. on success the new spline, the velocity as initial velocity and path_state 2
 *      (kModifiedPath) replace the planner's; the next tpamd_planner_set_plan plans it as
 *      PathTimingTrajectory::Plan plans a modified path. On failure the planner is unchanged.
 * Per planner: stop_parameter[k] (the one used), num_points[k] (the planner's control points after
 * the call) and status[k] TPAMD_PLAN_* (the first step that failed). Call-level errors (a bad or
 * repeated id, NULL arrays, waypoint_offsets[0] != 0 or decreasing) change nothing. The set's
 * per-planner capacity grows first if P + 3 + 3 (W + 1) - 2 does not fit. About 16 bytes per
 * planner plus the waypoints go up, 16 come down; no trajectory is downloaded. Host pointers;
 * synchronises. */
int tpamd_planner_set_switch_paths(tpamd_planner_set *set, int count, const int32_t *ids,
                                   const int64_t *time_ns, const double *keep_path_until,
                                   const int32_t *waypoint_offsets, const double *waypoints,
                                   double *stop_parameter, int32_t *num_points, int32_t *status);
/* The same with the PathOptions::rounding radius of the new control polygon as an argument (any
 * value passes through unchanged, 0 included): bit-identical to a host mirror path whose options
 * carry that radius. tpamd_planner_set_switch_paths is this entry with rounding 0.2. */
int tpamd_planner_set_switch_paths_rounded(tpamd_planner_set *set, int count, const int32_t *ids,
                                           const int64_t *time_ns, const double *keep_path_until,
                                           const int32_t *waypoint_offsets, const double *waypoints,
                                           double rounding, double *stop_parameter,
                                           int32_t *num_points, int32_t *status);
/* New waypoint paths for `count` planners of a set (ids[count], each listed once, or planners
 * 0..count-1 if ids is NULL), fitted on the device: TimeableJointSplinePath::SetWaypoints
 * (FitSplineToWaypoints, timeable_path_joint_spline.cc:199-206, :252-292) on planner k's waypoints
 * waypoints[waypoint_offsets[k] .. waypoint_offsets[k + 1])[D] with the PathOptions::rounding radius
 * `rounding` (0.2 is the default; any value passes through unchanged, 0 included), bit-identical to
 * the host mirror. Planner k then holds what tpamd_planner_set_upload_paths_ragged with path_state
 * 1 (kNewPath) leaves: the spline (max(3 W - 2, 4) control points), max_velocity[k] /
 * max_acceleration[k] / initial_velocity[k] [count][D] (initial_velocity NULL: zero) and delta[k];
 * the next tpamd_planner_set_plan plans it as a new path. Per planner: num_points[k] (may be NULL;
 * the planner's control points after the call, 0 for no path) and status[k] TPAMD_PLAN_*: a planner
 * with no waypoints gets TPAMD_PLAN_INVALID_ARGUMENT ("Control point vector empty.") and keeps its
 * state. Call-level errors change nothing: NULL set / waypoint_offsets / max_velocity /
 * max_acceleration / delta / status, NULL waypoints with rows, count < 0 or > B, a bad or repeated
 * id, waypoint_offsets[0] != 0 or decreasing. The set's per-planner capacity grows (by doubling)
 * before anything changes. Host pointers; synchronises. */
int tpamd_planner_set_set_waypoints(tpamd_planner_set *set, int count, const int32_t *ids,
                                    const int32_t *waypoint_offsets, const double *waypoints,
                                    double rounding, const double *max_velocity,
                                    const double *max_acceleration, const double *delta,
                                    const double *initial_velocity, int32_t *num_points,
                                    int32_t *status);
/* The same with waypoints, max_velocity, max_acceleration, delta, initial_velocity, num_points and
 * status device pointers; ids and waypoint_offsets stay HOST arrays: the id checks, the planners'
 * control-point counts and the capacity growth need them on the host before the launch (they go
 * up through pinned staging on hip_stream). Enqueues on hip_stream (NULL: the null stream) and does
 * not synchronise, except when the capacity grows (on the null stream, first) or the staging of
 * the previous call of this entry is still in use. Stream ordering as for the _device readouts
 * (tpamd_planner_set_download_trajectories_device): the fit starts after the set's last change and
 * the last device readout; the calls that change or read planner state on the null stream wait for
 * it, and so do later device readouts. */
int tpamd_planner_set_set_waypoints_device(tpamd_planner_set *set, int count, const int32_t *ids,
                                           const int32_t *waypoint_offsets, const double *waypoints,
                                           double rounding, const double *max_velocity,
                                           const double *max_acceleration, const double *delta,
                                           const double *initial_velocity, int32_t *num_points,
                                           int32_t *status, void *hip_stream);
/* Retargets `count` moving planners of a set (ids[count], each listed once, or planners 0..count-1
 * if ids is NULL) onto new waypoints, abandoning the old path at time_ns[k], in one launch on the
 * resident trajectories. Per listed planner, the reference's sequence (path_tools.h:44-53):
 *   1. position and velocity at time_ns[k] on the resident trajectory
 *      (TrajectoryBuffer::GetPositionAtTime / GetVelocityAtTime: TPAMD_PLAN_FAILED_PRECONDITION
 *      without a plan, TPAMD_PLAN_OUT_OF_RANGE outside it);
 *   2. ComputeStoppingPoint(position, velocity, stopping_acceleration[k], rounding) (path_tools.cc
 *      :25-74; stopping_acceleration [count][D] may be NULL: max_acceleration[k]); a non-positive
 *      limit gives TPAMD_PLAN_INVALID_ARGUMENT;
 *   3. TimeableJointSplinePath::SetWaypoints on [position, stopping point, waypoints
 *      [waypoint_offsets[k] .. waypoint_offsets[k + 1])[D]...] with the PathOptions::rounding radius
 *      `rounding`; a planner at rest (every |velocity| < 100 epsilon) gets [position, waypoints...].
 *      No waypoints (W = 0) is allowed: the path is the straight stop, or four copies of position;
 *   4. planner k then holds what tpamd_planner_set_set_waypoints leaves (path_state 1, kNewPath)
 *      with max_velocity[k] / max_acceleration[k] [count][D], delta[k] and the velocity of step 1 as
 *      initial velocity, bit-identical to the host mirror; the next tpamd_planner_set_plan plans it
 *      as a new path from time_ns[k] on.
 * Steps 1 and 2 run before anything is written: a planner that fails keeps its state bit for bit.
 * Per planner: status[k] TPAMD_PLAN_* (the first step that failed), num_points[k] (may be NULL; the
 * planner's control points after the call, 0 for no path) and, each [count][D] and each may be
 * NULL, position / velocity / stopping_point (for a planner at rest the position); the rows of a
 * planner that failed are not written. Call-level errors are those of
 * tpamd_planner_set_set_waypoints plus a NULL time_ns, and change nothing; a Cartesian set gives
 * TPAMD_E_UNSUPPORTED. The set's per-planner capacity grows first if max(3 (W + 2) - 2, 4) points
 * do not fit. Host pointers; synchronises. */
int tpamd_planner_set_retarget(tpamd_planner_set *set, int count, const int32_t *ids,
                               const int64_t *time_ns, const int32_t *waypoint_offsets,
                               const double *waypoints, double rounding, const double *max_velocity,
                               const double *max_acceleration, const double *delta,
                               const double *stopping_acceleration, int32_t *num_points,
                               int32_t *status, double *position, double *velocity,
                               double *stopping_point);
/* The same with time_ns, waypoints, max_velocity, max_acceleration, delta, stopping_acceleration,
 * num_points (required here), status, position, velocity and stopping_point device pointers; ids
 * and waypoint_offsets stay HOST arrays. Contract and stream ordering exactly as
 * tpamd_planner_set_set_waypoints_device: enqueues on hip_stream and does not synchronise, except
 * when the capacity grows or the previous call's staging is still in use. How many control points
 * a planner ends with is decided on the device: tpamd_planner_set_download_path reads the count
 * back (after this call has finished) the first time it is asked about such a planner. */
int tpamd_planner_set_retarget_device(tpamd_planner_set *set, int count, const int32_t *ids,
                                      const int64_t *time_ns, const int32_t *waypoint_offsets,
                                      const double *waypoints, double rounding,
                                      const double *max_velocity, const double *max_acceleration,
                                      const double *delta, const double *stopping_acceleration,
                                      int32_t *num_points, int32_t *status, double *position,
                                      double *velocity, double *stopping_point, void *hip_stream);
/* ---- path_tools.{h,cc} as batch calls -------------------------------------------------------
 * ComputeStoppingPoint (path_tools.cc:25-74) for `count` rows: position, velocity and
 * acceleration_limit [count][num_dofs], corner_rounding [count]. point [count][num_dofs] receives
 * where the robot can come to rest on the straight line along its velocity without exceeding the
 * limits, shifted further by the corner rounding (CornerOffset, splines/spline_utils.cc:25-45);
 * position itself if every |velocity| is below 100 epsilon. status [count] is TPAMD_PLAN_OK, or
 * TPAMD_PLAN_INVALID_ARGUMENT ("Acceleration limits must be strictly positive.") for a row whose
 * smallest limit is <= 0: its point is not written. Bit-identical to the host mirror
 * (host/path_tools.h); eigenmath::ScaleDownToLimits is restated as a uniform scaling
 * (INTEGRATION.md). Call-level errors write nothing: a NULL engine, count < 0, num_dofs < 1, a NULL
 * array with count > 0 (TPAMD_E_INVALID_ARGUMENT). Host pointers; synchronises. */
int tpamd_compute_stopping_points_host(tpamd_engine *engine, int count, int num_dofs,
                                       const double *position, const double *velocity,
                                       const double *acceleration_limit,
                                       const double *corner_rounding, double *point,
                                       int32_t *status);
/* The same with every array a device pointer. Enqueues one kernel on hip_stream (NULL: the null
 * stream) and does not synchronise. */
int tpamd_compute_stopping_points_device(tpamd_engine *engine, int count, int num_dofs,
                                         const double *position, const double *velocity,
                                         const double *acceleration_limit,
                                         const double *corner_rounding, double *point,
                                         int32_t *status, void *hip_stream);
/* ProjectPointOnPath (path_tools.h:56-100) for a ragged batch: list k is rows waypoint_offsets[k] ..
 * waypoint_offsets[k + 1]) of waypoints [rows][num_dofs], projected onto is point[k] [num_dofs].
 * Per list the fields of ProjectedPointResult: waypoint_index[k] (the closest segment's first
 * waypoint), distance_to_path[k], line_parameter[k] (limited to 1 above, not below: a negative
 * value says "before the first waypoint") and projected_point [count][num_dofs]; a single waypoint
 * gives index 0, parameter 0 and that waypoint. status[k] is TPAMD_PLAN_OK, or
 * TPAMD_PLAN_INVALID_ARGUMENT ("No waypoints.") for an empty list, whose outputs are not written.
 * Bit-identical to the host mirror. Call-level errors write nothing: a NULL engine or array,
 * count < 0, num_dofs < 1, waypoint_offsets[0] != 0 or decreasing offsets
 * (TPAMD_E_INVALID_ARGUMENT). Host pointers; synchronises. */
int tpamd_project_points_on_paths_host(tpamd_engine *engine, int count, int num_dofs,
                                       const int32_t *waypoint_offsets, const double *waypoints,
                                       const double *point, int32_t *waypoint_index,
                                       double *distance_to_path, double *line_parameter,
                                       double *projected_point, int32_t *status);
/* The same with every array except waypoint_offsets a device pointer. Enqueues on hip_stream and
 * does not synchronise; the offsets go up on hip_stream first, into the buffer the _device pose-fit
 * entries use (tpamd_fit_pose_waypoints_device), with the same ordering between such calls. */
int tpamd_project_points_on_paths_device(tpamd_engine *engine, int count, int num_dofs,
                                         const int32_t *waypoint_offsets, const double *waypoints,
                                         const double *point, int32_t *waypoint_index,
                                         double *distance_to_path, double *line_parameter,
                                         double *projected_point, int32_t *status,
                                         void *hip_stream);
/* ---- Cartesian planner sets --------------------------------------------------------------
 * A set of the second kind: every planner's path is the IK table of a TimeableCartesianSplinePath
 * (path_ik_positions_, one row per multiple of delta_parameter, timeable_path_cartesian_spline.cc
 * :464-549, plus the Jacobian at each row). The IK and Jacobian callbacks are user code and run
 * before the upload; tpamd_planner_set_plan then plans entirely on the device: a window is rows
 * PathIkIndex(path_start) .. +N-1 of the resident table (SamplePath :527-542), differenced
 * (:39-68) and turned into 2D+2 constraint rows (:551-595). A planner whose table does not hold
 * its window gets TPAMD_PLAN_INTERNAL; the others are unaffected. A set holds one kind: the
 * joint-spline entries (upload_paths[_ragged], download_path, switch_paths, set_waypoints[_device])
 * return TPAMD_E_INVALID_ARGUMENT on a Cartesian set and change nothing, and so do the IK-table
 * entries on a joint set. Every other tpamd_planner_set_* entry and
 * tpamd_buffer_set_insert_from_planner_set[_device] work on both kinds.
 *
 * create_cartesian takes the same config (num_points is ignored); table_capacity (>= 1) is the
 * number of table rows per planner to start with. It grows by doubling, with a copy, before
 * anything else changes. */
int tpamd_planner_set_create_cartesian(tpamd_engine *engine, const tpamd_planner_set_config *config,
                                       int table_capacity, tpamd_planner_set **out);
/* The IK tables of `count` planners (ids[count], each listed once, or planners 0..count-1 if ids is
 * NULL). Planner k's table is rows row_offsets[k] .. row_offsets[k + 1]) of ik_positions [rows][D]
 * and jacobians [rows][6][D] (row-major, the layout of tpamd_cartesian_inputs); row r belongs to
 * path parameter r * delta[k]. path_end[k] is knots.back() (what CloseToEnd compares against);
 * max_velocity / max_acceleration / initial_velocity [count][D] (initial_velocity NULL: zero),
 * max_translational_velocity / max_rotational_velocity / delta [count]; path_state[k] 1 (kNewPath)
 * or 2 (kModifiedPath) as in tpamd_planner_set_upload_paths. Every id, state and size is checked
 * before the first copy: a NULL array, count < 0 or > B, a bad or repeated id, a state other than
 * 1 or 2, row_offsets[0] != 0 or decreasing, a planner with fewer than num_samples rows or
 * delta <= 0 fail the call and change nothing. Host pointers; synchronises. The tables are staged
 * in device memory for the call; staging above 16 MiB is freed before it returns. */
int tpamd_planner_set_upload_ik_tables(tpamd_planner_set *set, int count, const int32_t *ids,
                                       const int32_t *row_offsets, const double *ik_positions,
                                       const double *jacobians, const double *path_end,
                                       const double *max_velocity, const double *max_acceleration,
                                       const double *max_translational_velocity,
                                       const double *max_rotational_velocity, const double *delta,
                                       const double *initial_velocity, const int32_t *path_state);
/* The same with ik_positions .. initial_velocity and path_state device pointers; ids and row_offsets
 * stay HOST arrays (the checks and the capacity growth need them before the launch; they go up
 * through pinned staging on hip_stream). delta[k] and path_state[k] cannot be checked on the host
 * here; the kernel checks them: a planner whose delta is not > 0 or whose state is not 1 / 2 is left
 * WITHOUT a path (its Plan gives TPAMD_PLAN_FAILED_PRECONDITION; a path it had before is gone)
 * while the others are loaded. Its rows are written all the same, and
 * tpamd_planner_set_download_ik_table returns what was uploaded, whether the kernel accepted the
 * planner or not. Enqueues on hip_stream and does not synchronise,
 * except when the capacity grows or the previous call's staging is still in use. Stream ordering
 * as documented for tpamd_planner_set_set_waypoints_device. */
int tpamd_planner_set_upload_ik_tables_device(tpamd_planner_set *set, int count, const int32_t *ids,
                                              const int32_t *row_offsets, const double *ik_positions,
                                              const double *jacobians, const double *path_end,
                                              const double *max_velocity, const double *max_acceleration,
                                              const double *max_translational_velocity,
                                              const double *max_rotational_velocity, const double *delta,
                                              const double *initial_velocity, const int32_t *path_state,
                                              void *hip_stream);
/* ---- Streaming IK tables: plan, suspend, append ---------------------------------------------
 * A table need not cover its whole path. TimeableCartesianSplinePath::SamplePath extends
 * path_ik_positions_ lazily (:464-549): each window asks the IK callback only for the rows between
 * the table's last row and the window's last row. The streaming entries do the same for a set:
 *
 *   upload_ik_tables[_device]   rows 0 .. N-1 (or more) of every path
 *   plan_streaming              Plan; a planner whose next window is not resident WAITS
 *   while (num_waiting > 0):
 *     append_ik_rows[_device]   rows need_first[b] .. need_first[b] + need_count[b] - 1 (or more)
 *     plan_resume               the waiting planners re-enter the window loop where they stopped
 *
 * append_ik_rows: planner ids[k] (each listed once; ids NULL: 0..count-1) gets rows
 * row_offsets[k] .. row_offsets[k + 1]) of ik_positions [rows][D] / jacobians [rows][6][D] behind
 * its last resident row; a count of 0 is allowed. Limits, delta, path_end and the path state stay
 * as they are. The capacity grows by doubling, with a copy, before anything else changes. A joint
 * set, a NULL array, count < 0 or > B, a bad or repeated id, row_offsets[0] != 0 or decreasing, or
 * a planner that has no table as far as the host knows fail the call and change nothing. A planner
 * whose table the kernel rejected at a _device upload is left untouched by the kernel (the
 * destination row is the device's own row count; for such a planner
 * tpamd_planner_set_download_ik_table keeps reporting what the host was handed, as after the
 * rejected upload itself). Host pointers; synchronises. */
int tpamd_planner_set_append_ik_rows(tpamd_planner_set *set, int count, const int32_t *ids,
                                     const int32_t *row_offsets, const double *ik_positions,
                                     const double *jacobians);
/* The same with ik_positions and jacobians device pointers; ids and row_offsets stay HOST arrays.
 * Enqueues on hip_stream and does not synchronise, except when the capacity grows or the previous
 * call's staging is still in use. Stream ordering as for tpamd_planner_set_upload_ik_tables_device:
 * the next Plan / resume (null stream) waits for it. */
int tpamd_planner_set_append_ik_rows_device(tpamd_planner_set *set, int count, const int32_t *ids,
                                            const int32_t *row_offsets, const double *ik_positions,
                                            const double *jacobians, void *hip_stream);
/* tpamd_planner_set_plan with suspension (Cartesian sets only; TPAMD_E_INVALID_ARGUMENT on a joint
 * set). A planner whose next window is well formed but reaches past its table's last row does not
 * fail: its summary record carries TPAMD_PLAN_NEEDS_ROWS and the windows solved so far, its
 * trajectory, end time and final deceleration start stay as the call's prologue and its finished
 * windows left them, and need_first[b] / need_count[b] name the rows it lacks (need_first is the
 * table's row count; after the append the table has need_first + need_count rows, the size
 * SamplePath leaves it with). The other planners are not held up. need_first / need_count [B]
 * (host, may be NULL) are 0 / 0 for planners that do not wait; *num_waiting (may be NULL) counts
 * those that do. A window that no table can hold still gives TPAMD_PLAN_INTERNAL. Down: what
 * tpamd_planner_set_plan moves plus 8 bytes per planner. */
int tpamd_planner_set_plan_streaming(tpamd_planner_set *set, const int64_t *start_ns,
                                     const int64_t *horizon_ns, tpamd_planner_summary *summary,
                                     int32_t *need_first, int32_t *need_count, int32_t *num_waiting);
/* Re-enters the window loop for the planners that wait. Legal only while planners wait (otherwise
 * TPAMD_E_INVALID_ARGUMENT, nothing changes). A waiting planner whose table now holds its window
 * goes on with the loop state of the suspending call -- its start and horizon arguments, the loop's
 * start time, the windows and iterations counted so far (max_planning_iterations counts across
 * suspensions) -- and, when it finishes, reports what an uninterrupted Plan would report; it may
 * wait again at a later window. One still short of rows keeps waiting with a fresh need. Summary
 * records of planners that were not waiting repeat the previous call's. Nothing goes up.
 *
 * Dropping a suspension: any other tpamd_planner_set_plan / _plan_streaming, an upload_ik_tables*
 * that lists the planner, or tpamd_planner_set_reset drop it without error. The planner is then in
 * the state of a reference planner whose Plan returned an error in that window: the windows it
 * finished are in its history, its trajectory is cut at the Plan's start time. (This describes the
 * state; the reference has no suspension to compare with.) */
int tpamd_planner_set_plan_resume(tpamd_planner_set *set, tpamd_planner_summary *summary,
                                  int32_t *need_first, int32_t *need_count, int32_t *num_waiting);
/* The resident table of one planner: *rows (0: no table) and, if the arrays are not NULL,
 * ik_positions [rows][D] and jacobians [rows][6][D]. `capacity` is the number of rows the arrays
 * can hold; a longer table gives TPAMD_E_INVALID_ARGUMENT (*rows is still written). For a planner
 * whose front rows were discarded (first_row > 0, below) it writes *rows, the path rows supplied
 * so far, and returns TPAMD_E_INVALID_ARGUMENT: it cannot deliver rows from 0;
 * tpamd_planner_set_download_ik_rows reads such a table. */
int tpamd_planner_set_download_ik_table(tpamd_planner_set *set, int planner, int32_t *rows,
                                        double *ik_positions, double *jacobians, int capacity);
/* ---- Streaming IK tables: discarding the consumed rows ---------------------------------------
 * A receding-horizon planner never reads a table row again once its trajectory has moved past it.
 * Every planner has a first resident row, first_row[b]: the table holds path rows first_row ..
 * rows - 1, `rows` keeps counting the path rows supplied since the upload (need_first / need_count
 * and the append entries keep speaking in path rows), and rows - first_row rows are live. first_row
 * is 0 after create, upload_ik_tables[_device] and reset, and a set on which discard_ik_rows is
 * never called behaves, allocates and reports as before. With the discard in the loop,
 *
 *   plan_streaming / append_ik_rows / plan_resume      as above
 *   discard_ik_rows(keep_from = NULL)                  after each completed Plan
 *
 * a table's footprint stays at the rows one Plan reads instead of growing to the whole path: the
 * allocation is never shrunk, but an append whose rows fit into capacity - live rows does not
 * reallocate, and a growth copies the live rows only.
 *
 * discard_ik_rows: planner ids[k] (each listed once; ids NULL: 0..count-1) keeps path rows from
 * keep_from[k] on; its live rows move to the front of its table, in place, on the device.
 * keep_from NULL: every listed planner keeps the rows from its safe floor on, the lowest row any
 * later Plan or resume of that planner can read, computed on the device from its window history:
 * PathIkIndex of the path parameter at start_time_, the start of its last Plan, before which
 * HandleTimeArguments accepts no later start; 0 for a new path or a planner that has not planned.
 * An explicit keep_from is the caller's responsibility and may lie above the floor: a planner
 * whose next window starts below its first resident row gets TPAMD_PLAN_INTERNAL, that planner
 * alone, and stays so until upload_ik_tables* gives it a table from row 0 again (an append only goes
 * behind the last row). keep_from is clamped on the device to [first_row, rows - 1]: a value at or
 * below first_row changes nothing for that planner, and the last resident row is never discarded,
 * since the streaming chain seeds the next extension's IK with it. The call is legal while planners
 * wait for rows. It synchronises; first_row_out [count] (host, may be NULL) receives the new first
 * rows: 4 bytes per listed planner come down, the ids (and keep_from) go up. A joint set, count < 0
 * or > B, a bad or repeated id, or a planner that has no table as far as the host knows fail the
 * call, before the first launch, and change nothing. A planner whose table the kernel rejected at a
 * _device upload is left untouched. */
int tpamd_planner_set_discard_ik_rows(tpamd_planner_set *set, int count, const int32_t *ids,
                                      const int32_t *keep_from, int32_t *first_row_out);
/* Host bookkeeping of one planner's table, no device access: *first_row, *rows (path rows supplied;
 * 0 / 0: no table) and *capacity (table rows allocated per planner, the same for every planner).
 * Each pointer may be NULL. TPAMD_E_INVALID_ARGUMENT on a joint set or a bad planner index. */
int tpamd_planner_set_ik_table_info(const tpamd_planner_set *set, int planner, int32_t *first_row,
                                    int32_t *rows, int32_t *capacity);
/* The live rows of one planner's table: *first_row, *rows_live = rows - first_row (0: no table) and,
 * if the arrays are not NULL, ik_positions [rows_live][D] and jacobians [rows_live][6][D], path rows
 * first_row .. rows - 1. `capacity` is the number of rows the arrays can hold; more live rows give
 * TPAMD_E_INVALID_ARGUMENT (*first_row and *rows_live are still written). */
int tpamd_planner_set_download_ik_rows(tpamd_planner_set *set, int planner, int32_t *first_row,
                                       int32_t *rows_live, double *ik_positions, double *jacobians,
                                       int capacity);
/* The device addresses of the tables, [B][capacity][D] and [B][capacity][6][D] (either pointer may
 * be NULL); planner b's path row r is in slot r - first_row[b]. They change when the capacity grows
 * and only then, so a caller can tell that an append did not reallocate. Read-only. */
int tpamd_planner_set_ik_table_device_pointers(const tpamd_planner_set *set,
                                               const double **ik_positions,
                                               const double **jacobians);
/* TrajectoryPlanner::Reset for the listed planners (ids NULL: all): no path, no plan. */
int tpamd_planner_set_reset(tpamd_planner_set *set, int count, const int32_t *ids);
/* Plan(start, time_horizon) for every planner: start_ns / horizon_ns [B] host arrays;
 * summary [B] (host, may be NULL) receives one record per planner, status included. */
int tpamd_planner_set_plan(tpamd_planner_set *set, const int64_t *start_ns, const int64_t *horizon_ns,
                           tpamd_planner_summary *summary);
/* Capacity ahead of time. tpamd_planner_set_capacity: samples per planner the history and the
 * trajectory buffers hold now (either pointer may be NULL; no device access).
 * tpamd_planner_set_reserve grows them to at least history_capacity / trajectory_capacity samples
 * per planner, exactly as a synchronous Plan grows them when a planner needs room: it never
 * shrinks, a value <= the current size (0 included) leaves that buffer alone, and every planner's
 * state is kept bit for bit. It also sizes the engine's workspace for this set's windows, so that
 * a tpamd_planner_set_plan_device that follows allocates nothing. Host call; synchronises when
 * anything grows. Values above 2^28 give TPAMD_E_UNSUPPORTED. */
int tpamd_planner_set_capacity(const tpamd_planner_set *set, int32_t *history, int32_t *trajectory);
int tpamd_planner_set_reserve(tpamd_planner_set *set, int history_capacity, int trajectory_capacity);

typedef struct tpamd_plan_device_info {   /* 32 bytes, written once per call, device memory */
  int32_t num_ok, num_failed;      /* planners with status TPAMD_PLAN_OK / any other status */
  int32_t num_exhausted;           /* of the failed: TPAMD_PLAN_RESOURCE_EXHAUSTED */
  int32_t needed_history;          /* largest count + N a stopped planner asked for, 0 if none */
  int32_t needed_trajectory;       /* largest resample count that did not fit, 0 if none */
  int32_t max_windows_solved;      /* largest `windows` of any planner */
  int32_t reserved[2];
} tpamd_plan_device_info;
/* tpamd_planner_set_plan, enqueued only: start_ns / horizon_ns [B] are DEVICE arrays, summary [B]
 * (may be NULL) and info (may be NULL) are device memory, all of them valid until hip_stream (NULL:
 * the null stream) has run the call. Nothing is copied to the host, nothing blocks, and
 * tpamd_planner_set_last_plan_bytes reports 0 / 0 afterwards.
 * The host cannot ask whether a planner still loops, so the window loop is bounded by the caller:
 * exactly max_windows (>= 1) window iterations are enqueued, and every planner is left as
 * tpamd_planner_set_plan leaves it on a set whose max_planning_iterations is
 * min(config value, max_windows - 1) -- path state, history, planner scalars, resident trajectory,
 * status and summary record, bit for bit. A planner that still loops in the last iteration gets
 * TPAMD_PLAN_DEADLINE_EXCEEDED as there (:655-658); planners that do not loop take no part in an
 * iteration (the solver skips their paths), so a max_windows larger than needed costs the launches
 * of the empty iterations and nothing else.
 * Nothing is allocated or grown by the call; a shortage is decided per planner on the device:
 *   * a looping planner whose history has no room for one more window (history_count +
 *     num_samples > history capacity) stops looping with TPAMD_PLAN_RESOURCE_EXHAUSTED and, like
 *     any planner whose loop ended in an error, is neither resampled nor finished;
 *   * a planner whose resampled trajectory exceeds the trajectory capacity gets
 *     TPAMD_PLAN_RESOURCE_EXHAUSTED and an EMPTY resident trajectory (num_samples 0: a truncated
 *     trajectory does not end at rest and must never be read out); its scalars are those of a
 *     plan without samples, so its next Plan fails with TPAMD_PLAN_FAILED_PRECONDITION.
 * No array is written out of bounds and no other planner is affected. info->needed_history /
 * needed_trajectory are what tpamd_planner_set_reserve would have needed; the recovery is
 * reserve, then tpamd_planner_set_reset and a new path (or a retarget) for those planners.
 * Call tpamd_planner_set_reserve once before the first call (a Plan that ran before has sized the
 * workspace as well): otherwise the first call allocates the engine's workspace and may block.
 * Joint sets and Cartesian sets with resident tables; on a Cartesian set a window that is not
 * resident gives that planner TPAMD_PLAN_INTERNAL as in tpamd_planner_set_plan, and suspensions
 * left by a streaming Plan are dropped. Streaming needs the host for rows and has no _device entry.
 * Stream ordering, as for tpamd_planner_set_set_waypoints_device: the call starts after the set's
 * last change and after the device readouts in flight; later null-stream calls on the set (every
 * host entry) and later device readouts on any stream wait for it. The engine's workspace is busy
 * until the call has run: any later solve on the same engine, for this set or another, on any
 * stream, is ordered behind it by the library. The caller synchronises only to read summary / info
 * or its own outputs. Not for hipGraph capture.
 * Call-level errors change nothing: a NULL set / start_ns / horizon_ns, max_windows < 1
 * (TPAMD_E_INVALID_ARGUMENT). */
int tpamd_planner_set_plan_device(tpamd_planner_set *set, const int64_t *start_ns,
                                  const int64_t *horizon_ns, int max_windows,
                                  tpamd_planner_summary *summary, tpamd_plan_device_info *info,
                                  void *hip_stream);
/* The trajectory of one planner after its last Plan: samples first .. first + count - 1 of
 * GetTime / GetPathParameters / ...Derivatives [count] and GetPositions / GetVelocities /
 * GetAccelerations [count][D] into host arrays (any may be NULL). */
int tpamd_planner_set_download_trajectory(tpamd_planner_set *set, int planner, int first, int count,
                                          double *time, double *s, double *sd, double *sdd,
                                          double *q, double *qd, double *qdd);
/* Setpoints at control ticks. For listed planner k (ids[k], or k if ids is NULL; repeats allowed)
 * and tick j < num_ticks, time_ns = start_ns[k] + j * step_ns (converted as (double)ns / 1e9 like
 * the rest of the set). Outputs are TrajectoryBuffer::Get{Position,Velocity,Acceleration}AtTime
 * (trajectory_buffer.cc:228-294: the upper_bound bracket, then InterpolateLinear; at the last
 * sample that sample) on the planner's resident trajectory, in q / qd / qdd [count][num_ticks][D]
 * (any of them may be NULL), and status [count][num_ticks]: TPAMD_PLAN_OK,
 * TPAMD_PLAN_FAILED_PRECONDITION (no samples: never planned, or reset) or TPAMD_PLAN_OUT_OF_RANGE
 * (before the first or after the last sample, or a tick time that overflows int64). The values of
 * a tick that is not OK are left untouched. No planner state changes.
 * Call-level errors change nothing: a NULL set / start_ns / status, count < 0, count > B with a
 * NULL ids, step_ns <= 0, num_ticks < 1, and in this host variant an id out of range (every id is
 * checked before the first copy). One copy up, one launch, one copy down per requested array.
 * Host pointers; synchronises. */
int tpamd_planner_set_sample_at_ticks(tpamd_planner_set *set, int count, const int32_t *ids,
                                      const int64_t *start_ns, int64_t step_ns, int num_ticks,
                                      double *q, double *qd, double *qdd, int32_t *status);
/* The same with every array (ids, start_ns, q, qd, qdd, status) a device pointer. Only enqueues on
 * hip_stream (NULL: the null stream) and does not synchronise. ids are checked in the kernel: an
 * id out of range gives TPAMD_PLAN_INVALID_ARGUMENT for each of its ticks. Stream ordering: see
 * tpamd_planner_set_download_trajectories_device. */
int tpamd_planner_set_sample_at_ticks_device(tpamd_planner_set *set, int count, const int32_t *ids,
                                             const int64_t *start_ns, int64_t step_ns, int num_ticks,
                                             double *q, double *qd, double *qdd, int32_t *status,
                                             void *hip_stream);
/* The trajectories of the listed planners (ids[count], repeats allowed, or planners 0..count-1 if
 * ids is NULL), packed: planner k's samples fill rows offsets[k] .. offsets[k+1) of time / s / sd /
 * sdd [rows] and q / qd / qdd [rows][D] (any may be NULL), as tpamd_planner_set_download_trajectory
 * gives them one planner at a time. offsets [count + 1] is always written. If offsets[count] >
 * capacity (rows the arrays hold), no row is written and this host variant returns
 * TPAMD_E_INVALID_ARGUMENT: the caller grows its arrays to offsets[count] and calls again.
 * Call-level errors as for tpamd_planner_set_sample_at_ticks (NULL offsets, capacity < 0).
 * ids up, one scan, offsets down, one pack, one copy down per requested array. Host pointers;
 * synchronises. No planner state changes. */
int tpamd_planner_set_download_trajectories(tpamd_planner_set *set, int count, const int32_t *ids,
                                            int64_t *offsets, int64_t capacity, double *time,
                                            double *s, double *sd, double *sdd, double *q,
                                            double *qd, double *qdd);
/* The same with ids, offsets and the arrays on the device; enqueues on hip_stream and does not
 * synchronise. It cannot know the total when it returns: if offsets[count] > capacity the rows stay
 * unwritten, and the caller reads offsets[count] before using them. An id out of range gets an
 * empty row range.
 * Stream ordering of the two _device readouts with the set's other calls, whatever hip_stream is
 * (a non-blocking stream included): a readout sees the set's last change (the changing calls
 * enqueue on the null stream and synchronise before they return; the readout's stream also waits
 * on an event recorded on the null stream when it is enqueued). The calls that change planner
 * state (upload_paths*, switch_paths, reset, plan) make the null stream wait on an event recorded
 * after the last device readout before their first copy or launch, so they never overwrite a
 * trajectory a readout is still reading; successive device readouts on different streams are
 * chained the same way. The set must outlive the readouts' use of its trajectories until then
 * (tpamd_planner_set_destroy waits for them). */
int tpamd_planner_set_download_trajectories_device(tpamd_planner_set *set, int count,
                                                   const int32_t *ids, int64_t *offsets,
                                                   int64_t capacity, double *time, double *s,
                                                   double *sd, double *sdd, double *q, double *qd,
                                                   double *qdd, void *hip_stream);
/* TrajectoryBuffer::StopBeforeTime(TimeToSec(time_ns[k]), max_acceleration[k], time_step)
 * (trajectory_buffer.cc:296-385, as tpamd_stop_trajectories_*) on the resident trajectory of each
 * listed planner (ids[count], repeats allowed, or planners 0..count-1 if ids is NULL), as if it
 * were loaded into a TrajectoryBuffer (default timestep_tolerance 1e-6): status[k] TPAMD_PLAN_*,
 * keep[k] (samples of the trajectory kept before the segment) and the segment, packed: planner k's
 * rows fill offsets[k] .. offsets[k+1) of time [rows] and q / qd / qdd [rows][D] (any may be NULL).
 * The stopped trajectory is the planner's first keep[k] samples followed by those rows. A planner
 * without samples gives TPAMD_PLAN_OK, keep 0 and no rows; a stop that fails gives keep = its
 * sample count and no rows. max_acceleration [count][D]. offsets [count + 1], status and keep are
 * always written; if offsets[count] > capacity no row is written and this host variant returns
 * TPAMD_E_INVALID_ARGUMENT (grow to offsets[count] and call again). Call-level errors (NULL set /
 * time_ns / max_acceleration / status / keep / offsets, count < 0, count > B with a NULL ids,
 * capacity < 0, an id out of range) change nothing. No planner state changes: the next Plan is
 * the one it would have been without this call. Host pointers; synchronises. */
int tpamd_planner_set_stop_trajectories(tpamd_planner_set *set, int count, const int32_t *ids,
                                        const int64_t *time_ns, const double *max_acceleration,
                                        double time_step, int32_t *status, int32_t *keep,
                                        int64_t *offsets, int64_t capacity, double *time, double *q,
                                        double *qd, double *qdd);
/* The same with every array a device pointer; enqueues on hip_stream and does not synchronise.
 * An id out of range gives TPAMD_PLAN_INVALID_ARGUMENT, keep 0 and no rows. If offsets[count] >
 * capacity the rows stay unwritten. Stream ordering as for the _device readouts
 * (tpamd_planner_set_download_trajectories_device). */
int tpamd_planner_set_stop_trajectories_device(tpamd_planner_set *set, int count, const int32_t *ids,
                                               const int64_t *time_ns, const double *max_acceleration,
                                               double time_step, int32_t *status, int32_t *keep,
                                               int64_t *offsets, int64_t capacity, double *time,
                                               double *q, double *qd, double *qdd, void *hip_stream);
/* Bytes the last tpamd_planner_set_plan call moved over PCIe (host to device, device to host);
 * 0 / 0 after tpamd_planner_set_plan_device. */
void tpamd_planner_set_last_plan_bytes(const tpamd_planner_set *set, size_t *host_to_device,
                                       size_t *device_to_host);
/* Device memory the set holds: its state, and the staging of the switch and the host readouts,
 * which grows as calls need it. */
size_t tpamd_planner_set_device_bytes(const tpamd_planner_set *set);

/* ---- buffer sets: B TrajectoryBuffers resident on the device -------------------------------
 * A buffer set keeps B TrajectoryBuffers (trajectory_buffer.{h,cc}) of D joints on the device:
 * per buffer the samples (time, q, qd, qdd), the sample count and the sequence number. Every
 * operation takes a list of buffers (ids[count], or buffers 0..count-1 if ids is NULL), runs in one
 * launch and leaves each listed buffer as the same call on a TrajectoryBuffer would, bit for bit.
 * Per-buffer outcomes are TPAMD_PLAN_* in status[count].
 *
 * Host-pointer entries take host arrays, run on the null stream and synchronise. Call-level errors
 * (TPAMD_E_*: a NULL set or required array, count < 0, count > B with a NULL ids, an id out of
 * range, and in a call that changes buffers a buffer listed twice) change nothing; every id is
 * checked before the first copy. Entries that add samples grow the set's per-buffer capacity (by
 * doubling) before anything changes.
 * _device entries take device pointers for every array, ids included, only enqueue on hip_stream
 * (NULL: the null stream) and never allocate or synchronise, so after tpamd_buffer_set_reserve
 * they can be captured in a hipGraph and replayed with other lists (the exception is
 * tpamd_buffer_set_insert_from_planner_set_device, see there). An id out of range gets
 * TPAMD_PLAN_INVALID_ARGUMENT in the kernel; listing a buffer twice in a call that changes buffers
 * is outside the contract. A listed buffer whose result would not fit the capacity gets
 * TPAMD_PLAN_MORE and is left unchanged. status may be NULL where nothing but the id check can
 * fail (discard_before, add_offset, clear, info). Calls on one stream are ordered by that stream;
 * the caller orders calls on different streams. */
typedef struct tpamd_buffer_set tpamd_buffer_set;

/* num_buffers >= 1, num_dofs in [1, 16], capacity rows per buffer (0: 256), timestep_tolerance > 0
 * (TrajectoryBuffer::Create rejects the others: TPAMD_E_INVALID_ARGUMENT). The set must not
 * outlive the engine. */
int tpamd_buffer_set_create(tpamd_engine *engine, int num_buffers, int num_dofs, int capacity,
                            double timestep_tolerance, tpamd_buffer_set **out);
/* Waits for the device before it frees the set. */
void tpamd_buffer_set_destroy(tpamd_buffer_set *set);
/* At least `capacity` rows per buffer (TrajectoryBuffer::Reserve); contents unchanged.
 * Synchronises the device. */
int tpamd_buffer_set_reserve(tpamd_buffer_set *set, int capacity);
int tpamd_buffer_set_capacity(const tpamd_buffer_set *set);
/* Device memory the set holds: its state and the staging of the host-pointer entries. _device
 * entries never change it. */
size_t tpamd_buffer_set_device_bytes(const tpamd_buffer_set *set);

/* InsertSegment (trajectory_buffer.cc:79-133). Listed buffer k receives rows offsets[k] ..
 * offsets[k+1) of time [rows] and q / qd / qdd [rows][D]: the packed layout that
 * tpamd_planner_set_download_trajectories* and tpamd_planner_set_stop_trajectories* write. The
 * sequence number goes up (an empty segment included) and back to 0 when the segment replaces the
 * whole buffer. status: TPAMD_PLAN_OK. offsets must not decrease (call-level error). Up: offsets,
 * the rows, ids in one copy; down: status. */
int tpamd_buffer_set_insert(tpamd_buffer_set *set, int count, const int32_t *ids, const int64_t *offsets,
                            const double *time, const double *q, const double *qd, const double *qdd,
                            int32_t *status);
/* The same on the device; `capacity` is the number of rows the arrays hold. An entry whose row
 * range is negative or ends behind `capacity` (a producer that ran out of room leaves its rows
 * unwritten and offsets[count] > capacity) gets TPAMD_PLAN_INVALID_ARGUMENT, a buffer without room
 * TPAMD_PLAN_MORE; both leave the buffer unchanged. */
int tpamd_buffer_set_insert_device(tpamd_buffer_set *set, int count, const int32_t *ids,
                                   const int64_t *offsets, int64_t capacity, const double *time,
                                   const double *q, const double *qd, const double *qdd, int32_t *status,
                                   void *hip_stream);
/* InsertSegment of the resident trajectory of planner planner_ids[k] (NULL: planner k) of a
 * planner set on the same engine and with the same D into listed buffer k, device to device:
 * nothing crosses PCIe but the lists and the statuses. A planner without samples is an empty
 * segment. Call-level errors also: another engine or D, a planner out of range. */
int tpamd_buffer_set_insert_from_planner_set(tpamd_buffer_set *set, tpamd_planner_set *planners, int count,
                                             const int32_t *ids, const int32_t *planner_ids,
                                             int32_t *status);
/* The same with ids, planner_ids and status on the device; a planner out of range gets
 * TPAMD_PLAN_INVALID_ARGUMENT. It counts as a device readout of the planner set and joins its
 * event chain (tpamd_planner_set_download_trajectories_device): it records and waits on the
 * planner set's events, so a later Plan cannot overwrite a trajectory it is still reading. That
 * event record is on the null stream: this entry is not meant to be captured in a graph. */
int tpamd_buffer_set_insert_from_planner_set_device(tpamd_buffer_set *set, tpamd_planner_set *planners,
                                                    int count, const int32_t *ids,
                                                    const int32_t *planner_ids, int32_t *status,
                                                    void *hip_stream);
/* AppendSample (:135-149): time [count], q / qd / qdd [count][D]. status TPAMD_PLAN_OK, or
 * TPAMD_PLAN_INVALID_ARGUMENT unless the time is after the buffer's last sample. */
int tpamd_buffer_set_append_sample(tpamd_buffer_set *set, int count, const int32_t *ids, const double *time,
                                   const double *q, const double *qd, const double *qdd, int32_t *status);
int tpamd_buffer_set_append_sample_device(tpamd_buffer_set *set, int count, const int32_t *ids,
                                          const double *time, const double *q, const double *qd,
                                          const double *qdd, int32_t *status, void *hip_stream);
/* DiscardSegmentBefore (:151-208) at time_ns[k] (converted as (double)ns / 1e9) or time_sec[k]:
 * exactly one of the two arrays is given. No sample moves: the buffer's first row advances, and
 * the new first sample is the interpolated state where the reference creates one. A time after
 * the last sample clears the buffer, sequence number included. */
int tpamd_buffer_set_discard_before(tpamd_buffer_set *set, int count, const int32_t *ids,
                                    const int64_t *time_ns, const double *time_sec);
int tpamd_buffer_set_discard_before_device(tpamd_buffer_set *set, int count, const int32_t *ids,
                                           const int64_t *time_ns, const double *time_sec, int32_t *status,
                                           void *hip_stream);
/* StopBeforeTime (:296-385) that changes the buffer: the samples from the kept count on become
 * the tail time-scaled to rest, and count and sequence number follow InsertSegment; on the last
 * sample at rest only its velocity and acceleration are zeroed. status as
 * tpamd_planner_set_stop_trajectories (TPAMD_PLAN_INTERNAL where the reference aborts); a stop
 * that fails leaves the buffer untouched. max_acceleration [count][D]. A stop never needs more
 * rows than the buffer holds. */
int tpamd_buffer_set_stop_before_time(tpamd_buffer_set *set, int count, const int32_t *ids,
                                      const int64_t *time_ns, const double *time_sec,
                                      const double *max_acceleration, double time_step, int32_t *status);
int tpamd_buffer_set_stop_before_time_device(tpamd_buffer_set *set, int count, const int32_t *ids,
                                             const int64_t *time_ns, const double *time_sec,
                                             const double *max_acceleration, double time_step,
                                             int32_t *status, void *hip_stream);
/* Get{Position,Velocity,Acceleration}AtTime at ticks start_ns[k] + j step_ns: arguments, outputs
 * and statuses as tpamd_planner_set_sample_at_ticks, on the buffers (repeats allowed). */
int tpamd_buffer_set_sample_at_ticks(tpamd_buffer_set *set, int count, const int32_t *ids,
                                     const int64_t *start_ns, int64_t step_ns, int num_ticks, double *q,
                                     double *qd, double *qdd, int32_t *status);
int tpamd_buffer_set_sample_at_ticks_device(tpamd_buffer_set *set, int count, const int32_t *ids,
                                            const int64_t *start_ns, int64_t step_ns, int num_ticks,
                                            double *q, double *qd, double *qdd, int32_t *status,
                                            void *hip_stream);
/* AddOffsetToTimestamps (:387-393): offset_sec[k], or offset_ns[k] / 1e9 (a duration); exactly one
 * of the two arrays is given. */
int tpamd_buffer_set_add_offset(tpamd_buffer_set *set, int count, const int32_t *ids,
                                const int64_t *offset_ns, const double *offset_sec);
int tpamd_buffer_set_add_offset_device(tpamd_buffer_set *set, int count, const int32_t *ids,
                                       const int64_t *offset_ns, const double *offset_sec, int32_t *status,
                                       void *hip_stream);
/* Clear (:64-70): no samples, sequence number 0. */
int tpamd_buffer_set_clear(tpamd_buffer_set *set, int count, const int32_t *ids);
int tpamd_buffer_set_clear_device(tpamd_buffer_set *set, int count, const int32_t *ids, int32_t *status,
                                  void *hip_stream);
/* GetNumSamples, GetSequenceNumber, GetStartTime and GetEndTime (nanoseconds; :50-62: both 0 for
 * an empty buffer) and, if time_ns is given, the size of GetPositionsUpToTime(time_ns[k])
 * (:210-226) of each listed buffer (repeats allowed). Any output may be NULL. */
int tpamd_buffer_set_info(tpamd_buffer_set *set, int count, const int32_t *ids, const int64_t *time_ns,
                          int32_t *num_samples, int32_t *sequence, int64_t *start_ns, int64_t *end_ns,
                          int32_t *positions_up_to);
int tpamd_buffer_set_info_device(tpamd_buffer_set *set, int count, const int32_t *ids, const int64_t *time_ns,
                                 int32_t *num_samples, int32_t *sequence, int64_t *start_ns, int64_t *end_ns,
                                 int32_t *positions_up_to, void *hip_stream);
/* The samples of the listed buffers (repeats allowed), packed as
 * tpamd_planner_set_download_trajectories packs trajectories: offsets [count + 1] always written,
 * rows only if offsets[count] <= capacity (host variant: TPAMD_E_INVALID_ARGUMENT otherwise). */
int tpamd_buffer_set_download(tpamd_buffer_set *set, int count, const int32_t *ids, int64_t *offsets,
                              int64_t capacity, double *time, double *q, double *qd, double *qdd);
int tpamd_buffer_set_download_device(tpamd_buffer_set *set, int count, const int32_t *ids, int64_t *offsets,
                                     int64_t capacity, double *time, double *q, double *qd, double *qdd,
                                     void *hip_stream);

/* Batched TimeOptimalPathProfile::FindMaxSd2Simplex (time_optimal_path_timing.cc:1149-1363)
 * on num_lps independent constraint sets of C rows each ([num_lps][C] arrays);
 * outputs sd2max/sddmax/sd2zero [num_lps]. Host pointers. */
int tpamd_find_max_sd2_host(tpamd_engine *engine, int num_lps, int num_rows,
                            const double *a, const double *b, const double *lower,
                            const double *upper, double *sd2max, double *sddmax,
                            double *sd2zero);

/* ------------------------------------------------------------------------
 * s(t) query: batched TimeOptimalPathProfile::GetPathParameterAndDerivatives
 * (time_optimal_path_timing.cc:1549-1627) on solved profiles. For each path b
 * and query k: t_query[b][k] -> s, sd, sdd, ok [B][K]. time/s/sd/sd2 are the [B][N]
 * outputs of ONE solve (tpamd_path_outputs.time/.s/.sd/.sd2); the per-path ds, s_start and
 * s_end are recovered from the s rows. sd2 may be NULL: the engine then uses the copy of
 * sd2_ it keeps from its LAST solve, and returns TPAMD_E_STALE unless `time` is that solve's
 * output array and the shape matches (a later solve into other buffers invalidates it).
 * Every path has num_samples samples (no ragged batches). status may be NULL. Device pointers.
 * A path whose status is not 0 gets ok = 0 and its out_* entries are not written; ok may be
 * NULL; where ok is 0 on a live path (the reference returns false and leaves its outputs
 * alone) out_s, out_sd, out_sdd are unspecified. Query times that are not finite are outside
 * the bit-for-bit agreement with the reference (its search and this one end in different
 * brackets on a NaN), and so are start_sec values of tpamd_resample_* that are not finite.
 * ------------------------------------------------------------------------ */
int tpamd_query_device(tpamd_engine *engine, int num_paths, int num_samples,
                       int num_queries, const double *time, const double *s,
                       const double *sd, const double *sd2, const int32_t *status,
                       const double *t_query, double *out_s, double *out_sd, double *out_sdd,
                       int32_t *ok, void *hip_stream);

/* ------------------------------------------------------------------------
 * Time samples rebuilt from the velocities of solved paths: time[i] = time[i-1] +
 * 2 ds / (sd[i-1] + sd[i]) (0 across a stationary pair), summed left to right as
 * TimeOptimalPathProfile::OptimizePathParameter does (time_optimal_path_timing.cc:447-455) --
 * bit-identical to the `time` output of the solve that produced sd. For the root of a multi-GPU
 * job: shards send (sd, sdd) and the two scalars (ds, time_start) per path, the root rebuilds
 * time. num_shards blocks of paths_per_shard paths each; block r keeps its arrays at
 * base + r * shard_stride (in doubles): sd [paths_per_shard][num_samples] at sd, ds and
 * time_start [paths_per_shard] at ds / time_start (pointers into shard 0). time_out is
 * [num_shards * paths_per_shard][num_samples], densely packed. num_samples_per_path (per global
 * path index) may be NULL. ds of a path = (s_end - s_start) / (n - 1) with
 * s_end = path_start + delta (n - 1) (path_timing_trajectory.cc:340-341). Device pointers.
 * ------------------------------------------------------------------------ */
int tpamd_rebuild_time_device(tpamd_engine *engine, int num_shards, int paths_per_shard,
                              int num_samples, size_t shard_stride, const double *sd,
                              const double *ds, const double *time_start,
                              const int32_t *num_samples_per_path, double *time_out,
                              void *hip_stream);

/* ------------------------------------------------------------------------
 * Sharding a batch of independent paths over several devices (the arithmetic of
 * sharding.shard_bounds / balanced_bounds, which bench.py uses across processes): contiguous
 * blocks of path indices, block k = [begin[k], begin[k+1]). begin has num_shards + 1 entries.
 * tpamd_shard_bounds: sizes differ by at most one. tpamd_shard_bounds_balanced: blocks of roughly
 * equal total cost for per-path costs (ragged batches: samples x rows^2), every block non-empty
 * while paths last. Host arithmetic only (no device needed).
 * ------------------------------------------------------------------------ */
void tpamd_shard_bounds(int num_paths, int num_shards, int32_t *begin);
void tpamd_shard_bounds_balanced(int num_paths, const double *cost, int num_shards, int32_t *begin);

/* ------------------------------------------------------------------------
 * Uniform-in-time resample: PathTimingTrajectory::ResampleEquidistantlyInTime
 * (path_timing_trajectory.cc:755-783) with InterpolateAtTime (:709-753) for a
 * batch of solved paths. Output row b holds count[b] = ceil((t_end-start)/dt)+1
 * samples, written at [b][0..count) of arrays with stride max_out; if
 * count[b] > max_out only max_out samples are written (count still reports the
 * full number), and the end sample (end position, zero qd and qdd) is special only if
 * it is among them. No slot at or above min(count[b], max_out) is written. For a
 * start_sec more than a time step past the last time stamp count[b] is 0 or negative
 * (the formula above, as the reference evaluates it) and nothing but count[b] is
 * written. A path skipped by status gets count 0. Device pointers.
 * ------------------------------------------------------------------------ */
typedef struct tpamd_resample_args {
  int32_t num_paths, num_samples, num_dofs, max_out;
  const double *time, *s, *sd, *sdd; /* [B][N] */
  const double *q, *qd, *qdd;        /* [B][N][D] */
  const double *max_acceleration;    /* [B][D] */
  const double *start_sec;           /* [B] */
  double time_step;
  const int32_t *status;             /* [B] paths with status != 0 are skipped; may be NULL */
  double *out_time, *out_s, *out_sd, *out_sdd; /* [B][max_out] */
  double *out_q, *out_qd, *out_qdd;            /* [B][max_out][D] */
  int32_t *count;                              /* [B] */
} tpamd_resample_args;

int tpamd_resample_uniform_device(tpamd_engine *engine, const tpamd_resample_args *args,
                                  void *hip_stream);
/* Same with HOST pointers in args (copies in, runs, copies out, synchronises). */
int tpamd_resample_uniform_host(tpamd_engine *engine, const tpamd_resample_args *args);

/* PathTimingTrajectory::ResampleSkippingSamplesCloserThanTimeStep
 * (path_timing_trajectory.cc:785-836; TimeSamplingMethod::kSkipSamplesCloserThanTimeStep):
 * the first output is interpolated at start_sec, then every path sample at least
 * 0.95 * time_step (GetMinTimeDeltaToKeep, :893-900) after the last kept one is taken
 * unchanged; the last output gets the end position and zero derivatives. Same argument
 * struct; count[b] = number of outputs of path b (at most num_samples + 1). There is no
 * limit on num_samples: one wave per path walks the time stamps 64 at a time and keeps no
 * per-sample table (a path's arrays must stay within int indexing, as everywhere). */
int tpamd_resample_skip_device(tpamd_engine *engine, const tpamd_resample_args *args,
                               void *hip_stream);
int tpamd_resample_skip_host(tpamd_engine *engine, const tpamd_resample_args *args);

/* ------------------------------------------------------------------------
 * Fastest stop: PathTimingTrajectory::GetPathStopParameter (path_timing_trajectory.cc:235-287)
 * with ComputeFastestStop (:75-172) on a batch of timed paths. For path b and query_time[b]:
 * the start index is the lower_bound of query_time[b] in time[b][0 .. count[b]); from there the
 * path is time-scaled to rest as fast as max_acceleration[b] allows. Outputs the path parameter
 * s[b][stop_index] of the sample the robot could be at rest at, stop_index (absolute, within
 * the row), the stopping duration and a TPAMD_PLAN_* status: TPAMD_PLAN_INVALID_ARGUMENT if no
 * sample is at or after the query time ("not in timed path range"; stop_parameter 0, stop_index
 * -1). A query on the last sample gives s[b][count-1], duration 0.
 * Rows are the outputs of tpamd_time_joint_paths_* (count = num_samples_per_path) or of
 * tpamd_resample_* (out_*, count) as they are. count [B] may be NULL (every row has `stride`
 * samples); counts are clamped to [0, stride]. profile_time / profile_rate2 / profile_drate2
 * [B][stride] (all three or none) receive ComputeFastestStop's append_time /
 * append_rate_squared / append_diff_rate_squared samples, stop_index - start + 1 per path
 * (nothing for an invalid query); the braking velocities are qd * sqrt(rate2). Results are
 * bit-identical to the scalar restatement in host/fastest_stop.cc. Non-finite inputs are
 * outside the contract. Device pointers.
 * ------------------------------------------------------------------------ */
typedef struct tpamd_fastest_stop_args {
  int32_t num_paths, stride, num_dofs; /* num_dofs 1..16 */
  int32_t reserved;
  const double *time, *s;              /* [B][stride] */
  const double *qd, *qdd;              /* [B][stride][D] */
  const int32_t *count;                /* [B] samples per row; NULL: stride */
  const double *max_acceleration;      /* [B][D] */
  const double *query_time;            /* [B] seconds */
  double *stop_parameter;              /* [B] */
  int32_t *stop_index;                 /* [B] */
  double *duration;                    /* [B] */
  int32_t *status;                     /* [B] TPAMD_PLAN_* */
  double *profile_time, *profile_rate2, *profile_drate2; /* [B][stride], NULL: not written */
} tpamd_fastest_stop_args;

int tpamd_fastest_stop_device(tpamd_engine *engine, const tpamd_fastest_stop_args *args,
                              void *hip_stream);
/* Same with HOST pointers in args (copies in, runs, copies out, synchronises). */
int tpamd_fastest_stop_host(tpamd_engine *engine, const tpamd_fastest_stop_args *args);

/* ------------------------------------------------------------------------
 * Stopping trajectories: TrajectoryBuffer::StopBeforeTime / StopAtIndex (trajectory_buffer.cc:
 * 296-385) with RescaleTrajectoryBackwardToStop (rescale_to_stop.cc) for B sampled trajectories:
 * row b (time [stride], qd / qdd [stride][D], count[b] samples) is cut after sample index and the
 * samples up to it are time-scaled so that the robot comes to rest at q[index] along the same
 * positions within max_acceleration[b]. index = min(lower_bound(stop_time[b]) + 1, count - 1)
 * (StopBeforeTime), or stop_index[b] if stop_index is not NULL (StopAtIndex).
 * Per row: status[b] TPAMD_PLAN_* -- OUT_OF_RANGE (index outside [1, count - 1], a stop time
 * before the first sample), INVALID_ARGUMENT (max_acceleration <= 0, time_step <= 0, times not
 * strictly increasing up to index), NOT_FOUND (the stop needs every sample and still misses the
 * velocity there by more than 1e-2), INTERNAL (sample index < count - 1 already at rest: the
 * reference aborts there; or no admissible deceleration at sample index, every candidate invalid
 * at rate 0: the reference builds a segment with NaN times there), OK; keep[b], the samples of
 * the row kept before the segment; first[b], last[b], the segment's rows within the row.
 * out_time [B][stride] and out_qd / out_qdd
 * [B][stride][D] are written at rows [first, last] only; the segment's positions are the input's
 * q[first .. last], unchanged. The trajectory after the stop is input[0, keep) ++ segment. No
 * samples: OK, keep 0 and an empty segment (first 0, last -1); a failed stop: keep = count and an
 * empty segment (first = count, last = count - 1). On the last sample with |v| < 1e-4 the segment
 * is that sample with zero velocity and acceleration. time_step is checked, not used (as in the
 * reference). count [B] may be NULL (stride samples each); counts are clamped to [0, stride].
 * Bit-identical to the mirror's TrajectoryBuffer (host/trajectory_buffer.cc). Non-finite inputs
 * are outside the contract. Device pointers.
 * ------------------------------------------------------------------------ */
typedef struct tpamd_stop_trajectory_args {
  int32_t num_paths, stride, num_dofs; /* num_dofs 1..16 */
  int32_t reserved;
  const double *time;                  /* [B][stride] */
  const double *qd, *qdd;              /* [B][stride][D] */
  const int32_t *count;                /* [B] samples per row; NULL: stride */
  const double *max_acceleration;      /* [B][D] */
  double time_step;
  const double *stop_time;             /* [B] seconds (StopBeforeTime) */
  const int32_t *stop_index;           /* [B] (StopAtIndex); not NULL: used instead of stop_time */
  int32_t *status, *keep, *first, *last; /* [B] */
  double *out_time;                    /* [B][stride] */
  double *out_qd, *out_qdd;            /* [B][stride][D] */
} tpamd_stop_trajectory_args;

int tpamd_stop_trajectories_device(tpamd_engine *engine, const tpamd_stop_trajectory_args *args,
                                   void *hip_stream);
/* Same with HOST pointers in args (copies in, runs, copies out, synchronises). */
int tpamd_stop_trajectories_host(tpamd_engine *engine, const tpamd_stop_trajectory_args *args);

/* GetPathStopParameter(time) for `count` planners of a set (ids[count], or planners
 * 0..count-1 if ids is NULL) on their resident trajectories after the last Plan: time_ns [count]
 * (TimeToSec: ns / 1e9), stop_parameter, duration (may be NULL), status [count] TPAMD_PLAN_*.
 * A planner without a plan yet gives 0.0 with TPAMD_PLAN_OK (:239-242). Every id is checked
 * before anything runs. One launch; 8 bytes per planner up (12 with ids) and 20 down; no planner
 * state changes. Host pointers; synchronises. */
int tpamd_planner_set_stop_parameters(tpamd_planner_set *set, int count, const int32_t *ids,
                                      const int64_t *time_ns, double *stop_parameter,
                                      double *duration, int32_t *status);

/* ------------------------------------------------------------------------
 * Checking a batch's solutions against its constraint rows:
 * TimeOptimalPathProfile::SolutionSatisfiesConstraints (time_optimal_path_timing.cc:492-518) for
 * every path of a batch. TPAMD_PATH_OK does NOT imply that a path keeps its constraints: on an
 * undersampled path the reference's solver returns OK with violated rows, and so does this engine,
 * bit for bit ("Checking a batch against its constraints").
 *
 * The calls are stateless: the caller passes the batch description it gave the solve and the
 * solution the solve wrote. For path b, samples i < n_b and rows c < C, with sd2 = sol->sd2[b][i] and
 * sdd = sol->sdd[b][i]:
 *   v = a(i,c) * sdd + b(i,c) * sd2           (two products and one sum, not contracted)
 *   row (i,c) is violated  <=>  v + kTiny < lower || v - kTiny > upper, kTiny = 1e5 * DBL_EPSILON
 *                               (time_optimal_path_timing.h:275-279, the reference's test)
 *   excess(i,c) = max(lower - v, v - upper): negative where the row has margin
 * and the rows a, b, lower, upper are exactly those the matching solve forms. Per path:
 *   violations    the number of violated rows; -1: the path is not checked -- sol->status[b] is not
 *                 TPAMD_PATH_OK (the reference's "No valid solution"), or its sample count is one
 *                 for which the solve entry fails the path (outside [2, num_samples]); its
 *                 worst_excess is then NaN and its three indices are -1
 *   worst_excess  the largest excess over the rows whose excess is not NaN; NaN if there is none
 *   worst_sample, worst_row   i and c of that row; among equal values the smallest i * C + c (so no
 *                 order of evaluation can change the answer); -1 if there is none
 *   first_sample  the smallest i with a violated row; -1 if there is none
 * A NaN v violates nothing (both comparisons are false, as in the reference) and has no excess.
 * Without sol->sd2, sd[i] * sd[i] takes its place; the count can then differ from the reference's
 * where a row sits at the kTiny edge, because sqrt followed by the square does not give sd2 back.
 * ------------------------------------------------------------------------ */
typedef struct tpamd_solution {      /* what a solve wrote (tpamd_path_outputs); device pointers for _device */
  const double *sd2;     /* [B][N], or NULL: sd*sd */
  const double *sd;      /* [B][N], read only if sd2 is NULL */
  const double *sdd;     /* [B][N] */
  const int32_t *status; /* [B] TPAMD_PATH_*; NULL: every path is checked */
} tpamd_solution;
typedef struct tpamd_check_outputs {
  int32_t *violations;   /* [B], required */
  double *worst_excess;  /* [B], may be NULL (as the three below) */
  int32_t *worst_sample, *worst_row, *first_sample;
} tpamd_check_outputs;

/* Conventions of the six entries: _device takes device pointers, enqueues one kernel on hip_stream
 * (one workgroup per path) and does not synchronise; _host takes host pointers and synchronises.
 * Neither reads nor disturbs what the engine holds of the last solve (tpamd_query_device still sees
 * it); the check is never pipelined. Call-level errors write nothing and follow the matching solve
 * entry: a NULL engine, struct or required input array, num_paths < 0, a NULL sol, sol->sdd, out or
 * out->violations, or sol->sd2 and sol->sd both NULL (TPAMD_E_INVALID_ARGUMENT); num_dofs outside
 * 1..16, num_rows outside 1..64, num_samples outside 3..8192, more than 65535 paths, or a spline
 * that does not fit the sampling/LP kernel's LDS (TPAMD_E_UNSUPPORTED).
 *
 * Rows form (tpamd_optimize_rows_*, tpamd_optimize_rows_ragged_*): the rows are the caller's arrays.
 * num_samples_per_path [B] as the ragged solve takes it, NULL: every path has num_samples.
 * in->s_start .. in->time_start are not read and may be NULL. */
int tpamd_check_rows_device(tpamd_engine *engine, const tpamd_rows_batch *batch, const tpamd_rows_inputs *in,
                            const int32_t *num_samples_per_path, const tpamd_solution *sol,
                            const tpamd_check_outputs *out, void *hip_stream);
int tpamd_check_rows_host(tpamd_engine *engine, const tpamd_rows_batch *batch, const tpamd_rows_inputs *in,
                          const int32_t *num_samples_per_path, const tpamd_solution *sol,
                          const tpamd_check_outputs *out);
/* Joint form (tpamd_time_joint_paths_*): SamplePath and ConstraintSetup as the sampling/LP kernel
 * does them (the clamp of the parameter to the knots, the end padding with zero derivatives,
 * B = q' * q' for the velocity rows) and the set-up kernel's limits, C = 2D. Ragged through
 * in->num_samples_per_path, as the solve. in->sd_start, sdd_start, time_start and
 * batch->max_solver_loops are not read.
 * num_points_per_path [B] (NULL: every path has batch->num_points control points) checks a waypoint
 * batch (tpamd_time_waypoint_paths_*) from its own fit outputs: knots [B][S + 3] and control_points
 * [B][S][D] then have the slot layout tpamd_waypoint_fit_outputs writes, S = batch->num_points, path
 * k uses the first num_points_per_path[k] entries of its slot, in->delta = delta_used and
 * in->path_start = zeros. A path with fewer than 3 (or more than S) control points is not checked. */
int tpamd_check_joint_paths_device(tpamd_engine *engine, const tpamd_joint_batch *batch,
                                   const tpamd_joint_inputs *in, const int32_t *num_points_per_path,
                                   const tpamd_solution *sol, const tpamd_check_outputs *out, void *hip_stream);
int tpamd_check_joint_paths_host(tpamd_engine *engine, const tpamd_joint_batch *batch,
                                 const tpamd_joint_inputs *in, const int32_t *num_points_per_path,
                                 const tpamd_solution *sol, const tpamd_check_outputs *out);
/* Cartesian form (tpamd_time_cartesian_paths_*, tpamd_time_cartesian_paths_ragged_*):
 * ComputePathDerivatives with the edge rules of the forward differences at n_b - 1 and the
 * C = 2D + 2 rows of ConstraintSetup, J q' summed over the joints in index order.
 * num_samples_per_path and first_row may both be NULL (uniform, strided); otherwise they mean what
 * they mean to the ragged solve, packed row tables included (num_rows: the rows the _host entry
 * stages, read only with first_row). in->sd_start, sdd_start and time_start are not read. */
int tpamd_check_cartesian_paths_device(tpamd_engine *engine, const tpamd_cartesian_batch *batch,
                                       const tpamd_cartesian_inputs *in, const int32_t *num_samples_per_path,
                                       const int32_t *first_row, const tpamd_solution *sol,
                                       const tpamd_check_outputs *out, void *hip_stream);
int tpamd_check_cartesian_paths_host(tpamd_engine *engine, const tpamd_cartesian_batch *batch,
                                     const tpamd_cartesian_inputs *in, const int32_t *num_samples_per_path,
                                     const int32_t *first_row, int64_t num_rows, const tpamd_solution *sol,
                                     const tpamd_check_outputs *out);

/* ------------------------------------------------------------------------
 * Refining violating paths on the device: solve, check, and solve the violators again at doubled
 * sample counts, in one call and without a round trip to the host. Joint batches
 * (tpamd_time_joint_paths_*) and waypoint batches (tpamd_time_waypoint_paths_*); Cartesian batches,
 * explicit rows and planner sets have no refined form (a finer grid needs new rows from the caller).
 *
 * Round 0 is the plain call: `out` receives, bit for bit, what tpamd_time_joint_paths_* /
 * tpamd_time_waypoint_paths_* write for the same arguments, for the paths that are refined too (their
 * coarse solution stays available), and ref->check receives what tpamd_check_joint_paths_* writes
 * for it. The solve is asked for sd2 internally if out->sd2 is NULL.
 *
 * Selection. Path b (n_b samples) needs refinement if violations[b] > 0 and worst_excess[b] >
 * tolerance (tolerance 0 is the reference's criterion: a violated row has a positive excess). Of
 * those, the paths with 2 n_b - 1 <= max_samples take slots 0, 1, .. in ascending path index, up to
 * max_refined slots. The slot numbers come from a prefix count, not from atomics: the slot map is
 * the same in every run. ref->slot[b] is
 *   >= 0   the slot path b is refined in
 *   -1     nothing to refine: the path is clean, within tolerance, or was not checked
 *   -2     the path needs refinement but no slot is left
 *   -3     the path needs refinement but 2 n_b - 1 > max_samples
 *
 * Rounds r = 1 .. max_rounds run on the sub-batch of max_refined slots. A slot's path is solved with
 * n_r = 2 n_{r-1} - 1 samples and delta_r = delta_{r-1} / 2 (exact: the old samples are every second
 * new one) on the same spline, limits, path_start, sd_start, sdd_start and time_start, into
 * ref->refined (arrays of stride max_samples), and checked. The slot goes on to round r + 1 only if
 * that solve still needs refinement by the rule above, r < max_rounds and 2 n_r - 1 <= max_samples;
 * otherwise it is settled and later rounds leave its outputs alone. A finer solve that fails (status
 * not TPAMD_PATH_OK) is not checked and therefore settles: its status is in ref->refined.status and
 * the caller still has the coarse solution in `out`.
 *
 * Per slot k: slot_path[k] (the path, -1 for an unused slot), rounds[k] (solves made), num_samples[k]
 * and delta[k] (of the last solve made; 0 for an unused slot) and refined_check (the record of that
 * last solve; "not checked" for an unused slot). A slot's entries of ref->refined are, bit for bit,
 * what tpamd_time_joint_paths_* writes for that path alone at (num_samples[k], delta[k]); entries
 * behind num_samples[k], and unused slots, are not written.
 *
 * REFINEMENT MAY END WITH VIOLATIONS LEFT. It is a bounded loop whose outcome is reported per path,
 * not a promise: most violators are clean after one doubling, some need two, and a few keep a
 * violated row at every sample count tried ("Refining a batch"). Read refined_check.
 *
 * _device: device pointers (waypoint_offsets stays a host array); enqueues round 0 and max_rounds
 * rounds on hip_stream and does not synchronise except where the plain entry may (workspace or
 * scratch growth); a round with nothing left to do costs its empty launches. _host: host pointers,
 * synchronises, and stops after the round that settles the last slot. Never pipelined. The rounds
 * use a workspace of their own: afterwards tpamd_query_device answers as after the plain call.
 * Call-level errors write nothing and follow the plain entry; in addition a NULL opt or ref or a
 * NULL required array is TPAMD_E_INVALID_ARGUMENT, and options out of range (max_samples below
 * batch->num_samples included) or more than 65535 paths are TPAMD_E_UNSUPPORTED.
 * ------------------------------------------------------------------------ */
typedef struct tpamd_refine_options {
  int32_t max_rounds;   /* 1..8 */
  int32_t max_samples;  /* stride of the refined arrays, 3..8192, >= batch->num_samples */
  int32_t max_refined;  /* M slots, 1..65535 */
  int32_t reserved;
  double tolerance;     /* >= 0 */
} tpamd_refine_options;

typedef struct tpamd_refine_outputs {
  tpamd_check_outputs check;          /* [B] round 0; violations required */
  int32_t *slot;                      /* [B] required */
  int32_t *slot_path;                 /* [M] path of a slot, -1 unused; required */
  int32_t *num_refined;               /* [1] required */
  int32_t *rounds;                    /* [M] solves made in the slot; may be NULL */
  int32_t *num_samples;               /* [M] of the slot's last solve; may be NULL */
  double *delta;                      /* [M] of the slot's last solve; may be NULL */
  tpamd_path_outputs refined;         /* [M][max_samples](..[D]); time, s, sd, sdd, status required */
  tpamd_check_outputs refined_check;  /* [M] record of each slot's final solve; every array may be NULL */
} tpamd_refine_outputs;

int tpamd_time_joint_paths_refined_device(tpamd_engine *engine, const tpamd_joint_batch *batch,
                                          const tpamd_joint_inputs *in, const tpamd_path_outputs *out,
                                          const tpamd_refine_options *opt, const tpamd_refine_outputs *ref,
                                          void *hip_stream);
int tpamd_time_joint_paths_refined_host(tpamd_engine *engine, const tpamd_joint_batch *batch,
                                        const tpamd_joint_inputs *in, const tpamd_path_outputs *out,
                                        const tpamd_refine_options *opt, const tpamd_refine_outputs *ref);
int tpamd_time_waypoint_paths_refined_device(tpamd_engine *engine, const tpamd_waypoint_batch *batch,
                                             const tpamd_waypoint_inputs *in, const tpamd_path_outputs *out,
                                             const tpamd_waypoint_fit_outputs *fit,
                                             const tpamd_refine_options *opt, const tpamd_refine_outputs *ref,
                                             void *hip_stream);
int tpamd_time_waypoint_paths_refined_host(tpamd_engine *engine, const tpamd_waypoint_batch *batch,
                                           const tpamd_waypoint_inputs *in, const tpamd_path_outputs *out,
                                           const tpamd_waypoint_fit_outputs *fit,
                                           const tpamd_refine_options *opt, const tpamd_refine_outputs *ref);

/* ------------------------------------------------------------------------
 * Checking every window a planner set plans: the same question, asked inside
 * tpamd_planner_set_plan / _plan_streaming / _plan_resume / _plan_device, where the windows, their
 * path_start and (Cartesian sets) their table slots exist only until the next window iteration.
 * Off by default; with it off a Plan call enqueues, allocates and writes exactly what it does
 * without this feature. With it on, every window iteration runs one more kernel directly behind the
 * sweep (one workgroup per planner, no atomics, no synchronisation): the rows are those of the
 * window's solve, formed by the same device functions (the joint form above on the planner's
 * resident spline and limits from the window's path_start; the Cartesian form on the window's slots
 * of the resident IK table), and the solution is the solver's sd2 and sdd. The set then owns a
 * [B][N] sd2 buffer and B records (counted in tpamd_planner_set_device_bytes).
 *
 * A planner's window is checked if the planner solved a window in that iteration and the window's
 * status is TPAMD_PATH_OK. A planner that is idle, only erased, waits for IK rows, was stopped by
 * the start-velocity test or by a full history, or whose window failed, is not checked in that
 * iteration and nothing is counted for it.
 *
 * The record covers the windows of the planner's last Plan call, numbered from 0 in solve order (the
 * number of windows the planner had solved in the call before this one). plan, plan_streaming and
 * plan_device start with empty records for every planner; plan_resume continues the records and the
 * numbering of the streaming call it resumes. Across windows the counts add, the larger excess wins
 * and, among equal excesses, the smaller (window, sample, row); the first violated (window, sample)
 * in solve order is kept.
 *
 * `violations` counts whole windows -- what SolutionSatisfiesConstraints answers for each of them. The
 * tail of a window that is not the last, behind the sample where the next window starts, is planned
 * again by that next window, so only the last window is in the history as a whole: hence
 * last_window_violations, and worst_window / worst_sample tell a violation in a replaced tail from
 * one that is executed.
 * ------------------------------------------------------------------------ */
typedef struct tpamd_planner_check {     /* 48 bytes; over the windows the planner's last Plan call solved */
  int32_t windows;                 /* windows checked; 0: none */
  int32_t violations;              /* violated rows summed over them; -1: nothing checked */
  int32_t last_window_violations;  /* of the last checked window alone; -1 */
  int32_t worst_window, worst_sample, worst_row;   /* -1: no row with an excess */
  int32_t first_window, first_sample;              /* -1: no violated row */
  double worst_excess;             /* max(lower - v, v - upper) over all checked rows; NaN: none. Negative: margin */
  double worst_parameter;          /* the window's s at worst_sample; NaN: none */
} tpamd_planner_check;
/* Switches checking on or off. Switching it on allocates the sd2 buffer and the records (kept when
 * it is switched off again) and empties the records; synchronises. */
int tpamd_planner_set_set_checking(tpamd_planner_set *set, int on);
int tpamd_planner_set_checking(const tpamd_planner_set *set);     /* 1 on, 0 off or NULL */
/* out[k] = the record of planner ids[k]; ids NULL: planners 0 .. count-1. With checking off every
 * record is the one of "nothing checked": 0, -1, -1, -1, -1, -1, -1, -1, NaN, NaN. Call-level errors
 * write nothing: a NULL set or out, count < 0 or > B (TPAMD_E_INVALID_ARGUMENT); the host entry also
 * refuses an id outside the set or listed twice. The host entry takes host arrays and synchronises.
 * The _device entry takes device arrays, enqueues one kernel on hip_stream, ordered like the device
 * readouts (behind a tpamd_planner_set_plan_device enqueued before it, on the same or on another
 * stream), and does not synchronise; an id outside the set yields "nothing checked". */
int tpamd_planner_set_check_results(tpamd_planner_set *set, int count, const int32_t *ids,
                                    tpamd_planner_check *out);
int tpamd_planner_set_check_results_device(tpamd_planner_set *set, int count, const int32_t *ids,
                                           tpamd_planner_check *out, void *hip_stream);

/* ------------------------------------------------------------------------
 * Planner state records: a planner of a set as bytes, for another set to take.
 *
 * A record holds everything of one planner that a later call on its set can read: the path
 * (spline or resident IK rows, limits, delta, initial velocity), the window history, the planner
 * scalars, the last window's time profile and the resampled trajectory. It is versioned,
 * position-independent and canonical (csrc/tpamd_state.h states the format): the same planner
 * state always gives the same bytes, all padding is zero, the trajectory is stored from its first
 * live sample (an imported planner's trajectory starts at sample 0), and export(import(r)) == r.
 * Not in a record: per-call scratch, the check record of tpamd_planner_set_set_checking (with
 * checking on, a planner that imports OK reports "nothing checked" until its next Plan) and
 * anything a host mirror knows about where a path came from.
 *
 * A record fits a set of the same kind (joint / Cartesian), num_dofs, num_samples,
 * sampling_method and time_step_ns whose constraint_safety and max_initial_velocity_error have
 * the same bit patterns; num_planners and the capacities may differ.
 *
 * Records are packed into a blob: record k occupies bytes offsets[k] .. offsets[k + 1]); every
 * offset is a multiple of 16 and the blob is 16-byte aligned. Per listed planner a status comes
 * back (TPAMD_PLAN_*): OK; RESOURCE_EXHAUSTED (export: the slot is too small, only the header was
 * written, and not even that below 192 bytes; import_state_device: the record needs more path,
 * history, trajectory or table capacity than the set has reserved, the planner keeps its state);
 * FAILED_PRECONDITION (the planner waits for IK rows in a suspended streaming Plan: it neither
 * exports nor imports); INVALID_ARGUMENT (the _device entries: an id outside the set, an offset
 * that is no multiple of 16, a record that is malformed or of another shape; the planner keeps
 * its state). The host entries check ids (each listed once for an import), offsets and every
 * record before anything changes and return TPAMD_E_INVALID_ARGUMENT for the whole call instead.
 * ids NULL: planners 0 .. count-1. count == 0 returns 0 and touches nothing; count above the
 * set's num_planners is TPAMD_E_INVALID_ARGUMENT in every entry. Bytes of the blob that no record
 * covers (between or behind the records, behind the header of a slot that was too small) keep what
 * they held, in both export entries.
 *
 * The _host entries take host arrays, grow the destination's path, history, trajectory and table
 * capacity as the records need, and synchronise. The _device entries take device arrays (ids
 * included), enqueue two kernels on hip_stream, ordered against the set's other work like the
 * device readouts and tpamd_planner_set_retarget_device, and neither synchronise nor allocate
 * once any state entry has run on the set (the first one allocates 560 bytes of scratch per
 * planner). An import through the _device entry must list every planner once; it leaves the
 * host's copies of the path sizes stale until they are next needed, as a device retarget does:
 * on a Cartesian set the next host entry that reads row counts (tpamd_planner_set_ik_table_info,
 * _append_ik_rows, _discard_ik_rows, the table downloads, a table growth) waits for the import and
 * reads them back once.
 * The summaries an import writes are those of tpamd_planner_set_plan with windows = 0 and the
 * call's per-planner status.
 * ------------------------------------------------------------------------ */
typedef struct tpamd_planner_state_info {   /* 56 bytes */
  int64_t bytes;                /* the planner's record, a multiple of 16 */
  int32_t num_points;           /* control points (joint sets with a path, else 0) */
  int32_t history_count, trajectory_count;
  int32_t table_rows, first_row; /* Cartesian sets: path rows so far, first resident row */
  int32_t has_path, path_state, initial_plan, planned_to_end, target_reached;
  int32_t trajectory_first;     /* samples erased at the front of the trajectory buffer */
  int32_t status;               /* OK, or FAILED_PRECONDITION for a planner that waits for rows */
} tpamd_planner_state_info;
/* The exact record size and the counts of each listed planner; host arrays, one small download,
 * synchronises. */
int tpamd_planner_set_state_info(tpamd_planner_set *set, int count, const int32_t *ids,
                                 tpamd_planner_state_info *info);
/* The largest record the set's current capacities allow. Does not synchronise. */
size_t tpamd_planner_set_state_bytes_bound(const tpamd_planner_set *set);
int tpamd_planner_set_export_state_host(tpamd_planner_set *set, int count, const int32_t *ids, void *blob,
                                        const int64_t *offsets, int32_t *status);
int tpamd_planner_set_export_state_device(tpamd_planner_set *set, int count, const int32_t *ids, void *blob,
                                          const int64_t *offsets, int32_t *status, void *hip_stream);
int tpamd_planner_set_import_state_host(tpamd_planner_set *set, int count, const int32_t *ids, const void *blob,
                                        const int64_t *offsets, tpamd_planner_summary *summary, int32_t *status);
int tpamd_planner_set_import_state_device(tpamd_planner_set *set, int count, const int32_t *ids, const void *blob,
                                          const int64_t *offsets, tpamd_planner_summary *summary, int32_t *status,
                                          void *hip_stream);
/* Planner src_ids[k] of src becomes planner dst_ids[k] of dst (host id arrays, NULL: 0 .. count-1;
 * the destination ids each listed once); synchronises. The sets must have the same shape (else
 * TPAMD_E_INVALID_ARGUMENT) and may be the same set: the records travel through a scratch blob, so
 * any permutation of a set's planners is legal. Sets on different devices go through host memory.
 * If a source planner waits for IK rows nothing is copied and status says which. dst grows as
 * import_state_host grows it. summary (may be NULL) and status are host arrays [count]. */
int tpamd_planner_set_copy_planners(tpamd_planner_set *dst, const int32_t *dst_ids, tpamd_planner_set *src,
                                    const int32_t *src_ids, int count, tpamd_planner_summary *summary,
                                    int32_t *status);

/* ------------------------------------------------------------------------
 * Debug/inspection: copy the boundary curve of the LAST solve to host arrays
 * [B][N] (Boundary::sd2_max, sdd_max_for_sd2_max, sdd_min_for_sd2_max,
 * sd2_max_for_sdd0, type; time_optimal_path_timing.h:225-255) and the squared
 * velocity sd2_. Any pointer may be NULL. Synchronises the device.
 * ------------------------------------------------------------------------ */
int tpamd_debug_copy_boundary(tpamd_engine *engine, int num_paths, int num_samples,
                              double *sd2_max, double *sdd_max, double *sdd_min,
                              double *sd2_zero, uint8_t *type, double *sd2);
/* The specialised joint-space sweep kernels run CalculateBoundary's passes 2-4 themselves and
 * keep sdd_max/sdd_min/type on chip; switch this on BEFORE a solve to have them stored for
 * tpamd_debug_copy_boundary as well (off by default: 17 bytes per sample less HBM traffic). */
void tpamd_debug_keep_boundary(tpamd_engine *engine, int on);

/* Diagnostic builds (-DTPAMD_DIAG) only: per-path counters of the specialised sweep kernel,
 * [B][64] int64: slots 0..31 of the backward wave, 32..63 of the forward wave (meaning of a
 * slot: csrc/tpamd_sweep_joint.h, JointSweep::diag). The product build leaves them zero. */
int tpamd_debug_copy_diag(tpamd_engine *engine, int num_paths, long long *out);
/* The further slots of the same counters, [B][32] int64: 0..15 of the backward wave, 16..31 of
 * the forward wave (JointSweep::diagx: how the wait at a switching-point loop's closing barrier
 * splits up, trips of the qd/qdd emission). */
int tpamd_debug_copy_diag_ext(tpamd_engine *engine, int num_paths, long long *out);
/* Registers per lane of the two hot kernels of the 7-joint path as the loaded code object
 * reports them (hipFuncGetAttributes): which = 0 the sampling/LP kernel, 1 the sweep kernel.
 * The pipelined modes rely on 2 x sweep + 1 x sampling/LP <= 512 (one SIMD's register file);
 * tests/test_gpu_configs.py checks it. Negative: error code. */
int tpamd_debug_kernel_vgprs(tpamd_engine *engine, int which);

/* Per-kernel launch durations for bench.py: HIP events recorded on the launch stream
 * around each kernel (enable = 1) or around the sweep kernel only (enable = 2: two events
 * per solve, so that the measurement barely disturbs the timed region); 0 switches it off.
 * tpamd_profile_mean_ms returns the mean duration in milliseconds over the launches since
 * the last reset (0 if none). */
void tpamd_profile_reset(tpamd_engine *engine);
void tpamd_profile_enable(tpamd_engine *engine, int enable);
double tpamd_profile_mean_ms(tpamd_engine *engine, int kernel_index, int *num_launches);
const char *tpamd_profile_kernel_name(int kernel_index);
int tpamd_profile_num_kernels(void);

#ifdef __cplusplus
}
#endif
#endif /* TPAMD_H_ */
