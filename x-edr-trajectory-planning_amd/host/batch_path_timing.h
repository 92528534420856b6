// BatchPathTiming -- the addition to the reference API: many independent
// TimeableJointSplinePath objects timed by ONE engine call (B >> 1). Each path gets the
// result PathTimingTrajectory::ComputeTimingProfile would have produced for it
// (path_timing_trajectory.cc:307-475, new-path case: s from 0, zero start velocity
// unless the path carries an initial velocity).
#ifndef TPAMD_HOST_BATCH_PATH_TIMING_H_
#define TPAMD_HOST_BATCH_PATH_TIMING_H_

#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "timeable_path_joint_spline.h"

namespace trajectory_planning {

// Results are packed path after path without padding: path b owns
// time/s/sd/sdd[sample_offset[b] .. sample_offset[b+1]) and
// q/qd/qdd[joint_offset[b] .. joint_offset[b+1]) (row-major [n_b][D_b]). For a uniform
// batch that is the dense [B][N] / [B][N][D] layout.
struct BatchTimingResult {
  int num_samples = 0, num_dofs = 0;         // maxima over the batch (= the common values if uniform)
  std::vector<int32_t> status;               // [B] TPAMD_PATH_* (0 = solved)
  std::vector<int32_t> last_extremal_index;  // [B]
  std::vector<int32_t> samples_per_path, dofs_per_path;  // [B]
  std::vector<size_t> sample_offset, joint_offset;        // [B+1]
  std::vector<double> time, s, sd, sdd;
  std::vector<double> q, qd, qdd;
  // CheckSolutions(true) only (empty otherwise): per path what tpamd_check_*_host reports --
  // TimeOptimalPathProfile::SolutionSatisfiesConstraints (time_optimal_path_timing.cc:492-518) as a count of
  // violated rows (-1: not checked, the path has no solution), the row with the largest excess over its
  // bound and that excess. status == 0 does NOT imply violations == 0.
  std::vector<int32_t> violations, worst_sample, worst_row;  // [B]
  std::vector<double> worst_excess;                          // [B]
  // RefineSolutions only (empty otherwise): the solves made in the path's slot (0: the path was not refined)
  // and its slot code -- the slot (>= 0), -1 nothing to refine, -2 no slot left, -3 too long
  // (include/tpamd.h tpamd_refine_outputs). With the option on the check vectors above are always filled
  // and describe the solution the result carries.
  std::vector<int32_t> refine_rounds, refine_slot_code;      // [B]
};

// RefineSolutions of BatchPathTiming and BatchWaypointTiming (include/tpamd.h, "Refining violating paths"):
// every group goes through the refined _host entry, one group at a time. A path whose slot ended with
// status TPAMD_PATH_OK and fewer violated rows than its coarse solve carries the refined arrays (2 n - 1,
// 4 n - 3, .. samples: samples_per_path and the offsets follow); every other path carries its coarse
// arrays. Refinement may end with violations left: read `violations`.
struct RefineOptions {
  bool enabled = true;
  int max_rounds = 2;     // 1..8
  int max_samples = 0;    // stride of the refined arrays; 0: what max_rounds doublings of the group's largest
                          // sample count need, at most 8192
  int max_refined = 0;    // slots per group; 0: one per path of the group
  double tolerance = 0.0; // a path is refined if it has violated rows and its worst excess lies above this
};

// (shared by the three batch classes) the check result of a batch, sized or emptied; the records of one
// group's check call and their way into the packed result
void PrepareCheckResult(bool on, size_t num_paths, BatchTimingResult *result);
struct CheckRecords {
  explicit CheckRecords(size_t n) : violations(n, -1), worst_sample(n, -1), worst_row(n, -1), worst_excess(n, 0.0) {}
  tpamd_check_outputs outputs();
  void scatter(const std::vector<size_t> &ids, BatchTimingResult *result) const;
  std::vector<int32_t> violations, worst_sample, worst_row;
  std::vector<double> worst_excess;
};

// (shared by BatchPathTiming and BatchWaypointTiming) One group's arrays of a refined _host call, and what
// each of its paths contributes to the result. The result is packed after all solves (PackRefinedResult),
// because the sample counts are only known then.
struct PathSolution {
  int32_t status = -1, last_extremal_index = 0, samples = 0, dofs = 0;
  std::vector<double> time, s, sd, sdd, q, qd, qdd;          // [samples](..[dofs]); zeros without a solution
  int32_t violations = -1, worst_sample = -1, worst_row = -1, rounds = 0, slot_code = -1;
  double worst_excess = 0.0;
};
struct RefinedGroup {
  // B paths timed at stride N (the group's largest count), D joints
  RefinedGroup(size_t B, size_t N, size_t D, const RefineOptions &options);
  tpamd_refine_options options() const;
  tpamd_refine_outputs outputs();
  // Path i of the group, with `samples` samples in the coarse arrays (stride N, as the plain entry
  // fills them): the refined solution of its slot if that is OK and has fewer violated rows, else the
  // coarse one. keep_last_extremal_index false: a path without waypoints, whose index is not written.
  PathSolution Solution(size_t i, size_t samples, const tpamd_path_outputs &coarse, bool keep_last_extremal_index = true) const;
  size_t B, N, D, M, NS;
  RefineOptions opt;
  CheckRecords check, refined_check;
  std::vector<int32_t> slot, slot_path, num_refined, rounds, num_samples, status, lei;
  std::vector<double> delta, time, s, sd, sdd, q, qd, qdd;
};
void PackRefinedResult(const std::vector<PathSolution> &paths, BatchTimingResult *result);

class BatchPathTiming {
 public:
  // Off by default; with it off the engine calls and the result are what they are without this option.
  void RefineSolutions(const RefineOptions &options) { refine_ = options; }
  // Paths may differ in num_dofs, num_path_samples and waypoint count (BASELINE.json configs[4]):
  // they are grouped by (dofs, control points, constraint safety[, ceil(samples / bucket)]) with
  // per-path sample counts, and ALL groups of a device are solved by one engine call, side by side
  // (tpamd_time_joint_groups_host; within a group the sweep takes the paths longest first).
  Status SetPaths(const std::vector<std::shared_ptr<TimeableJointSplinePath>> &paths);
  // HIP devices that share the batch: the paths are cut into contiguous blocks of
  // roughly equal cost (samples x rows^2, tpamd_shard_bounds_balanced), one block, one engine from
  // the pool and one host thread per device; results go straight into the caller's result, nothing
  // travels between devices. Default: the default device (TPAMD_DEVICE, else 0) alone.
  Status SetDevices(const std::vector<int> &devices);
  // Sample-count bucket of ragged batches: 0 (default) = one group per (dofs, control points,
  // safety), its stride the largest sample count; w > 0 = also by ceil(samples / w), as
  // SURVEY.md 8d sketches with w = 512. Measured on MI355X (DESIGN.md, configs[4]): the coarser
  // the faster -- every group costs four launches and the runtime has four hardware queues.
  void SetSampleBucket(int samples) { sample_bucket_ = samples > 0 ? samples : 0; }
  // Times every path starting at path parameter 0 and time `time_start_sec`.
  Status ComputeTimingProfiles(double time_start_sec, BatchTimingResult *result);
  // On: every engine solve of a group is followed by one check of its solutions against the group's
  // constraint rows on the device (tpamd_check_joint_paths_host; the solve is asked for sd2), and the
  // result carries violations / worst_sample / worst_row / worst_excess. Off (default): the engine calls
  // and the result are what they are without this option.
  void CheckSolutions(bool on = true) { check_solutions_ = on; }

 private:
  // refined: null, or one entry per path of the batch that the block fills in place of the result's arrays
  Status ComputeBlock(int device, size_t lo, size_t hi, double time_start_sec, BatchTimingResult *r,
                      std::vector<PathSolution> *refined) const;
  RefineOptions refine_{/*enabled=*/false};
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths_;
  std::vector<int> devices_;
  int sample_bucket_ = 0;
  bool check_solutions_ = false;
};

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_BATCH_PATH_TIMING_H_
