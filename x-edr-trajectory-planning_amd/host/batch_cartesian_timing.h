// BatchCartesianTiming -- many Cartesian-space paths timed by ONE engine call per group.
//
// A TimeableCartesianSplinePath samples its pose splines, runs the user's path-IK callback
// (timeable_path_cartesian_spline.cc:508-510) and then does arithmetic only:
// ComputePathDerivatives (:39-68), ConstraintSetup (:551-595, which calls the user's
// Jacobian callback per sample, :576), the solver and the planner epilogue. This class
// takes over from the point where the IK solution exists: per path the IK positions
// (path_position_) and the Jacobian callback. The callbacks run on the host, everything
// after them on the GPU (tpamd_time_cartesian_paths_ragged_host: paths of different lengths share
// one call).
#ifndef TPAMD_HOST_BATCH_CARTESIAN_TIMING_H_
#define TPAMD_HOST_BATCH_CARTESIAN_TIMING_H_

#include <functional>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "batch_path_timing.h"

namespace trajectory_planning {

// Stands where the reference has JacobianFunction
// (timeable_path_cartesian_spline.h:39-42, absl::Status(const VectorXd&, Matrix6Xd*)): the
// 6 x D Jacobian is written row-major into `jacobian`.
using CartesianJacobianFunction = std::function<Status(const VectorXd &joints, double *jacobian)>;

struct CartesianPathSamples {
  std::vector<VectorXd> ik_positions;     // N samples of D joints (path_position_)
  CartesianJacobianFunction jacobian;     // jacobian_func_
  VectorXd max_joint_velocity, max_joint_acceleration;   // D each
  double max_translational_velocity = 0.0, max_rotational_velocity = 0.0;
  double delta_parameter = 0.0;           // CartesianPathOptions::delta_parameter
  double constraint_safety = 0.8;         // CartesianPathOptions::constraint_safety
  double path_start = 0.0;                // SamplePath(path_start)
  double start_velocity = 0.0;            // path_start_velocity_ (sd at the first sample)
};

// The engine calls of a block of paths: paths lo .. hi - 1 bucketed by (dofs, constraint safety,
// ceil(samples / 512)), as BatchPathTiming buckets joint paths. Every bucket is one
// ragged engine call whose stride is its largest sample count, so a bucket's stride is less than
// 512 above its shortest path. The buckets come in key order, the paths of a bucket in index order.
// A pure function of the three lists (dofs / samples / safety: one entry per path).
constexpr size_t kCartesianSampleBucket = 512;
inline std::vector<std::vector<size_t>> CartesianTimingBuckets(const std::vector<size_t> &dofs,
                                                               const std::vector<size_t> &samples,
                                                               const std::vector<double> &safety, size_t lo,
                                                               size_t hi) {
  std::map<std::tuple<size_t, double, size_t>, std::vector<size_t>> keyed;
  for (size_t b = lo; b < hi; b++)
    keyed[std::make_tuple(dofs[b], safety[b], (samples[b] + kCartesianSampleBucket - 1) / kCartesianSampleBucket)]
        .push_back(b);
  std::vector<std::vector<size_t>> buckets;
  for (auto &kv : keyed) buckets.push_back(std::move(kv.second));
  return buckets;
}

class BatchCartesianTiming {
 public:
  // Paths may differ in joint count and sample count; they are bucketed by (dofs, constraint safety,
  // ceil(samples / 512)) -- CartesianTimingBuckets -- and every bucket is one ragged engine call
  // (tpamd_time_cartesian_paths_ragged_host) on the packed rows of its paths.
  Status SetPaths(std::vector<CartesianPathSamples> paths);
  // HIP devices that share the batch: contiguous blocks of roughly equal cost (samples x rows^2),
  // one engine from the pool and one host thread per device (the Jacobian callbacks of a block run
  // on its thread: they must be callable concurrently for different paths). Default: the default
  // device alone.
  Status SetDevices(const std::vector<int> &devices);
  // Results in the packed layout of BatchTimingResult; q holds the IK positions.
  Status ComputeTimingProfiles(double time_start_sec, BatchTimingResult *result);
  // Engine calls the last ComputeTimingProfiles made, over all devices: its number of buckets.
  // (the check calls of CheckSolutions are not counted)
  int EngineCallsOfLastCompute() const { return engine_calls_; }
  // On: every bucket's solve is followed by one check of its solutions against the bucket's constraint
  // rows on the device (tpamd_check_cartesian_paths_host, the same packed rows; the solve is asked for
  // sd2), and the result carries violations / worst_sample / worst_row / worst_excess. Off (default):
  // the engine calls and the result are what they are without this option.
  void CheckSolutions(bool on = true) { check_solutions_ = on; }

 private:
  Status ComputeBlock(int device, size_t lo, size_t hi, double time_start_sec, BatchTimingResult *r,
                      int *engine_calls) const;
  std::vector<CartesianPathSamples> paths_;
  std::vector<int> devices_;
  int engine_calls_ = 0;
  bool check_solutions_ = false;
};

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_BATCH_CARTESIAN_TIMING_H_
