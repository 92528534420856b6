// The per-path host loop a Cartesian goal went through before the device fit and the device target
// sampler existed (tools/gpu_ik_targets_bench.py builds and runs this): for every path,
// TimeableCartesianSplinePath::SetWaypoints (the fit on the host) and then the target part of
// ExtendIkSolution for the whole IK table -- the pose sampler with num_paths = 1 (one upload, one
// launch, one download) plus the host EvalCurve loop. ExtendIkSolution is reached through
// SamplePath(knots.back() + delta), whose horizon is the table's last row; the IK callback only copies
// the joint targets (the IK itself is not part of either side), the Jacobian callback is never called.
//
// usage: ik_targets_host_loop INPUT REPEATS
// INPUT: int32 paths, dofs, samples, waypoints per path; then per path double delta, pose waypoints
// [W][7] (translation, quaternion w x y z), joint waypoints [W][D]. Prints one JSON line.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../x-edr-trajectory-planning_amd/host/timeable_path_cartesian_spline.h"

using namespace trajectory_planning;
using tpamd::compat::OkStatus;

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  if (std::fread(hdr, 4, 4, f) != 4) return 2;
  const int B = hdr[0], D = hdr[1], N = hdr[2], W = hdr[3], repeats = std::atoi(argv[2]);
  std::vector<double> delta(B);
  std::vector<std::vector<Pose3d>> poses(B);
  std::vector<std::vector<VectorXd>> joints(B);
  for (int b = 0; b < B; b++) {
    std::vector<double> p((size_t)W * 7), j((size_t)W * D);
    if (std::fread(&delta[b], 8, 1, f) != 1 || std::fread(p.data(), 8, p.size(), f) != p.size() ||
        std::fread(j.data(), 8, j.size(), f) != j.size())
      return 2;
    for (int i = 0; i < W; i++) {
      const double *r = &p[(size_t)7 * i];
      poses[b].push_back(Pose3d(Quaterniond(r[3], r[4], r[5], r[6]), Vector3d(r[0], r[1], r[2])));
      joints[b].push_back(VectorXd(&j[(size_t)i * D], (size_t)D));
    }
  }
  std::fclose(f);
  long rows = 0;
  const auto ik = [&rows](const VectorXd &, const std::vector<Pose3d> &, const std::vector<VectorXd> &joint_targets,
                          std::vector<VectorXd> *result) {
    *result = joint_targets;
    rows += (long)joint_targets.size() - 1;      // the first target repeats the initial condition
    return OkStatus();
  };
  const auto jac = [](const VectorXd &, Matrix6Xd *) { return OkStatus(); };
  // the path objects are the caller's and outlive a goal: built once, outside the timed loop
  std::vector<std::unique_ptr<TimeableCartesianSplinePath>> paths;
  for (int b = 0; b < B; b++) {
    CartesianPathOptions opt;
    opt.set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta[b]);
    opt.set_path_ik_func(ik).set_jacobian_func(jac);
    paths.emplace_back(new TimeableCartesianSplinePath(opt));
  }
  std::vector<double> seconds;
  for (int rep = 0; rep < repeats + 1; rep++) {          // the first pass warms the engine up
    rows = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int b = 0; b < B; b++) {
      TimeableCartesianSplinePath &path = *paths[b];
      if (!path.SetWaypoints({poses[b].data(), poses[b].size()}, {joints[b].data(), joints[b].size()}).ok()) return 1;
      if (!path.SamplePath(path.knots().back() + delta[b]).ok()) return 1;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rep > 0) seconds.push_back(s);
  }
  std::sort(seconds.begin(), seconds.end());
  std::printf("{\"paths\": %d, \"rows\": %ld, \"repeats\": %d, \"loop_ms_median\": %.3f, \"loop_ms_min\": %.3f, "
              "\"loop_ms_max\": %.3f}\n",
              B, rows, repeats, 1e3 * seconds[seconds.size() / 2], 1e3 * seconds.front(), 1e3 * seconds.back());
  return 0;
}
