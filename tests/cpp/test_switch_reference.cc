// Driver for tests/test_switch_reference_cpu.py: runs the spline edits two ways on the cases of an
// input file and writes every result in binary, so that the Python restatement
// (tests/switch_reference.py) can compare bit for bit:
//   R  the host-compilable routines of the kernels: sw_switch_to_waypoint_path and
//      sw_velocity_at_time (csrc/tpamd_switch.h), fit_waypoints (csrc/tpamd_fit.h);
//   M  the mirror: TimeableJointSplinePath::SetWaypoints / SwitchToWaypointPath
//      (host/timeable_path_joint_spline.cc, host/spline_edit.cc) and
//      TrajectoryBuffer::GetVelocityAtTime (host/trajectory_buffer.cc).
//
// Input (whitespace separated, doubles as C99 hex floats): num_records, then per record
//   S id D first raw P W keep  knots[P + 3] points[P * D] waypoints[W * D]  [first: W0 waypoints0[W0 * D]]
//       one switch of planner `id`. The mirror object of `id` is made by SetWaypoints(waypoints0)
//       at the planner's first record and keeps its state from record to record. raw = 1: the
//       spline was not made by a fit (a non-zero first knot); the mirror is not run (count -1).
//   F D W rounding  waypoints[W * D]
//   V D n query  time[n] velocity[n * D]
// Output, per record and for R then M: int32 status, int32 count, double[count].
//   S: count = K + P' * D doubles, the new knots then the new points (0 unless the status is OK)
//   F: the same layout for the fitted spline; V: the D velocities (0 unless the status is OK)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_fit.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"
#include "../../x-edr-trajectory-planning_amd/host/trajectory_buffer.h"

using namespace trajectory_planning;
using tpamd::compat::StatusCode;

static FILE *g_in, *g_out;

static double ReadDouble() {
  double v = 0.0;
  if (std::fscanf(g_in, "%la", &v) != 1) { std::fprintf(stderr, "bad input\n"); std::exit(2); }
  return v;
}

static int ReadInt() {
  int v = 0;
  if (std::fscanf(g_in, "%d", &v) != 1) { std::fprintf(stderr, "bad input\n"); std::exit(2); }
  return v;
}

static std::vector<double> ReadDoubles(size_t n) {
  std::vector<double> v(n);
  for (double &x : v) x = ReadDouble();
  return v;
}

static std::vector<VectorXd> Rows(const std::vector<double> &flat, int rows, int D) {
  std::vector<VectorXd> out;
  for (int i = 0; i < rows; i++) out.push_back(VectorXd(flat.data() + (size_t)i * D, D));
  return out;
}

static int Code(const Status &s) {
  switch (s.code()) {
    case StatusCode::kOk: return tpamd::kSwOk;
    case StatusCode::kFailedPrecondition: return tpamd::kSwFailedPrecondition;
    case StatusCode::kOutOfRange: return tpamd::kSwOutOfRange;
    case StatusCode::kInvalidArgument: return tpamd::kSwInvalidArgument;
    default: return tpamd::kSwInternal;
  }
}

static void Write(int status, int count, const double *a, size_t na, const double *b, size_t nb) {
  const int32_t head[2] = {status, count};
  std::fwrite(head, sizeof(int32_t), 2, g_out);
  if (count > 0) {
    std::fwrite(a, sizeof(double), na, g_out);
    if (nb) std::fwrite(b, sizeof(double), nb, g_out);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  g_in = std::fopen(argv[1], "r");
  g_out = std::fopen(argv[2], "wb");
  if (!g_in || !g_out) return 2;
  std::map<int, std::shared_ptr<TimeableJointSplinePath>> mirrors;
  const int records = ReadInt();
  for (int r = 0; r < records; r++) {
    char kind = 0;
    if (std::fscanf(g_in, " %c", &kind) != 1) return 2;
    if (kind == 'S') {
      const int id = ReadInt(), D = ReadInt(), first = ReadInt(), raw = ReadInt(), P = ReadInt(), W = ReadInt();
      const double keep = ReadDouble();
      const std::vector<double> knots = ReadDoubles(P + 3), points = ReadDoubles((size_t)P * D);
      const std::vector<double> wps = ReadDoubles((size_t)W * D);
      if (first) {
        const int W0 = ReadInt();
        const std::vector<double> wps0 = ReadDoubles((size_t)W0 * D);
        auto path = std::make_shared<TimeableJointSplinePath>(JointPathOptions().set_num_dofs(D).set_num_path_samples(8));
        const std::vector<VectorXd> rows = Rows(wps0, W0, D);
        if (!path->SetWaypoints({rows.data(), rows.size()}).ok()) return 3;
        mirrors[id] = path;
      }
      {   // R: the arrays have their documented sizes and a guard row behind each
        const int bound = tpamd::sw_points_bound(P, W);
        const size_t nk_doc = bound + 3, np_doc = (size_t)bound * D, nw_doc = (size_t)(W + 2) * D, guard = D;
        std::vector<double> k(nk_doc + guard, -7.0), p(np_doc + guard, -7.0), work(nw_doc + guard, -7.0);
        std::copy(knots.begin(), knots.end(), k.begin());
        std::copy(points.begin(), points.end(), p.begin());
        int nk = 0, np = 0;
        const int st = tpamd::sw_switch_to_waypoint_path(k.data(), p.data(), P + 3, P, D, keep, wps.data(), W,
                                                         tpamd::kSwitchRounding, work.data(), &nk, &np);
        if (st == tpamd::kSwOk && (np > bound || nk != np + 3)) return 4;
        for (size_t i = 0; i < guard; i++)
          if (k[nk_doc + i] != -7.0 || p[np_doc + i] != -7.0 || work[nw_doc + i] != -7.0) {
            std::fprintf(stderr, "record %d: the edit wrote behind its documented area\n", r);
            return 5;
          }
        if (st == tpamd::kSwOk) Write(st, nk + np * D, k.data(), nk, p.data(), (size_t)np * D);
        else Write(st, 0, nullptr, 0, nullptr, 0);
      }
      if (raw) {
        Write(0, -1, nullptr, 0, nullptr, 0);
      } else {   // M
        TimeableJointSplinePath &path = *mirrors.at(id);
        const std::vector<VectorXd> rows = Rows(wps, W, D);
        const Status st = path.SwitchToWaypointPath(keep, {rows.data(), rows.size()});
        const int nk = (int)path.knots().size(), np = path.num_control_points();
        // a failed switch leaves the mirror's spline as it was: written out so that Python sees it
        Write(Code(st), nk + np * D, path.knots().data(), nk, path.packed_control_points().data(), (size_t)np * D);
      }
    } else if (kind == 'F') {
      const int D = ReadInt(), W = ReadInt();
      const double rounding = ReadDouble();
      const std::vector<double> wps = ReadDoubles((size_t)W * D);
      {   // R
        const int cap = W < 1 ? 1 : tpamd::fit_points(W);
        std::vector<double> k(cap + 3 + 1, -7.0), p((size_t)cap * D + D, -7.0);
        const int P = tpamd::fit_waypoints(wps.data(), W, D, rounding, k.data(), p.data());
        if (k[cap + 3] != -7.0 || p[(size_t)cap * D] != -7.0) return 5;        // behind fit_points(W) points
        if (P > 0) Write(tpamd::kSwOk, P + 3 + P * D, k.data(), P + 3, p.data(), (size_t)P * D);
        else Write(tpamd::kSwInvalidArgument, 0, nullptr, 0, nullptr, 0);
      }
      {   // M
        TimeableJointSplinePath path(JointPathOptions().set_num_dofs(D).set_num_path_samples(8).set_rounding(rounding));
        const std::vector<VectorXd> rows = Rows(wps, W, D);
        const Status st = path.SetWaypoints({rows.data(), rows.size()});
        const int nk = (int)path.knots().size(), np = path.num_control_points();
        if (st.ok()) Write(0, nk + np * D, path.knots().data(), nk, path.packed_control_points().data(), (size_t)np * D);
        else Write(Code(st), 0, nullptr, 0, nullptr, 0);
      }
    } else if (kind == 'V') {
      const int D = ReadInt(), n = ReadInt();
      const double query = ReadDouble();
      const std::vector<double> t = ReadDoubles(n), v = ReadDoubles((size_t)n * D);
      {   // R
        std::vector<double> out(D, -7.0);
        const int st = tpamd::sw_velocity_at_time(t.data(), v.data(), n, D, query, out.data());
        Write(st, st == tpamd::kSwOk ? D : 0, out.data(), D, nullptr, 0);
      }
      {   // M
        const std::vector<VectorXd> V = Rows(v, n, D);
        auto buf = *TrajectoryBuffer::Create();
        if (n > 0) {
          buf->InsertSegment(Span<const double>(t.data(), n), Span<const VectorXd>(V.data(), n),
                             Span<const VectorXd>(V.data(), n), Span<const VectorXd>(V.data(), n));
        }
        const auto got = buf->GetVelocityAtTime(query);
        if (got.ok()) Write(0, D, (*got).data(), D, nullptr, 0);
        else Write(Code(got.status()), 0, nullptr, 0, nullptr, 0);
      }
    } else {
      return 2;
    }
  }
  std::fclose(g_in);
  std::fclose(g_out);
  return 0;
}
