// CPU test of the Cartesian waypoint fit (run by tests/test_pose_fit_cpu.py): fit_pose_waypoints of
// csrc/tpamd_pose_fit.h, compiled here for the host, on the case file tests/pose_fit_reference.py
// writes (families of rotations and translations, W = 0..6, D = 1, 6, 7, 16, four rounding pairs).
//
// Default build: every case against the mirror, bit for bit -- the knots of
// TimeableCartesianSplinePath::SetWaypoints (they carry the translation control polygon's length),
// the pose control points of the mirror's PolyLineToBspline3Waypoints and the joint control points of
// TimeableJointSplinePath::PolyLineToControlPoints with the rotation rounding, which are what
// SetWaypoints computes (host/timeable_path_cartesian_spline.cc:175-205). A path without waypoints
// is an error on both sides and writes nothing.
// With -DPOSE_FIT_STANDALONE the mirror is left out: the program needs nothing but the header, so it
// can be built with -fsanitize=address,undefined and run on its own. Output arrays have exactly the
// documented sizes, so that an overrun is a heap-buffer-overflow there.
//
// usage: test_pose_fit CASES [DUMP]; DUMP receives every fit (P, knots, translation, rotation, joint
// control points) for the Python side. Prints one line per family and "ALL OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_pose_fit.h"
#ifndef POSE_FIT_STANDALONE
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_cartesian_spline.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"
using namespace trajectory_planning;
#endif
#include "test_support.h"

static const char *kFamilies[] = {"random", "identical", "tiny", "near_pi", "antipodal", "repeated_translation",
                                  "short", "empty", "golden"};

struct Case {
  int W, D, family;
  double tr, rr;
  std::vector<double> pose, joints;
};

static bool ReadCases(const char *file, std::vector<Case> *cases) {
  FILE *f = std::fopen(file, "rb");
  if (!f) return false;
  int32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1;
  for (int i = 0; ok && i < n; i++) {
    int32_t hdr[4];
    double r[2];
    ok = std::fread(hdr, 4, 4, f) == 4 && std::fread(r, 8, 2, f) == 2 && hdr[0] >= 0 && hdr[0] < 1000 &&
         hdr[1] >= 1 && hdr[1] <= 16 && hdr[2] >= 0 && hdr[2] < 9;
    if (!ok) break;
    Case c;
    c.W = hdr[0]; c.D = hdr[1]; c.family = hdr[2]; c.tr = r[0]; c.rr = r[1];
    c.pose.resize((size_t)c.W * 7);
    c.joints.resize((size_t)c.W * c.D);
    ok = std::fread(c.pose.data(), 8, c.pose.size(), f) == c.pose.size() &&
         std::fread(c.joints.data(), 8, c.joints.size(), f) == c.joints.size();
    cases->push_back(std::move(c));
  }
  std::fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: test_pose_fit CASES [DUMP]\n");
    return 2;
  }
  std::vector<Case> cases;
  if (!ReadCases(argv[1], &cases)) {
    std::printf("cannot read %s\n", argv[1]);
    return 2;
  }
  FILE *dump = argc > 2 ? std::fopen(argv[2], "wb") : nullptr;
  std::map<std::string, int> seen;
  int floor_knots = 0;
  for (const Case &c : cases) {
    const int W = c.W, D = c.D;
    const int P = W < 1 ? 0 : tpamd::fit_points(W);
    std::vector<double> k(P ? P + 3 : 0), t((size_t)3 * P), r((size_t)4 * P), j((size_t)P * D);
    const int got = tpamd::fit_pose_waypoints(c.pose.data(), c.joints.data(), W, D, c.tr, c.rr, k.data(), t.data(),
                                              r.data(), j.data());
    CHECK(got == P);
    if (P && k[P + 2] == 0.1 * 10.0) floor_knots++;
#ifndef POSE_FIT_STANDALONE
    {
      using tpamd::compat::OkStatus;
      CartesianPathOptions opt;
      opt.set_num_dofs(D).set_num_path_samples(3).set_rounding(c.rr);
      opt.set_translation_rounding(c.tr);
      opt.set_path_ik_func([](const VectorXd &, const std::vector<Pose3d> &, const std::vector<VectorXd> &,
                              std::vector<VectorXd> *) { return OkStatus(); });
      opt.set_jacobian_func([](const VectorXd &, Matrix6Xd *) { return OkStatus(); });
      TimeableCartesianSplinePath path(opt);
      std::vector<Pose3d> poses;
      std::vector<VectorXd> joints;
      for (int i = 0; i < W; i++) {
        const double *p = &c.pose[(size_t)7 * i];
        poses.push_back(Pose3d(Quaterniond(p[3], p[4], p[5], p[6]), Vector3d(p[0], p[1], p[2])));
        joints.push_back(VectorXd(&c.joints[(size_t)i * D], (size_t)D));
      }
      const Status st = path.SetWaypoints({poses.data(), poses.size()}, {joints.data(), joints.size()});
      if (W < 1) {
        CHECK(st.code() == tpamd::compat::StatusCode::kInvalidArgument);
      } else {
        CHECK(st.ok());
        bool same = path.knots().size() == (size_t)P + 3 && SameBits(path.knots().data(), k.data(), (size_t)P + 3);
        std::vector<Pose3d> mp;
        PolyLineToBspline3Waypoints(poses, c.tr, c.rr, &mp);
        same = same && (int)mp.size() == P;
        for (int i = 0; same && i < P; i++) {
          const Quaterniond &q = mp[i].quaternion();
          const double mq[4] = {q.w, q.x, q.y, q.z};
          same = SameBits(mp[i].translation().v, &t[(size_t)3 * i], 3) && SameBits(mq, &r[(size_t)4 * i], 4);
        }
        std::vector<VectorXd> mj;
        TimeableJointSplinePath::PolyLineToControlPoints(joints, c.rr, &mj);
        same = same && (int)mj.size() == P;
        for (int i = 0; same && i < P; i++) same = SameBits(mj[i].data(), &j[(size_t)i * D], (size_t)D);
        CHECK(same);
        if (!same)
          std::printf("  %s: differs from the mirror (W %d D %d roundings %.17g %.17g)\n", kFamilies[c.family], W, D,
                      c.tr, c.rr);
      }
    }
#endif
    seen[kFamilies[c.family]]++;
    if (dump) {
      const int32_t p32 = P;
      std::fwrite(&p32, 4, 1, dump);
      std::fwrite(k.data(), 8, k.size(), dump);
      std::fwrite(t.data(), 8, t.size(), dump);
      std::fwrite(r.data(), 8, r.size(), dump);
      std::fwrite(j.data(), 8, j.size(), dump);
    }
  }
  if (dump) std::fclose(dump);
  for (const auto &kv : seen) std::printf("category %s: %d\n", kv.first.c_str(), kv.second);
  std::printf("pose fit cases: %d\n", (int)cases.size());
  std::printf("final knot at the floor: %d\n", floor_knots);
#ifdef POSE_FIT_STANDALONE
  std::printf("standalone: mirror not linked\n");
#endif
  if (g_fail) {
    std::printf("%d FAILURES\n", g_fail);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}
