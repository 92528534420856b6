// GPU test of BatchCartesianTiming on paths of different lengths (run by
// tests/test_gpu_cartesian_ragged_mirror.py): 40 paths of 40 distinct lengths (500, 510, .. 890
// samples), 6 and 7 joints alternating. Every path's result is bit-equal to timing that path alone
// through the uniform entry (tpamd_time_cartesian_paths_host, B = 1, N = its length) and to the
// oracle, and the batch takes one engine call per (dofs, safety, ceil(samples / 512)) bucket: 4,
// where one call per exact sample count would be 40.
// --cpu-check: the oracle alone (no GPU call): every path must solve.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/tpamd.h"
#include "../../oracle/tp_oracle.h"
#include "../../x-edr-trajectory-planning_amd/host/batch_cartesian_timing.h"
#include "../../x-edr-trajectory-planning_amd/host/engine_handle.h"
#include "test_support.h"

using namespace trajectory_planning;

static bool Same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * 8) == 0; }

static const int kPaths = 40;
static const double kTimeStart = 2.0;

static std::vector<CartesianPathSamples> MakePaths() {
  unsigned long long seed = 4711;
  auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
  std::vector<CartesianPathSamples> paths(kPaths);
  for (int b = 0; b < kPaths; b++) {
    const int D = (b % 2) ? 7 : 6, N = 500 + 10 * b;
    CartesianPathSamples &p = paths[b];
    p.delta_parameter = 0.004 + 0.002 * rnd();
    std::vector<double> amp(D), freq(D), phase(D), slope(D);
    for (int d = 0; d < D; d++) {
      amp[d] = 0.2 + 0.5 * rnd(); freq[d] = 0.5 + 1.5 * rnd(); phase[d] = 6.28 * rnd(); slope[d] = 0.6 * rnd() - 0.3;
    }
    for (int i = 0; i < N; i++) {
      const double s = i * p.delta_parameter;
      VectorXd q(D);
      for (int d = 0; d < D; d++) q[d] = amp[d] * std::sin(freq[d] * s + phase[d]) + slope[d] * s;
      p.ik_positions.push_back(q);
    }
    p.jacobian = [D](const VectorXd &q, double *J) {
      for (int r = 0; r < 6; r++)
        for (int d = 0; d < D; d++)
          J[r * D + d] = 0.25 * std::sin(q[d] * (r + 1.0) + 0.37 * d) + ((r == d % 6) ? 1.0 : 0.0);
      return ::tpamd::compat::OkStatus();
    };
    p.max_joint_velocity = VectorXd(D, 1.0 + rnd());
    p.max_joint_acceleration = VectorXd(D, 2.0 + 2.0 * rnd());
    p.max_translational_velocity = 0.6 + 0.9 * rnd();
    p.max_rotational_velocity = 0.8 + 1.2 * rnd();
    if (b % 5 == 3) p.start_velocity = 0.02;
  }
  return paths;
}

struct Alone {
  std::vector<double> q, J, t, s, sd, sdd, qd, qdd;
  int32_t status = -1, lei = 0;
};

static void Flatten(const CartesianPathSamples &p, Alone *a) {
  const size_t N = p.ik_positions.size(), D = p.ik_positions[0].size();
  a->q.resize(N * D); a->J.resize(N * 6 * D);
  a->t.assign(N, 0); a->s.assign(N, 0); a->sd.assign(N, 0); a->sdd.assign(N, 0);
  a->qd.assign(N * D, 0); a->qdd.assign(N * D, 0);
  for (size_t i = 0; i < N; i++) {
    for (size_t d = 0; d < D; d++) a->q[i * D + d] = p.ik_positions[i][d];
    CHECK(p.jacobian(p.ik_positions[i], &a->J[i * 6 * D]).ok());
  }
}

static int OracleAlone(const CartesianPathSamples &p, Alone *a) {
  const int N = (int)p.ik_positions.size(), D = (int)p.ik_positions[0].size();
  Flatten(p, a);
  int lei = 0;
  a->status = tpo_time_cartesian_path(a->q.data(), a->J.data(), N, D, p.max_joint_velocity.data(),
                                      p.max_joint_acceleration.data(), p.max_translational_velocity,
                                      p.max_rotational_velocity, p.constraint_safety, p.path_start, p.delta_parameter,
                                      p.start_velocity, 0.0, kTimeStart, a->t.data(), a->s.data(), a->sd.data(),
                                      a->sdd.data(), a->qd.data(), a->qdd.data(), &lei);
  a->lei = lei;
  return a->status;
}

// the uniform entry on the path alone
static int EngineAlone(tpamd_engine *engine, const CartesianPathSamples &p, Alone *a) {
  const int N = (int)p.ik_positions.size(), D = (int)p.ik_positions[0].size();
  Flatten(p, a);
  const double vt = p.max_translational_velocity, vr = p.max_rotational_velocity, ps = p.path_start,
               dl = p.delta_parameter, sd0 = p.start_velocity, sdd0 = 0.0, t0 = kTimeStart;
  tpamd_cartesian_batch batch{1, D, N, 0, p.constraint_safety};
  tpamd_cartesian_inputs in{a->q.data(), a->J.data(), p.max_joint_velocity.data(), p.max_joint_acceleration.data(),
                            &vt, &vr, &ps, &dl, &sd0, &sdd0, &t0};
  tpamd_path_outputs out{a->t.data(), a->s.data(), a->sd.data(), a->sdd.data(), nullptr, a->qd.data(), a->qdd.data(),
                         &a->lei, nullptr, &a->status, nullptr};
  return tpamd_time_cartesian_paths_host(engine, &batch, &in, &out);
}

static void Compare(const BatchTimingResult &r, int b, const Alone &a, int *equal) {
  const size_t N = a.t.size(), so = r.sample_offset[b], jo = r.joint_offset[b];
  const bool same = r.status[b] == a.status && r.last_extremal_index[b] == a.lei && Same(&r.time[so], a.t.data(), N) &&
                    Same(&r.s[so], a.s.data(), N) && Same(&r.sd[so], a.sd.data(), N) &&
                    Same(&r.sdd[so], a.sdd.data(), N) && Same(&r.q[jo], a.q.data(), a.q.size()) &&
                    Same(&r.qd[jo], a.qd.data(), a.qd.size()) && Same(&r.qdd[jo], a.qdd.data(), a.qdd.size());
  CHECK(same);
  *equal += same;
}

int main(int argc, char **argv) {
  const std::vector<CartesianPathSamples> paths = MakePaths();
  std::vector<Alone> oracle(kPaths);
  int solved = 0;
  for (int b = 0; b < kPaths; b++) solved += OracleAlone(paths[b], &oracle[b]) == 0;
  std::printf("oracle: %d of %d paths solved\n", solved, kPaths);
  CHECK(solved == kPaths);
  if (argc > 1 && std::strcmp(argv[1], "--cpu-check") == 0) {
    if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
  }
  BatchCartesianTiming batch;
  CHECK(batch.SetPaths(paths).ok());
  CHECK(batch.EngineCallsOfLastCompute() == 0);
  BatchTimingResult r;
  CHECK(batch.ComputeTimingProfiles(kTimeStart, &r).ok());
  // the buckets, from the pure function the mirror uses
  std::vector<size_t> dofs, samples;
  std::vector<double> safety;
  for (const auto &p : paths) {
    dofs.push_back(p.ik_positions[0].size()); samples.push_back(p.ik_positions.size()); safety.push_back(p.constraint_safety);
  }
  const size_t buckets = CartesianTimingBuckets(dofs, samples, safety, 0, paths.size()).size();
  std::printf("engine calls: %d, buckets: %d, distinct sample counts: %d\n", batch.EngineCallsOfLastCompute(),
              (int)buckets, kPaths);
  CHECK(buckets == 4 && batch.EngineCallsOfLastCompute() == (int)buckets);
  ::tpamd::EngineLease lease = ::tpamd::acquire_engine(::tpamd::default_device());
  CHECK(lease.get() != nullptr);
  if (!lease.get()) { std::printf("%d FAILURES\n", g_fail); return 1; }
  int equal_engine = 0, equal_oracle = 0;
  for (int b = 0; b < kPaths; b++) {
    CHECK(r.samples_per_path[b] == 500 + 10 * b);
    Alone a;
    CHECK(EngineAlone(lease.get(), paths[b], &a) == 0);
    Compare(r, b, a, &equal_engine);
    Compare(r, b, oracle[b], &equal_oracle);
  }
  std::printf("bit-equal to the path alone: %d of %d; to the oracle: %d of %d\n", equal_engine, kPaths, equal_oracle,
              kPaths);
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
