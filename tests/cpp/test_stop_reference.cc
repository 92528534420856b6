// Driver for tests/test_stop_reference_cpu.py: runs a backward stop three ways on the cases of an
// input file and prints every result as hex floats, so that the Python restatement
// (tests/stop_reference.py) can compare bit for bit:
//   M  the mirror's TrajectoryBuffer (host/trajectory_buffer.cc, host/rescale_to_stop.cc): loaded
//      with one InsertSegment (sequence number 0), then StopAtIndex / StopBeforeTime;
//   S  rs_stop_serial (csrc/tpamd_rescale.h), the scalar parts of k_stop_trajectories composed on
//      the host;
//   B  bs_stop_in_place (csrc/tpamd_buffer.h), the code k_bset_stop runs, on the same buffer.
//
// Input (whitespace separated, doubles as C99 hex floats):
//   num_cases
//   per case: n D by_index stop_index stop_time time_step,
//             time[n], q[n*D], qd[n*D], qdd[n*D], amax[D]
// Output, three lines per case:
//   M status sequence count  time[count] q[count*D] qd[count*D] qdd[count*D]
//   S status keep first last  time[m] qd[m*D] qdd[m*D]        (m = last - first + 1 rows)
//   B status sequence count  time[count] q[count*D] qd[count*D] qdd[count*D]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_buffer.h"
#include "../../x-edr-trajectory-planning_amd/host/trajectory_buffer.h"

using namespace trajectory_planning;
using tpamd::compat::StatusCode;

static double ReadDouble(FILE *f) {
  double v = 0.0;
  if (std::fscanf(f, "%la", &v) != 1) { std::fprintf(stderr, "bad input\n"); std::exit(2); }
  return v;
}

static int Code(const Status &s) {
  switch (s.code()) {
    case StatusCode::kOk: return tpamd::kRsOk;
    case StatusCode::kFailedPrecondition: return 1;
    case StatusCode::kOutOfRange: return tpamd::kRsOutOfRange;
    case StatusCode::kInvalidArgument: return tpamd::kRsInvalidArgument;
    case StatusCode::kInternal: return tpamd::kRsInternal;
    case StatusCode::kNotFound: return tpamd::kRsNotFound;
    default: return 99;
  }
}

static void Print(const double *v, size_t n) {
  for (size_t i = 0; i < n; i++) std::printf(" %a", v[i]);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int cases = 0;
  if (std::fscanf(f, "%d", &cases) != 1) return 2;
  for (int c = 0; c < cases; c++) {
    int n = 0, D = 0, by_index = 0, stop_index = 0;
    if (std::fscanf(f, "%d %d %d %d", &n, &D, &by_index, &stop_index) != 4) return 2;
    const double stop_time = ReadDouble(f), time_step = ReadDouble(f);
    std::vector<double> t(n), q((size_t)n * D), qd((size_t)n * D), qdd((size_t)n * D), amax(D);
    for (auto *v : {&t, &q, &qd, &qdd, &amax})
      for (double &x : *v) x = ReadDouble(f);

    // M: the mirror
    {
      std::vector<VectorXd> Q(n), V(n), A(n);
      for (int i = 0; i < n; i++) {
        Q[i] = VectorXd(&q[(size_t)i * D], D);
        V[i] = VectorXd(&qd[(size_t)i * D], D);
        A[i] = VectorXd(&qdd[(size_t)i * D], D);
      }
      auto buf = *TrajectoryBuffer::Create();
      if (n > 0) {
        buf->InsertSegment(Span<const double>(t.data(), n), Span<const VectorXd>(Q.data(), n),
                           Span<const VectorXd>(V.data(), n), Span<const VectorXd>(A.data(), n));
      }
      const VectorXd am(amax.data(), D);
      const Status st = by_index ? buf->StopAtIndex(stop_index, am, time_step) : buf->StopBeforeTime(stop_time, am, time_step);
      const size_t m = buf->GetNumSamples();
      std::printf("M %d %d %zu", Code(st), buf->GetSequenceNumber(), m);
      Print(buf->GetTimes().data(), m);
      for (size_t i = 0; i < m; i++) Print(buf->GetPositions()[i].data(), D);
      for (size_t i = 0; i < m; i++) Print(buf->GetVelocities()[i].data(), D);
      for (size_t i = 0; i < m; i++) Print(buf->GetAccelerations()[i].data(), D);
      std::printf("\n");
    }
    // S: the scalar parts of k_stop_trajectories
    {
      std::vector<double> ot(n + 1, -7.0), oqd((size_t)(n + 1) * D, -7.0), oqdd((size_t)(n + 1) * D, -7.0);
      int keep = -7, first = -7, last = -7;
      const int st = tpamd::rs_stop_serial(t.data(), qd.data(), qdd.data(), n, D, amax.data(), time_step, by_index != 0,
                                           stop_index, stop_time, &keep, &first, &last, ot.data(), oqd.data(), oqdd.data());
      if (n == 0 && st == tpamd::kRsOk) keep = 0, first = 0, last = -1;    // as the kernel reports no samples
      std::printf("S %d %d %d %d", st, keep, first, last);
      const int m = last - first + 1;
      if (m > 0) {
        Print(&ot[first], m);
        Print(&oqd[(size_t)first * D], (size_t)m * D);
        Print(&oqdd[(size_t)first * D], (size_t)m * D);
      }
      std::printf("\n");
    }
    // B: the code of k_bset_stop
    {
      const int cap = n + 4;
      std::vector<double> bt(cap, -7.0), bq((size_t)cap * D, -7.0), bqd((size_t)cap * D, -7.0), bqdd((size_t)cap * D, -7.0);
      for (int i = 0; i < n; i++) bt[i] = t[i];
      for (size_t i = 0; i < (size_t)n * D; i++) { bq[i] = q[i]; bqd[i] = qd[i]; bqdd[i] = qdd[i]; }
      int first = 0, count = n, sequence = 0, what = 0;
      const tpamd::BufRef ref{&first, &count, &sequence, bt.data(), bq.data(), bqd.data(), bqdd.data(), cap, D, 1e-6};
      const int st = tpamd::bs_stop_in_place_any(ref, by_index != 0, stop_index, stop_time, amax.data(), time_step, &what);
      std::printf("B %d %d %d", st, sequence, count);
      Print(&bt[first], count);
      Print(&bq[(size_t)first * D], (size_t)count * D);
      Print(&bqd[(size_t)first * D], (size_t)count * D);
      Print(&bqdd[(size_t)first * D], (size_t)count * D);
      std::printf("\n");
    }
  }
  std::fclose(f);
  return 0;
}
