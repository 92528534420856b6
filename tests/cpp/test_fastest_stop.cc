// Driver for tests/test_fastest_stop_cpu.py: runs the mirror's FastestStopAtTime
// (host/fastest_stop.h) on the cases of an input file and prints every result as a hex float, so
// that the Python restatement can compare bit for bit.
//
// Input (whitespace separated, doubles as C99 hex floats):
//   num_cases
//   per case: count num_dofs query_time, time[count], s[count], qd[count*D], qdd[count*D], amax[D]
// Output, one line per case:
//   status stop_index stop_parameter duration n  time[n] rate2[n] drate2[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/host/fastest_stop.h"

using namespace trajectory_planning;

static double ReadDouble(FILE *f) {
  double v = 0.0;
  if (std::fscanf(f, "%la", &v) != 1) { std::fprintf(stderr, "bad input\n"); std::exit(2); }
  return v;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int cases = 0;
  if (std::fscanf(f, "%d", &cases) != 1) return 2;
  for (int c = 0; c < cases; c++) {
    int count = 0, D = 0;
    if (std::fscanf(f, "%d %d", &count, &D) != 2) return 2;
    const double query = ReadDouble(f);
    std::vector<double> t(count), s(count), qd((size_t)count * D), qdd((size_t)count * D), amax(D);
    for (auto *v : {&t, &s, &qd, &qdd, &amax})
      for (double &x : *v) x = ReadDouble(f);
    double stop = 0.0, duration = 0.0;
    int index = 0;
    FastestStopProfile prof;
    const int st = FastestStopAtTime(count, D, t.data(), s.data(), qd.data(), qdd.data(), amax.data(), query, &stop,
                                     &index, &duration, &prof);
    std::printf("%d %d %a %a %zu", st, index, stop, duration, prof.time.size());
    for (auto *v : {&prof.time, &prof.rate_squared, &prof.diff_rate_squared})
      for (double x : *v) std::printf(" %a", x);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
