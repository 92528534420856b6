// GPU test of the buffer sets (run by tests/test_gpu_buffer_set.py; argv[1]: the planner paths):
//   fuzz      random rounds of insert / discard / stop / append / offset / clear on lists with a
//             subset of the buffers of a 256-buffer set, through the host-pointer entries on one
//             set and the _device entries on another, next to mirror TrajectoryBuffers
//             (host/trajectory_buffer.h): statuses equal, and after a download every few rounds
//             and at the end times, positions, velocities, accelerations, sample counts and
//             sequence numbers (and GetStartTime / GetEndTime / GetPositionsUpToTime) equal bit
//             for bit;
//   planner   a planner set on the paths of argv[1] (the structured families of
//             tests/structured_paths.py, written by the Python test): Plan -> insert_from ->
//             sample_at_ticks equals the planner set's own sample_at_ticks; replans with
//             discard_before against mirror buffers fed from download_trajectories; the in-place
//             stop against the planner set's stop_trajectories (keep + segment) and against the
//             mirror's stopped buffer at ticks, OUT_OF_RANGE ones included; packed output of
//             stop_trajectories_device / download_trajectories_device inserted on the device
//             against the host route;
//   graph     a linear hipGraph capture of insert -> discard -> sample after reserve, replayed
//             once, against the eager calls; TPAMD_PLAN_MORE leaves a buffer unchanged;
//             device_bytes constant across _device calls; call-level errors.
// Prints a line per part and "ALL OK".
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/trajectory_buffer.h"
#include "../../x-edr-trajectory-planning_amd/host/trajectory_buffer_set.h"

#define TEST_SUPPORT_SEED 20261018ULL
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::StatusCode;

static int Code(const Status &s) {
  switch (s.code()) {
    case StatusCode::kOk: return TPAMD_PLAN_OK;
    case StatusCode::kFailedPrecondition: return TPAMD_PLAN_FAILED_PRECONDITION;
    case StatusCode::kOutOfRange: return TPAMD_PLAN_OUT_OF_RANGE;
    case StatusCode::kInvalidArgument: return TPAMD_PLAN_INVALID_ARGUMENT;
    case StatusCode::kInternal: return TPAMD_PLAN_INTERNAL;
    case StatusCode::kNotFound: return TPAMD_PLAN_NOT_FOUND;
    default: return 99;
  }
}

// device copies of host vectors, freed together
struct DeviceArrays {
  std::vector<void *> all;
  template <typename T>
  T *up(const std::vector<T> &v) {
    T *p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (!v.empty()) HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    all.push_back(p);
    return p;
  }
  template <typename T>
  T *room(size_t n) { return up(std::vector<T>(n)); }
  template <typename T>
  std::vector<T> down(const T *p, size_t n) {
    std::vector<T> v(n);
    HIP_OK(hipDeviceSynchronize());
    if (n) HIP_OK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
  }
  ~DeviceArrays() {
    (void)hipDeviceSynchronize();
    for (void *p : all) (void)hipFree(p);
  }
};

struct Packed {   // packed rows of several buffers / segments
  std::vector<int64_t> offsets;
  std::vector<double> time, q, qd, qdd;
};

static bool Equal(const Packed &a, const Packed &b) {
  return a.offsets == b.offsets && a.time.size() == b.time.size() &&
         (a.time.empty() || (!std::memcmp(a.time.data(), b.time.data(), a.time.size() * 8) &&
                             !std::memcmp(a.q.data(), b.q.data(), a.q.size() * 8) &&
                             !std::memcmp(a.qd.data(), b.qd.data(), a.qd.size() * 8) &&
                             !std::memcmp(a.qdd.data(), b.qdd.data(), a.qdd.size() * 8)));
}

static Packed PackMirror(const std::vector<std::shared_ptr<TrajectoryBuffer>> &m, const std::vector<int32_t> &ids) {
  Packed p;
  p.offsets.push_back(0);
  for (int32_t b : ids) {
    const TrajectoryBuffer &buf = *m[b];
    for (size_t i = 0; i < buf.GetNumSamples(); i++) {
      p.time.push_back(buf.GetTimes()[i]);
      p.q.insert(p.q.end(), buf.GetPositions()[i].begin(), buf.GetPositions()[i].end());
      p.qd.insert(p.qd.end(), buf.GetVelocities()[i].begin(), buf.GetVelocities()[i].end());
      p.qdd.insert(p.qdd.end(), buf.GetAccelerations()[i].begin(), buf.GetAccelerations()[i].end());
    }
    p.offsets.push_back((int64_t)p.time.size());
  }
  return p;
}

// the whole set through the host-pointer download, or through the _device download
static Packed Download(tpamd_buffer_set *bs, const std::vector<int32_t> &ids, int D, bool device) {
  Packed p;
  const int n = (int)ids.size();
  p.offsets.assign(n + 1, -1);
  if (!device) {
    double dummy = 0;
    const int rc = tpamd_buffer_set_download(bs, n, ids.data(), p.offsets.data(), 0, &dummy, &dummy, &dummy, &dummy);
    CHECK(rc == 0 || rc == TPAMD_E_INVALID_ARGUMENT);
    const size_t rows = (size_t)p.offsets[n];
    p.time.resize(rows); p.q.resize(rows * D); p.qd.resize(rows * D); p.qdd.resize(rows * D);
    if (rows)
      CHECK(tpamd_buffer_set_download(bs, n, ids.data(), p.offsets.data(), (int64_t)rows, p.time.data(), p.q.data(),
                                      p.qd.data(), p.qdd.data()) == 0);
    return p;
  }
  DeviceArrays d;
  int32_t *d_ids = d.up(ids), *d_cnt = d.room<int32_t>(n);
  CHECK(tpamd_buffer_set_info_device(bs, n, d_ids, nullptr, d_cnt, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  size_t cap = 1;
  for (int32_t c : d.down(d_cnt, n)) cap += (size_t)c;
  int64_t *d_off = d.room<int64_t>(n + 1);
  double *t = d.room<double>(cap), *q = d.room<double>(cap * D), *qd = d.room<double>(cap * D), *qdd = d.room<double>(cap * D);
  CHECK(tpamd_buffer_set_download_device(bs, n, d_ids, d_off, (int64_t)cap, t, q, qd, qdd, nullptr) == 0);
  p.offsets = d.down(d_off, n + 1);
  const size_t rows = (size_t)p.offsets[n];
  CHECK(rows <= cap);
  p.time = d.down(t, rows); p.q = d.down(q, rows * D); p.qd = d.down(qd, rows * D); p.qdd = d.down(qdd, rows * D);
  return p;
}

struct Rows {
  std::vector<double> time, q, qd, qdd;
};
// n rows from `front` on (the generator of tests/cpp/test_buffer_core.cc)
static Rows MakeRows(int n, int D, double front) {
  Rows f;
  const double dt = RndInt(0, 1) ? 1e-3 * RndInt(1, 8) : 1e-3 * (0.5 + Rnd());
  for (int i = 0; i < n; i++) f.time.push_back(i == 0 ? front : f.time[i - 1] + dt * (RndInt(0, 1) ? 1.0 : 0.5 + Rnd()));
  if (n > 3 && RndInt(0, 60) == 0) f.time[RndInt(2, n - 1)] = f.time[1];
  f.q.resize((size_t)n * D); f.qd.resize((size_t)n * D); f.qdd.resize((size_t)n * D);
  const int shape = RndInt(0, 2);
  for (int j = 0; j < D; j++) {
    const double v0 = (2.0 * Rnd() - 1.0) * (shape == 2 ? 3.0 : 1.0);
    for (int i = 0; i < n; i++) {
      const double frac = n > 1 ? (double)i / (n - 1) : 0.0;
      const double v = shape == 0 ? v0 : shape == 1 ? v0 * (1.0 - frac) : v0 * (0.5 + Rnd());
      f.qd[(size_t)i * D + j] = v;
      f.qdd[(size_t)i * D + j] = shape == 1 ? -v0 / std::max(1e-3, f.time[n - 1] - f.time[0]) : (2.0 * Rnd() - 1.0);
      f.q[(size_t)i * D + j] = 10.0 * Rnd();
    }
  }
  if (n > 0 && RndInt(0, 5) == 0)
    for (int j = 0; j < D; j++) f.qd[(size_t)(n - 1) * D + j] = RndInt(0, 1) ? 0.0 : 5e-5 * (2.0 * Rnd() - 1.0);
  if (n > 2 && RndInt(0, 6) == 0) {
    const int r = RndInt(1, n - 2);
    for (int j = 0; j < D; j++) f.qd[(size_t)r * D + j] = RndInt(0, 1) ? 0.0 : 5e-9;
  }
  return f;
}

static Status MirrorInsert(TrajectoryBuffer &m, const double *t, const double *q, const double *qd, const double *qdd,
                           size_t n, int D) {
  std::vector<VectorXd> Q, V, A;
  for (size_t i = 0; i < n; i++) {
    Q.push_back(VectorXd(q + i * D, D));
    V.push_back(VectorXd(qd + i * D, D));
    A.push_back(VectorXd(qdd + i * D, D));
  }
  return m.InsertSegment(Span<const double>(t, n), Span<const VectorXd>(Q.data(), n), Span<const VectorXd>(V.data(), n),
                         Span<const VectorXd>(A.data(), n));
}

// ------------------------------------------------------------------ fuzz
static void Fuzz(tpamd_engine *e, int B, int D, int rounds) {
  const double tol = 1e-6;
  tpamd_buffer_set *hs = nullptr, *ds = nullptr;
  CHECK(tpamd_buffer_set_create(e, B, D, 16, tol, &hs) == 0);       // grows through the host entries
  CHECK(tpamd_buffer_set_create(e, B, D, 64, tol, &ds) == 0);
  CHECK(tpamd_buffer_set_reserve(ds, 2048) == 0 && tpamd_buffer_set_capacity(ds) == 2048);
  const size_t ds_bytes = tpamd_buffer_set_device_bytes(ds);
  std::vector<std::shared_ptr<TrajectoryBuffer>> mirror(B);
  for (auto &m : mirror) m = *TrajectoryBuffer::Create(TrajectoryBufferOptions{tol});
  std::vector<int32_t> all(B);
  for (int b = 0; b < B; b++) all[b] = b;
  long ops = 0, more = 0;
  for (int round = 0; round < rounds; round++) {
    // a subset of the buffers in random order (now and then all of them through a NULL list)
    std::vector<int32_t> ids = all;
    for (int b = B - 1; b > 0; b--) std::swap(ids[b], ids[RndInt(0, b)]);
    const bool whole = RndInt(0, 7) == 0;
    if (whole) ids = all; else ids.resize(RndInt(1, B));
    const int n = (int)ids.size();
    const int32_t *h_ids = whole ? nullptr : ids.data();
    DeviceArrays d;
    const int32_t *d_ids = whole ? nullptr : d.up(ids);
    int32_t *d_status = d.room<int32_t>(n);
    std::vector<int32_t> st_m(n, 0), st_h(n, -1), st_d;
    const int kind = round < 3 ? 0 : RndInt(0, 99);
    if (kind < 40) {  // insert
      Packed seg;
      seg.offsets.push_back(0);
      for (int k = 0; k < n; k++) {
        TrajectoryBuffer &m = *mirror[ids[k]];
        const size_t cnt = m.GetNumSamples();
        const auto t = m.GetTimes();
        const int rows = RndInt(0, 11) == 0 ? 0 : RndInt(1, 30);
        double front = 1.0 + Rnd();
        if (cnt > 0) {
          const size_t i = (size_t)RndInt(0, (int)cnt - 1);
          switch (RndInt(0, 7)) {
            case 0: front = RndInt(0, 1) ? t[0] : t[0] - 1e-3 * Rnd(); break;
            case 1: front = t[cnt - 1]; break;
            case 2: front = t[i] + 0.3 * tol; break;
            case 3: front = t[i] + 1.5 * tol; break;
            case 4: case 5: front = i + 1 < cnt ? t[i] + (t[i + 1] - t[i]) * (0.2 + 0.6 * Rnd()) : t[i] + 1e-3; break;
            default: front = t[cnt - 1] + 1e-3 * (0.5 + Rnd()); break;
          }
        }
        const Rows r = MakeRows(rows, D, front);
        st_m[k] = Code(MirrorInsert(m, r.time.data(), r.q.data(), r.qd.data(), r.qdd.data(), rows, D));
        seg.time.insert(seg.time.end(), r.time.begin(), r.time.end());
        seg.q.insert(seg.q.end(), r.q.begin(), r.q.end());
        seg.qd.insert(seg.qd.end(), r.qd.begin(), r.qd.end());
        seg.qdd.insert(seg.qdd.end(), r.qdd.begin(), r.qdd.end());
        seg.offsets.push_back((int64_t)seg.time.size());
      }
      double dummy = 0;
      const bool none = seg.time.empty();
      CHECK(tpamd_buffer_set_insert(hs, n, h_ids, seg.offsets.data(), none ? &dummy : seg.time.data(),
                                    none ? &dummy : seg.q.data(), none ? &dummy : seg.qd.data(),
                                    none ? &dummy : seg.qdd.data(), st_h.data()) == 0);
      CHECK(tpamd_buffer_set_insert_device(ds, n, d_ids, d.up(seg.offsets), (int64_t)seg.time.size(), d.up(seg.time),
                                           d.up(seg.q), d.up(seg.qd), d.up(seg.qdd), d_status, nullptr) == 0);
    } else if (kind < 60) {  // discard, in seconds or nanoseconds
      const bool in_ns = RndInt(0, 1);
      std::vector<double> sec(n);
      std::vector<int64_t> ns(n);
      for (int k = 0; k < n; k++) {
        TrajectoryBuffer &m = *mirror[ids[k]];
        const size_t cnt = m.GetNumSamples();
        const auto t = m.GetTimes();
        double time = Rnd();
        if (cnt > 0) {
          const size_t i = (size_t)RndInt(0, (int)cnt - 1);
          switch (RndInt(0, 9)) {
            case 0: time = RndInt(0, 1) ? t[0] : t[0] - 1e-3 * Rnd(); break;
            case 1: time = t[cnt - 1] + 1e-9 + 1e-3 * Rnd() * RndInt(0, 1); break;
            case 2: case 3: time = t[i]; break;
            case 4: time = t[i] + 0.5 * tol; break;
            case 5: time = t[i] - 0.5 * tol; break;
            default: time = i + 1 < cnt ? t[i] + (t[i + 1] - t[i]) * (0.1 + 0.8 * Rnd()) : t[i]; break;
          }
        }
        sec[k] = time;
        ns[k] = (int64_t)(time * 1e9);
        if (in_ns) m.DiscardSegmentBefore(FromUnixNanos(ns[k])); else m.DiscardSegmentBefore(time);
      }
      st_h.assign(n, 0);
      CHECK(tpamd_buffer_set_discard_before(hs, n, h_ids, in_ns ? ns.data() : nullptr, in_ns ? nullptr : sec.data()) == 0);
      CHECK(tpamd_buffer_set_discard_before_device(ds, n, d_ids, in_ns ? d.up(ns) : nullptr, in_ns ? nullptr : d.up(sec),
                                                   d_status, nullptr) == 0);
    } else if (kind < 82) {  // stop in place
      const double time_step = RndInt(0, 30) == 0 ? 0.0 : 1e-3;
      const bool in_ns = RndInt(0, 2) == 0;
      std::vector<double> sec(n), amax((size_t)n * D);
      std::vector<int64_t> ns(n);
      for (int k = 0; k < n; k++) {
        TrajectoryBuffer &m = *mirror[ids[k]];
        const size_t cnt = m.GetNumSamples();
        const auto t = m.GetTimes();
        for (int j = 0; j < D; j++) amax[(size_t)k * D + j] = 0.5 + 5.0 * Rnd();
        if (RndInt(0, 40) == 0) amax[(size_t)k * D + RndInt(0, D - 1)] = RndInt(0, 1) ? 0.0 : -1.0;
        double time = Rnd();
        if (cnt > 0) {
          const int where = RndInt(0, 6);
          const size_t i = (size_t)RndInt(0, (int)cnt - 1);
          time = where == 0 ? t[0] - 1e-3 * Rnd() - 1e-9 : where == 1 ? t[i] : where == 2 ? t[cnt - 1] + 0.5 * Rnd()
                 : where == 3 ? t[cnt - 1] : (i + 1 < cnt ? t[i] + (t[i + 1] - t[i]) * Rnd() : t[i]);
          if (where == 5)
            for (size_t r = 1; r + 1 < cnt; r++)
              if (m.GetVelocities()[r].maxAbs() < 1e-8) { time = t[r - 1]; break; }
        }
        sec[k] = time;
        ns[k] = (int64_t)(time * 1e9);
        const VectorXd am(&amax[(size_t)k * D], D);
        st_m[k] = Code(in_ns ? m.StopBeforeTime(FromUnixNanos(ns[k]), am, time_step) : m.StopBeforeTime(time, am, time_step));
      }
      CHECK(tpamd_buffer_set_stop_before_time(hs, n, h_ids, in_ns ? ns.data() : nullptr, in_ns ? nullptr : sec.data(),
                                              amax.data(), time_step, st_h.data()) == 0);
      CHECK(tpamd_buffer_set_stop_before_time_device(ds, n, d_ids, in_ns ? d.up(ns) : nullptr,
                                                     in_ns ? nullptr : d.up(sec), d.up(amax), time_step, d_status,
                                                     nullptr) == 0);
    } else if (kind < 90) {  // append
      Rows rows;
      for (int k = 0; k < n; k++) {
        TrajectoryBuffer &m = *mirror[ids[k]];
        const size_t cnt = m.GetNumSamples();
        const double back = cnt ? m.GetTimes()[cnt - 1] : 0.0;
        const double time = cnt == 0 ? Rnd() : RndInt(0, 3) ? back + 1e-3 * (0.5 + Rnd()) : (RndInt(0, 1) ? back : back - 1e-3 * Rnd());
        const Rows r = MakeRows(1, D, time);
        st_m[k] = Code(m.AppendSample(time, VectorXd(r.q.data(), D), VectorXd(r.qd.data(), D), VectorXd(r.qdd.data(), D)));
        rows.time.push_back(time);
        rows.q.insert(rows.q.end(), r.q.begin(), r.q.end());
        rows.qd.insert(rows.qd.end(), r.qd.begin(), r.qd.end());
        rows.qdd.insert(rows.qdd.end(), r.qdd.begin(), r.qdd.end());
      }
      CHECK(tpamd_buffer_set_append_sample(hs, n, h_ids, rows.time.data(), rows.q.data(), rows.qd.data(), rows.qdd.data(),
                                           st_h.data()) == 0);
      CHECK(tpamd_buffer_set_append_sample_device(ds, n, d_ids, d.up(rows.time), d.up(rows.q), d.up(rows.qd),
                                                  d.up(rows.qdd), d_status, nullptr) == 0);
    } else if (kind < 97) {  // offset, in seconds or as a duration
      const bool in_ns = RndInt(0, 1);
      std::vector<double> sec(n);
      std::vector<int64_t> ns(n);
      for (int k = 0; k < n; k++) {
        sec[k] = 2.0 * Rnd() - 1.0;
        ns[k] = (int64_t)RndInt(-500, 500) * kMs;
        if (in_ns) mirror[ids[k]]->AddOffsetToTimestamps(tpamd::compat::Nanoseconds(ns[k]));
        else mirror[ids[k]]->AddOffsetToTimestamps(sec[k]);
      }
      st_h.assign(n, 0);
      CHECK(tpamd_buffer_set_add_offset(hs, n, h_ids, in_ns ? ns.data() : nullptr, in_ns ? nullptr : sec.data()) == 0);
      CHECK(tpamd_buffer_set_add_offset_device(ds, n, d_ids, in_ns ? d.up(ns) : nullptr, in_ns ? nullptr : d.up(sec),
                                               d_status, nullptr) == 0);
    } else {  // clear
      for (int k = 0; k < n; k++) mirror[ids[k]]->Clear();
      st_h.assign(n, 0);
      CHECK(tpamd_buffer_set_clear(hs, n, h_ids) == 0);
      CHECK(tpamd_buffer_set_clear_device(ds, n, d_ids, d_status, nullptr) == 0);
    }
    st_d = d.down(d_status, n);
    for (int k = 0; k < n; k++) more += st_d[k] == TPAMD_PLAN_MORE;
    CHECK(st_h == st_m);
    CHECK(st_d == st_m);
    ops += n;
    if (round % 6 == 5 || round == rounds - 1) {
      const Packed want = PackMirror(mirror, all);
      CHECK(Equal(Download(hs, all, D, false), want));
      CHECK(Equal(Download(ds, all, D, true), want));
      // the info readout against the mirror's getters
      std::vector<int64_t> at(B), s0(B), s1(B);
      std::vector<int32_t> cnt(B), seq(B), up(B);
      for (int b = 0; b < B; b++) {
        const auto t = mirror[b]->GetTimes();
        at[b] = t.size() ? (int64_t)((t[0] + (t[t.size() - 1] - t[0]) * (1.2 * Rnd() - 0.1)) * 1e9) : 0;
      }
      CHECK(tpamd_buffer_set_info(hs, B, nullptr, at.data(), cnt.data(), seq.data(), s0.data(), s1.data(), up.data()) == 0);
      DeviceArrays di;
      int32_t *d_cnt = di.room<int32_t>(B), *d_seq = di.room<int32_t>(B), *d_up = di.room<int32_t>(B);
      int64_t *d_s0 = di.room<int64_t>(B), *d_s1 = di.room<int64_t>(B);
      CHECK(tpamd_buffer_set_info_device(ds, B, nullptr, di.up(at), d_cnt, d_seq, d_s0, d_s1, d_up, nullptr) == 0);
      CHECK(di.down(d_cnt, B) == cnt && di.down(d_seq, B) == seq && di.down(d_up, B) == up && di.down(d_s0, B) == s0 &&
            di.down(d_s1, B) == s1);
      for (int b = 0; b < B; b++) {
        const TrajectoryBuffer &m = *mirror[b];
        CHECK((size_t)cnt[b] == m.GetNumSamples() && seq[b] == m.GetSequenceNumber());
        CHECK(s0[b] == tpamd::compat::ToUnixNanos(m.GetStartTime()) && s1[b] == tpamd::compat::ToUnixNanos(m.GetEndTime()));
        CHECK((size_t)up[b] == m.GetPositionsUpToTime(FromUnixNanos(at[b])).size());
      }
    }
  }
  CHECK(more == 0);
  CHECK(tpamd_buffer_set_device_bytes(ds) == ds_bytes);     // no _device call allocates
  CHECK(tpamd_buffer_set_capacity(hs) > 16);                // the host entries grew their set
  std::printf("fuzz vs mirror (B %d, D %d): %d rounds, %ld buffer operations, host set capacity %d\n", B, D, rounds, ops,
              tpamd_buffer_set_capacity(hs));
  tpamd_buffer_set_destroy(hs);
  tpamd_buffer_set_destroy(ds);
}

// ------------------------------------------------------------------ with a planner set
struct Paths {
  int B = 0, D = 0, N = 0;
  std::vector<int32_t> num_points;
  std::vector<double> knots, cps, vmax, amax, delta;
};
static bool ReadPaths(const char *file, Paths *p) {
  FILE *f = std::fopen(file, "rb");
  if (!f) return false;
  int32_t head[3];
  bool ok = std::fread(head, 4, 3, f) == 3;
  p->B = head[0]; p->D = head[1]; p->N = head[2];
  p->num_points.resize(p->B);
  ok = ok && std::fread(p->num_points.data(), 4, p->B, f) == (size_t)p->B;
  size_t points = 0;
  for (int32_t n : p->num_points) points += n;
  auto rd = [&](std::vector<double> &v, size_t n) { v.resize(n); ok = ok && std::fread(v.data(), 8, n, f) == n; };
  rd(p->knots, points + 3 * p->B);
  rd(p->cps, points * p->D);
  rd(p->vmax, (size_t)p->B * p->D);
  rd(p->amax, (size_t)p->B * p->D);
  rd(p->delta, p->B);
  std::fclose(f);
  return ok;
}

static Packed PlannerTrajectories(tpamd_planner_set *ps, int B, int D) {
  Packed p;
  p.offsets.assign(B + 1, 0);
  double dummy = 0;
  const int rc = tpamd_planner_set_download_trajectories(ps, B, nullptr, p.offsets.data(), 0, &dummy, nullptr, nullptr,
                                                         nullptr, &dummy, &dummy, &dummy);
  CHECK(rc == 0 || rc == TPAMD_E_INVALID_ARGUMENT);
  const size_t rows = (size_t)p.offsets[B];
  p.time.resize(rows); p.q.resize(rows * D); p.qd.resize(rows * D); p.qdd.resize(rows * D);
  if (rows)
    CHECK(tpamd_planner_set_download_trajectories(ps, B, nullptr, p.offsets.data(), (int64_t)rows, p.time.data(), nullptr,
                                                  nullptr, nullptr, p.q.data(), p.qd.data(), p.qdd.data()) == 0);
  return p;
}

static void WithPlanners(tpamd_engine *e, const Paths &P) {
  const int B = P.B, D = P.D;
  // a coarse time step: the slowest families (limits spread over four decades) move for minutes
  const int64_t t0 = 1000 * kMs, step = 64 * kMs;
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = P.N; cfg.num_points = 16;
  cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8; cfg.max_initial_velocity_error = 1e-2;
  cfg.time_step_ns = step;
  tpamd_planner_set *ps = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &ps) == 0);
  std::vector<int32_t> state(B, 1);
  std::vector<double> iv((size_t)B * D, 0.0);
  CHECK(tpamd_planner_set_upload_paths_ragged(ps, B, nullptr, P.num_points.data(), P.knots.data(), P.cps.data(),
                                              P.vmax.data(), P.amax.data(), P.delta.data(), iv.data(), state.data()) == 0);
  std::vector<int32_t> all(B), st(B), st2(B);
  for (int b = 0; b < B; b++) all[b] = b;
  tpamd_buffer_set *bs = nullptr, *bd = nullptr;
  CHECK(tpamd_buffer_set_create(e, B, D, 32, 1e-6, &bs) == 0);      // host entries: grows
  CHECK(tpamd_buffer_set_create(e, B, D, 64, 1e-6, &bd) == 0);      // _device entries: reserved after the first Plan
  std::vector<std::shared_ptr<TrajectoryBuffer>> mirror(B);
  for (auto &m : mirror) m = *TrajectoryBuffer::Create();
  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  DeviceArrays d;
  int32_t *d_st = d.room<int32_t>(B);
  long planned = 0, ticks_ok = 0, ticks_out = 0;
  const int T = 48;
  for (int round = 0; round < 5; round++) {
    const int64_t now = t0 + round * 600 * kMs;
    std::vector<int64_t> start(B, now), horizon(B, 2000 * kMs);
    std::vector<tpamd_planner_summary> sum(B);
    if (round > 0) {   // the controller has consumed the samples before `now`
      CHECK(tpamd_buffer_set_discard_before(bs, B, nullptr, start.data(), nullptr) == 0);
      CHECK(tpamd_buffer_set_discard_before_device(bd, B, nullptr, d.up(start), nullptr, nullptr, stream) == 0);
      for (auto &m : mirror) m->DiscardSegmentBefore(FromUnixNanos(now));
    }
    CHECK(tpamd_planner_set_plan(ps, start.data(), horizon.data(), sum.data()) == 0);
    int longest = 0;
    for (int b = 0; b < B; b++) {
      planned += sum[b].status == TPAMD_PLAN_OK;
      longest = std::max(longest, sum[b].num_samples);
    }
    if (round == 0) CHECK(tpamd_buffer_set_reserve(bd, longest + 64) == 0);   // the _device entries never allocate
    CHECK(tpamd_buffer_set_insert_from_planner_set(bs, ps, B, nullptr, nullptr, st.data()) == 0);
    // the device variant on a non-blocking stream, with the next change of the planner set
    // (a reset that lists no planner) right behind it
    CHECK(tpamd_buffer_set_insert_from_planner_set_device(bd, ps, B, nullptr, nullptr, d_st, stream) == 0);
    const int32_t nobody = 0;
    CHECK(tpamd_planner_set_reset(ps, 0, &nobody) == 0);
    HIP_OK(hipStreamSynchronize(stream));
    st2 = d.down(d_st, B);
    const Packed traj = PlannerTrajectories(ps, B, D);
    for (int b = 0; b < B; b++) {
      const size_t o = (size_t)traj.offsets[b], n = (size_t)(traj.offsets[b + 1] - traj.offsets[b]);
      const Status ms = MirrorInsert(*mirror[b], traj.time.data() + o, traj.q.data() + o * D, traj.qd.data() + o * D,
                                     traj.qdd.data() + o * D, n, D);
      CHECK(Code(ms) == st[b]);
      CHECK(st2[b] == st[b]);
    }
    const Packed want = PackMirror(mirror, all);
    CHECK(Equal(Download(bs, all, D, false), want));
    CHECK(Equal(Download(bd, all, D, true), want));
    // setpoints: the buffers against the planner set itself on the times both hold (from the
    // new trajectory's start on the buffer holds exactly the planner's samples)
    std::vector<int64_t> s0(B);
    for (int b = 0; b < B; b++)   // just inside the new trajectory's first sample
      s0[b] = traj.offsets[b + 1] > traj.offsets[b] ? (int64_t)(traj.time[traj.offsets[b]] * 1e9) + 2 : now;
    std::vector<double> q1((size_t)B * T * D, -1), v1 = q1, a1 = q1, q2 = q1, v2 = q1, a2 = q1;
    std::vector<int32_t> ts1((size_t)B * T), ts2 = ts1;
    CHECK(tpamd_planner_set_sample_at_ticks(ps, B, nullptr, s0.data(), step / 2, T, q1.data(), v1.data(), a1.data(), ts1.data()) == 0);
    CHECK(tpamd_buffer_set_sample_at_ticks(bs, B, nullptr, s0.data(), step / 2, T, q2.data(), v2.data(), a2.data(), ts2.data()) == 0);
    for (int b = 0; b < B; b++) {
      if (traj.offsets[b + 1] == traj.offsets[b]) continue;        // no trajectory: the buffer keeps its samples
      const size_t o = (size_t)b * T;
      CHECK(!std::memcmp(&ts1[o], &ts2[o], T * 4) && !std::memcmp(&q1[o * D], &q2[o * D], T * D * 8) &&
            !std::memcmp(&v1[o * D], &v2[o * D], T * D * 8) && !std::memcmp(&a1[o * D], &a2[o * D], T * D * 8));
      for (int j = 0; j < T; j++) (ts1[o + j] == TPAMD_PLAN_OK ? ticks_ok : ticks_out)++;
    }
  }
  CHECK(planned > 0 && ticks_ok > 0);
  std::printf("planner set -> buffers: %d planners, 5 plans, %ld ok, setpoint ticks %ld ok / %ld not\n", B, planned,
              ticks_ok, ticks_out);

  // the stop in place against stop_trajectories (keep + segment) on the same trajectories
  {
    tpamd_buffer_set *b1 = nullptr;
    CHECK(tpamd_buffer_set_create(e, B, D, 0, 1e-6, &b1) == 0);
    CHECK(tpamd_buffer_set_insert_from_planner_set(b1, ps, B, nullptr, nullptr, st.data()) == 0);
    const Packed traj = PlannerTrajectories(ps, B, D);
    std::vector<int64_t> when(B);
    std::vector<double> amax((size_t)B * D);
    for (int b = 0; b < B; b++) {
      const size_t n = (size_t)(traj.offsets[b + 1] - traj.offsets[b]);
      const double first = n ? traj.time[traj.offsets[b]] : 1.0, last = n ? traj.time[traj.offsets[b + 1] - 1] : 1.0;
      when[b] = (int64_t)((first + (last - first) * (1.3 * Rnd() - 0.1)) * 1e9);
      for (int j = 0; j < D; j++) amax[(size_t)b * D + j] = (b % 5 == 4 ? 0.05 : 2.0) * P.amax[(size_t)b * D + j];
    }
    std::vector<int32_t> sst(B), keep(B), bst(B);
    Packed seg;
    seg.offsets.assign(B + 1, 0);
    double dummy = 0;
    int rc = tpamd_planner_set_stop_trajectories(ps, B, nullptr, when.data(), amax.data(), 4e-3, sst.data(), keep.data(),
                                                 seg.offsets.data(), 0, &dummy, &dummy, &dummy, &dummy);
    CHECK(rc == 0 || rc == TPAMD_E_INVALID_ARGUMENT);
    const size_t rows = (size_t)seg.offsets[B];
    seg.time.resize(rows + 1); seg.q.resize((rows + 1) * D); seg.qd.resize((rows + 1) * D); seg.qdd.resize((rows + 1) * D);
    CHECK(tpamd_planner_set_stop_trajectories(ps, B, nullptr, when.data(), amax.data(), 4e-3, sst.data(), keep.data(),
                                              seg.offsets.data(), (int64_t)rows, seg.time.data(), seg.q.data(),
                                              seg.qd.data(), seg.qdd.data()) == 0);
    CHECK(tpamd_buffer_set_stop_before_time(b1, B, nullptr, when.data(), nullptr, amax.data(), 4e-3, bst.data()) == 0);
    CHECK(bst == sst);
    Packed want;
    want.offsets.push_back(0);
    std::vector<std::shared_ptr<TrajectoryBuffer>> stopped(B);
    long ok = 0, failed = 0;
    for (int b = 0; b < B; b++) {
      const size_t o = (size_t)traj.offsets[b], n = (size_t)(traj.offsets[b + 1] - traj.offsets[b]);
      const size_t so = (size_t)seg.offsets[b], sn = (size_t)(seg.offsets[b + 1] - seg.offsets[b]);
      CHECK((size_t)keep[b] <= n);
      want.time.insert(want.time.end(), traj.time.begin() + o, traj.time.begin() + o + keep[b]);
      want.time.insert(want.time.end(), seg.time.begin() + so, seg.time.begin() + so + sn);
      for (auto pr : {std::make_pair(&want.q, std::make_pair(&traj.q, &seg.q)), std::make_pair(&want.qd, std::make_pair(&traj.qd, &seg.qd)),
                      std::make_pair(&want.qdd, std::make_pair(&traj.qdd, &seg.qdd))}) {
        pr.first->insert(pr.first->end(), pr.second.first->begin() + o * D, pr.second.first->begin() + (o + keep[b]) * D);
        pr.first->insert(pr.first->end(), pr.second.second->begin() + so * D, pr.second.second->begin() + (so + sn) * D);
      }
      want.offsets.push_back((int64_t)want.time.size());
      (sst[b] == TPAMD_PLAN_OK ? ok : failed)++;
      // the mirror's stopped buffer, for the setpoints below
      stopped[b] = *TrajectoryBuffer::Create();
      MirrorInsert(*stopped[b], traj.time.data() + o, traj.q.data() + o * D, traj.qd.data() + o * D, traj.qdd.data() + o * D, n, D);
      CHECK(Code(stopped[b]->StopBeforeTime(FromUnixNanos(when[b]), VectorXd(&amax[(size_t)b * D], D), 4e-3)) == bst[b]);
    }
    CHECK(ok > 0 && failed > 0);
    CHECK(Equal(Download(b1, all, D, false), want));
    CHECK(Equal(want, PackMirror(stopped, all)));
    // setpoints on the stopped buffers, beyond their new ends as well
    std::vector<int64_t> s0(B);
    for (int b = 0; b < B; b++) s0[b] = when[b] - 40 * kMs;
    const int T2 = 64;
    std::vector<double> q((size_t)B * T2 * D, -1), v = q, a = q;
    std::vector<int32_t> ts((size_t)B * T2);
    CHECK(tpamd_buffer_set_sample_at_ticks(b1, B, nullptr, s0.data(), 3 * kMs, T2, q.data(), v.data(), a.data(), ts.data()) == 0);
    long in = 0, out = 0;
    for (int b = 0; b < B; b++)
      for (int j = 0; j < T2; j++) {
        const size_t i = (size_t)b * T2 + j;
        const Time at = FromUnixNanos(s0[b] + j * 3 * kMs);
        const auto mq = stopped[b]->GetPositionAtTime(at);
        const auto mv = stopped[b]->GetVelocityAtTime(at);
        const auto ma = stopped[b]->GetAccelerationAtTime(at);
        CHECK(Code(mq.status()) == ts[i]);
        if (mq.ok()) {
          CHECK(!std::memcmp((*mq).data(), &q[i * D], D * 8) && !std::memcmp((*mv).data(), &v[i * D], D * 8) &&
                !std::memcmp((*ma).data(), &a[i * D], D * 8));
          in++;
        } else {
          CHECK(q[i * D] == -1 && ts[i] != TPAMD_PLAN_OK);
          out += ts[i] == TPAMD_PLAN_OUT_OF_RANGE;
        }
      }
    CHECK(in > 0 && out > 0);
    std::printf("stop in place vs stop_trajectories: %ld stopped, %ld not; setpoints %ld ok, %ld out of range\n", ok, failed, in, out);

    // packed device output inserted on the device against the host route
    tpamd_buffer_set *hd = nullptr, *dd = nullptr;
    const int room = tpamd_buffer_set_capacity(bd);
    CHECK(tpamd_buffer_set_create(e, B, D, room, 1e-6, &hd) == 0 && tpamd_buffer_set_create(e, B, D, room, 1e-6, &dd) == 0);
    DeviceArrays x;
    const int64_t cap = (int64_t)traj.time.size() + 64;
    int64_t *d_off = x.room<int64_t>(B + 1);
    int32_t *d_s = x.room<int32_t>(B), *d_keep = x.room<int32_t>(B);
    double *rt = x.room<double>(cap), *rq = x.room<double>(cap * D), *rqd = x.room<double>(cap * D), *rqdd = x.room<double>(cap * D);
    // (1) the trajectories: download_trajectories_device -> insert_device
    CHECK(tpamd_planner_set_download_trajectories_device(ps, B, nullptr, d_off, cap, rt, nullptr, nullptr, nullptr, rq, rqd, rqdd, stream) == 0);
    CHECK(tpamd_buffer_set_insert_device(dd, B, nullptr, d_off, cap, rt, rq, rqd, rqdd, d_s, stream) == 0);
    CHECK(tpamd_buffer_set_insert(hd, B, nullptr, traj.offsets.data(), traj.time.data(), traj.q.data(), traj.qd.data(),
                                  traj.qdd.data(), st.data()) == 0);
    HIP_OK(hipStreamSynchronize(stream));
    CHECK(x.down(d_s, B) == st);
    CHECK(Equal(Download(dd, all, D, true), Download(hd, all, D, false)));
    // (2) the stopping segments: stop_trajectories_device -> insert_device
    CHECK(tpamd_planner_set_stop_trajectories_device(ps, B, nullptr, x.up(when), x.up(amax), 4e-3, d_s, d_keep, d_off, cap,
                                                     rt, rq, rqd, rqdd, stream) == 0);
    CHECK(tpamd_buffer_set_insert_device(dd, B, nullptr, d_off, cap, rt, rq, rqd, rqdd, d_s, stream) == 0);
    CHECK(tpamd_buffer_set_insert(hd, B, nullptr, seg.offsets.data(), seg.time.data(), seg.q.data(), seg.qd.data(),
                                  seg.qdd.data(), st.data()) == 0);
    HIP_OK(hipStreamSynchronize(stream));
    CHECK(x.down(d_s, B) == st);
    const Packed after = Download(dd, all, D, true);
    CHECK(Equal(after, Download(hd, all, D, false)));
    CHECK(after.time == want.time && after.qd == want.qd);        // and it is the stopped trajectory
    std::printf("packed device outputs inserted on the device: equal to the host route\n");
    tpamd_buffer_set_destroy(hd);
    tpamd_buffer_set_destroy(dd);
    tpamd_buffer_set_destroy(b1);
    // another engine, another D: call-level errors
    tpamd_buffer_set *other = nullptr;
    CHECK(tpamd_buffer_set_create(e, 4, D == 3 ? 4 : 3, 0, 1e-6, &other) == 0);
    CHECK(tpamd_buffer_set_insert_from_planner_set(other, ps, 1, nullptr, nullptr, st.data()) == TPAMD_E_INVALID_ARGUMENT);
    tpamd_buffer_set_destroy(other);
  }
  HIP_OK(hipStreamDestroy(stream));
  tpamd_buffer_set_destroy(bs);
  tpamd_buffer_set_destroy(bd);
  tpamd_planner_set_destroy(ps);
}

// ------------------------------------------------------------------ graph capture, capacity, errors
static void GraphAndCapacity(tpamd_engine *e) {
  const int B = 64, D = 6, T = 8;
  tpamd_buffer_set *g = nullptr, *eager = nullptr;
  CHECK(tpamd_buffer_set_create(e, B, D, 8, 1e-6, &g) == 0 && tpamd_buffer_set_create(e, B, D, 8, 1e-6, &eager) == 0);
  CHECK(tpamd_buffer_set_reserve(g, 512) == 0 && tpamd_buffer_set_reserve(eager, 512) == 0);
  std::vector<int32_t> all(B);
  for (int b = 0; b < B; b++) all[b] = b;
  DeviceArrays d;
  Packed seg[2];
  for (int s = 0; s < 2; s++) {
    seg[s].offsets.push_back(0);
    for (int b = 0; b < B; b++) {
      const Rows r = MakeRows(RndInt(5, 40), D, s == 0 ? 1.0 : 1.0 + 1e-3 * RndInt(5, 30));
      seg[s].time.insert(seg[s].time.end(), r.time.begin(), r.time.end());
      seg[s].q.insert(seg[s].q.end(), r.q.begin(), r.q.end());
      seg[s].qd.insert(seg[s].qd.end(), r.qd.begin(), r.qd.end());
      seg[s].qdd.insert(seg[s].qdd.end(), r.qdd.begin(), r.qdd.end());
      seg[s].offsets.push_back((int64_t)seg[s].time.size());
    }
  }
  std::vector<int64_t> disc(B), s0(B);
  for (int b = 0; b < B; b++) { disc[b] = (int64_t)((1.0 + 1e-3 * RndInt(0, 20)) * 1e9); s0[b] = disc[b] - 2 * kMs; }
  const int64_t *d_disc = d.up(disc), *d_s0 = d.up(s0);
  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  struct Out { double *q, *qd, *qdd; int32_t *ts, *st, *st2; } o[2];
  for (int s = 0; s < 2; s++)
    o[s] = Out{d.room<double>((size_t)B * T * D), d.room<double>((size_t)B * T * D), d.room<double>((size_t)B * T * D),
               d.room<int32_t>((size_t)B * T), d.room<int32_t>(B), d.room<int32_t>(B)};
  for (int s = 0; s < 2; s++) {   // both sets start from the same first segment
    tpamd_buffer_set *bs = s == 0 ? g : eager;
    CHECK(tpamd_buffer_set_insert_device(bs, B, nullptr, d.up(seg[0].offsets), (int64_t)seg[0].time.size(), d.up(seg[0].time),
                                         d.up(seg[0].q), d.up(seg[0].qd), d.up(seg[0].qdd), o[s].st, stream) == 0);
  }
  HIP_OK(hipStreamSynchronize(stream));
  const int64_t *d_off = d.up(seg[1].offsets);
  const double *d_t = d.up(seg[1].time), *d_q = d.up(seg[1].q), *d_qd = d.up(seg[1].qd), *d_qdd = d.up(seg[1].qdd);
  auto chain = [&](tpamd_buffer_set *bs, const Out &w) {
    CHECK(tpamd_buffer_set_insert_device(bs, B, nullptr, d_off, (int64_t)seg[1].time.size(), d_t, d_q, d_qd, d_qdd, w.st, stream) == 0);
    CHECK(tpamd_buffer_set_discard_before_device(bs, B, nullptr, d_disc, nullptr, w.st2, stream) == 0);
    CHECK(tpamd_buffer_set_sample_at_ticks_device(bs, B, nullptr, d_s0, kMs, T, w.q, w.qd, w.qdd, w.ts, stream) == 0);
  };
  const size_t bytes = tpamd_buffer_set_device_bytes(g);
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  HIP_OK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
  chain(g, o[0]);
  HIP_OK(hipStreamEndCapture(stream, &graph));
  HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  HIP_OK(hipGraphLaunch(exec, stream));
  HIP_OK(hipStreamSynchronize(stream));
  chain(eager, o[1]);
  HIP_OK(hipStreamSynchronize(stream));
  CHECK(tpamd_buffer_set_device_bytes(g) == bytes);
  const size_t nv = (size_t)B * T * D;
  CHECK(d.down(o[0].ts, (size_t)B * T) == d.down(o[1].ts, (size_t)B * T) && d.down(o[0].st, B) == d.down(o[1].st, B));
  const auto qa = d.down(o[0].q, nv), qb = d.down(o[1].q, nv), va = d.down(o[0].qd, nv), vb = d.down(o[1].qd, nv);
  CHECK(!std::memcmp(qa.data(), qb.data(), nv * 8) && !std::memcmp(va.data(), vb.data(), nv * 8));
  const Packed a = Download(g, all, D, true), b = Download(eager, all, D, true);
  CHECK(Equal(a, b) && !a.time.empty());
  // the same chain on mirror buffers
  std::vector<std::shared_ptr<TrajectoryBuffer>> mirror(B);
  for (int k = 0; k < B; k++) {
    mirror[k] = *TrajectoryBuffer::Create();
    for (int s = 0; s < 2; s++) {
      const size_t off = (size_t)seg[s].offsets[k], n = (size_t)(seg[s].offsets[k + 1] - seg[s].offsets[k]);
      MirrorInsert(*mirror[k], seg[s].time.data() + off, seg[s].q.data() + off * D, seg[s].qd.data() + off * D,
                   seg[s].qdd.data() + off * D, n, D);
    }
    mirror[k]->DiscardSegmentBefore(FromUnixNanos(disc[k]));
  }
  CHECK(Equal(a, PackMirror(mirror, all)));
  HIP_OK(hipGraphExecDestroy(exec));
  HIP_OK(hipGraphDestroy(graph));
  std::printf("graph capture of insert -> discard -> sample: replay equals the eager calls and the mirror\n");

  // TPAMD_PLAN_MORE: a _device insert that does not fit leaves its buffer unchanged; the others go on
  tpamd_buffer_set *small = nullptr;
  CHECK(tpamd_buffer_set_create(e, 4, D, 16, 1e-6, &small) == 0);
  std::vector<int32_t> four = {0, 1, 2, 3};
  Packed first, big;
  first.offsets.push_back(0); big.offsets.push_back(0);
  for (int k = 0; k < 4; k++) {
    const Rows r = MakeRows(6, D, 1.0), r2 = MakeRows(k == 2 ? 20 : 8, D, 1.002);
    first.time.insert(first.time.end(), r.time.begin(), r.time.end()); first.q.insert(first.q.end(), r.q.begin(), r.q.end());
    first.qd.insert(first.qd.end(), r.qd.begin(), r.qd.end()); first.qdd.insert(first.qdd.end(), r.qdd.begin(), r.qdd.end());
    first.offsets.push_back((int64_t)first.time.size());
    big.time.insert(big.time.end(), r2.time.begin(), r2.time.end()); big.q.insert(big.q.end(), r2.q.begin(), r2.q.end());
    big.qd.insert(big.qd.end(), r2.qd.begin(), r2.qd.end()); big.qdd.insert(big.qdd.end(), r2.qdd.begin(), r2.qdd.end());
    big.offsets.push_back((int64_t)big.time.size());
  }
  int32_t *d_st = d.room<int32_t>(4);
  CHECK(tpamd_buffer_set_insert_device(small, 4, nullptr, d.up(first.offsets), (int64_t)first.time.size(), d.up(first.time),
                                       d.up(first.q), d.up(first.qd), d.up(first.qdd), d_st, nullptr) == 0);
  const Packed before = Download(small, four, D, true);
  const size_t small_bytes = tpamd_buffer_set_device_bytes(small);
  CHECK(tpamd_buffer_set_insert_device(small, 4, nullptr, d.up(big.offsets), (int64_t)big.time.size(), d.up(big.time),
                                       d.up(big.q), d.up(big.qd), d.up(big.qdd), d_st, nullptr) == 0);
  const std::vector<int32_t> ms = d.down(d_st, 4);
  CHECK(ms[2] == TPAMD_PLAN_MORE && ms[0] == 0 && ms[1] == 0 && ms[3] == 0);
  const Packed after = Download(small, {2}, D, true), was = Download(small, {2}, D, false);
  CHECK(Equal(after, was) && after.time.size() == 6 &&
        !std::memcmp(after.time.data(), before.time.data() + before.offsets[2], 6 * 8) &&
        !std::memcmp(after.qdd.data(), before.qdd.data() + before.offsets[2] * D, 6 * D * 8));
  std::vector<int32_t> seq(4);
  CHECK(tpamd_buffer_set_info(small, 4, nullptr, nullptr, nullptr, seq.data(), nullptr, nullptr, nullptr) == 0);
  CHECK(seq[2] == 0 && seq[0] == 1);
  CHECK(tpamd_buffer_set_device_bytes(small) >= small_bytes && tpamd_buffer_set_capacity(small) == 16);
  // ids: out of range in the kernel (device), at the call (host); a buffer listed twice (host)
  std::vector<int32_t> bad = {1, 7, -1}, twice = {1, 1};
  int32_t *d_bad_st = d.room<int32_t>(3);
  CHECK(tpamd_buffer_set_clear_device(small, 3, d.up(bad), d_bad_st, nullptr) == 0);
  CHECK(d.down(d_bad_st, 3) == (std::vector<int32_t>{0, TPAMD_PLAN_INVALID_ARGUMENT, TPAMD_PLAN_INVALID_ARGUMENT}));
  CHECK(tpamd_buffer_set_clear(small, 3, bad.data()) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_buffer_set_clear(small, 2, twice.data()) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_buffer_set_clear(small, 5, nullptr) == TPAMD_E_INVALID_ARGUMENT);
  std::vector<int32_t> cnt(4);
  CHECK(tpamd_buffer_set_info(small, 4, nullptr, nullptr, cnt.data(), nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(cnt[1] == 0 && cnt[0] > 0 && cnt[3] > 0);              // only the valid id of the device call was cleared
  tpamd_buffer_set *none = nullptr;
  CHECK(tpamd_buffer_set_create(e, 4, D, 0, 0.0, &none) == TPAMD_E_INVALID_ARGUMENT && none == nullptr);
  CHECK(tpamd_buffer_set_create(e, 4, D, 0, -1.0, &none) == TPAMD_E_INVALID_ARGUMENT);
  std::printf("TPAMD_PLAN_MORE leaves the buffer unchanged; id and option errors\n");
  HIP_OK(hipStreamDestroy(stream));
  tpamd_buffer_set_destroy(small);
  tpamd_buffer_set_destroy(g);
  tpamd_buffer_set_destroy(eager);
}

// the mirror-style class on top of the C-ABI
static void HostClass() {
  const int D = 3;
  TrajectoryBufferSet set(8, D);
  CHECK(set.status().ok());
  CHECK(!TrajectoryBufferSet(2, D, TrajectoryBufferOptions{0.0}).status().ok());
  auto m = *TrajectoryBuffer::Create();
  const Rows r = MakeRows(20, D, 1.0);
  SampledTrajectory s;
  s.times = r.time;
  for (int i = 0; i < 20; i++) {
    s.positions.push_back(VectorXd(&r.q[(size_t)i * D], D));
    s.velocities.push_back(VectorXd(&r.qd[(size_t)i * D], D));
    s.accelerations.push_back(VectorXd(&r.qdd[(size_t)i * D], D));
  }
  CHECK(set.InsertSegments({5}, {s})[0].ok() && m->InsertSegment(s.times, s.positions, s.velocities, s.accelerations).ok());
  const double mid = 0.5 * (r.time[4] + r.time[5]);
  CHECK(set.DiscardSegmentsBefore({5}, std::vector<double>{mid}).ok());
  m->DiscardSegmentBefore(mid);
  CHECK(set.AppendSamples({5}, {r.time[19] + 1e-3}, {s.positions[0]}, {s.velocities[0]}, {s.accelerations[0]})[0].ok());
  CHECK(m->AppendSample(r.time[19] + 1e-3, s.positions[0], s.velocities[0], s.accelerations[0]).ok());
  CHECK(set.AppendSamples({5}, {0.0}, {s.positions[0]}, {s.velocities[0]}, {s.accelerations[0]})[0].code() == StatusCode::kInvalidArgument);
  CHECK(set.AddOffsetsToTimestamps({5}, std::vector<double>{0.5}).ok());
  m->AddOffsetToTimestamps(0.5);
  std::vector<SampledTrajectory> got;
  CHECK(set.GetSamples({5, 0}, &got).ok() && got.size() == 2 && got[1].times.empty());
  CHECK(got[0].times.size() == m->GetNumSamples());
  for (size_t i = 0; i < got[0].times.size() && i < m->GetNumSamples(); i++)
    CHECK(got[0].times[i] == m->GetTimes()[i] && !std::memcmp(got[0].positions[i].data(), m->GetPositions()[i].data(), D * 8));
  std::vector<TrajectoryBufferInfo> info;
  CHECK(set.GetInfo({5}, {}, &info).ok() && info[0].num_samples == m->GetNumSamples() &&
        info[0].start_time == m->GetStartTime() && info[0].end_time == m->GetEndTime());
  CHECK(set.Clear({5}).ok() && set.GetInfo({5}, {}, &info).ok() && info[0].num_samples == 0);
  CHECK(!set.Clear({8}).ok());
  std::printf("TrajectoryBufferSet: ok\n");
}

int main(int argc, char **argv) {
  tpamd_engine *e = nullptr;
  if (tpamd_engine_create(0, &e) != 0) {
    std::printf("no engine\n");
    return 1;
  }
  Fuzz(e, 256, 7, 90);
  Fuzz(e, 260, 14, 40);
  Fuzz(e, 64, 1, 40);
  Paths paths;
  if (argc > 1 && ReadPaths(argv[1], &paths)) WithPlanners(e, paths);
  else { std::printf("FAIL: no planner paths given\n"); g_fail++; }
  GraphAndCapacity(e);
  HostClass();
  tpamd_engine_destroy(e);
  if (g_fail) {
    std::printf("%d FAILURES\n", g_fail);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}
