// tpamd_state.h -- the planner state record (include/tpamd.h tpamd_planner_set_export_state_* /
// import_state_* / copy_planners): everything of one planner of a planner set that a later call on
// the set can read, as one versioned, canonical, position-independent run of bytes. Plain C++ for
// the host and the device; the kernels that write and read records on the device are in
// tpamd_state.hip.
//
// A record is a StateRecordHeader (192 bytes) followed by kStateSections sections of 64-bit words,
// each starting on a 16-byte boundary, in the order of the kSec* enum:
//   knots [np + 3], control points [np][D]                  joint sets with a path (np >= 3)
//   vmax [D], amax [D], initial velocity [D]                a planner with a path
//   history time, s, sd, sdd [hc], q, qd, qdd [hc][D]       hc = history_count
//   w_time [N]                                              profile_ of the last window, once planned
//   trajectory time, s, sd, sdd [tc], q, qd, qdd [tc][D]    tc = trajectory_count, from t_first on
//   IK positions [live][D], Jacobians [live][6][D]          Cartesian sets: live = table_rows - first_row
// Where a section starts follows from the counts in the header alone (state_record_layout), so the
// record stores no offsets. Canonical: a section with an odd word count is followed by one zero
// word, nothing beyond the live counts is stored, a planner without a path stores no path, limits
// or table, a planner that has not planned stores no window. Payloads travel as 64-bit integers:
// the NaN marks keep their bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TPAMD_ST_HD __host__ __device__ __forceinline__
#else
#define TPAMD_ST_HD inline
#endif

namespace tpamd {

constexpr uint32_t kStateMagic = 0x54535054u;      // "TPST", little endian
constexpr uint32_t kStateVersion = 1;
constexpr int kStateMaxSamples = 1 << 28;          // history, trajectory and table rows of one planner
constexpr int kStateMaxPoints = 1 << 24;           // control points of one path

enum { kStateJoint = 0, kStateCartesian = 1 };

enum {
  kSecKnots = 0, kSecCp, kSecVmax, kSecAmax, kSecIv,
  kSecHTime, kSecHS, kSecHSd, kSecHSdd, kSecHQ, kSecHQd, kSecHQdd,
  kSecWTime,
  kSecTTime, kSecTS, kSecTSd, kSecTSdd, kSecTQ, kSecTQd, kSecTQdd,
  kSecTableQ, kSecTableJ,
  kStateSections
};

// what a record and the set that takes it must agree on
struct SetShape {
  int32_t kind, num_dofs, num_samples, sampling_method;
  int64_t time_step_ns;
  uint64_t constraint_safety_bits, max_initial_velocity_error_bits;
};

struct StateRecordHeader {
  uint32_t magic, version;
  uint64_t bytes;                       // the whole record, a multiple of 16
  SetShape shape;
  // counts
  int32_t num_points, history_count, trajectory_count, table_rows, first_row, has_path, path_state;
  // planner scalars
  int32_t initial_plan, planned_to_end, target_reached, w_lei, reserved;
  uint64_t path_horizon, path_start, path_start_velocity, path_time_start;   // doubles, by bit pattern
  int64_t start_time_ns, end_time_ns, final_decel_start_ns;
  uint64_t delta, path_end, vtrans, vrot;                                    // doubles, by bit pattern
};
static_assert(sizeof(SetShape) == 40, "record layout");
static_assert(sizeof(StateRecordHeader) == 192 && sizeof(StateRecordHeader) % 16 == 0, "record layout");

struct StateLayout {
  uint64_t off[kStateSections];         // bytes from the start of the record
  uint64_t words[kStateSections];       // 64-bit words of payload (the pad word not counted)
  uint64_t bytes;
};

// reasons state_record_validate gives (0: the record is good)
enum {
  kStateOk = 0, kStateTruncated, kStateBadMagic, kStateBadVersion, kStateBadCount, kStateBadSection,
  kStateShapeMismatch
};

// The sections of a record with these counts. Every count has passed the bounds of
// state_record_validate (or comes from a set, whose capacities obey them): nothing overflows 64 bits.
TPAMD_ST_HD StateLayout state_record_layout(const StateRecordHeader &h) {
  StateLayout L;
  const uint64_t D = (uint64_t)h.shape.num_dofs, N = (uint64_t)h.shape.num_samples;
  const uint64_t np = (uint64_t)h.num_points, hc = (uint64_t)h.history_count, tc = (uint64_t)h.trajectory_count;
  const uint64_t live = (uint64_t)(h.table_rows - h.first_row);
  const uint64_t lim = h.has_path ? D : 0;
  for (int s = 0; s < kStateSections; s++) L.words[s] = 0;
  L.words[kSecKnots] = np ? np + 3 : 0;
  L.words[kSecCp] = np * D;
  L.words[kSecVmax] = L.words[kSecAmax] = L.words[kSecIv] = lim;
  L.words[kSecHTime] = L.words[kSecHS] = L.words[kSecHSd] = L.words[kSecHSdd] = hc;
  L.words[kSecHQ] = L.words[kSecHQd] = L.words[kSecHQdd] = hc * D;
  L.words[kSecWTime] = h.initial_plan ? N : 0;
  L.words[kSecTTime] = L.words[kSecTS] = L.words[kSecTSd] = L.words[kSecTSdd] = tc;
  L.words[kSecTQ] = L.words[kSecTQd] = L.words[kSecTQdd] = tc * D;
  L.words[kSecTableQ] = live * D;
  L.words[kSecTableJ] = live * 6 * D;
  uint64_t at = sizeof(StateRecordHeader);
  for (int s = 0; s < kStateSections; s++) {
    L.off[s] = at;
    at += ((L.words[s] + 1) & ~(uint64_t)1) * 8;
  }
  L.bytes = at;
  return L;
}

TPAMD_ST_HD bool state_shape_equal(const SetShape &a, const SetShape &b) {
  return a.kind == b.kind && a.num_dofs == b.num_dofs && a.num_samples == b.num_samples &&
         a.sampling_method == b.sampling_method && a.time_step_ns == b.time_step_ns &&
         a.constraint_safety_bits == b.constraint_safety_bits &&
         a.max_initial_velocity_error_bits == b.max_initial_velocity_error_bits;
}

// The header of a record at any alignment; the caller has checked len >= sizeof(StateRecordHeader).
TPAMD_ST_HD StateRecordHeader state_record_header(const void *record) {
  StateRecordHeader h;
  const unsigned char *src = (const unsigned char *)record;
  unsigned char *dst = (unsigned char *)&h;
  for (size_t i = 0; i < sizeof(StateRecordHeader); i++) dst[i] = src[i];
  return h;
}

// Is `record` (len bytes are readable) a well-formed record for a set of this shape? Reads the
// header only, and that only once len covers it; every later read of the record goes through sizes
// that this function has bounded by len. Returns kStateOk or the first reason that applies.
TPAMD_ST_HD int state_record_validate(const void *record, size_t len, const SetShape &shape) {
  if (!record || len < sizeof(StateRecordHeader)) return kStateTruncated;
  const StateRecordHeader h = state_record_header(record);
  if (h.magic != kStateMagic) return kStateBadMagic;
  if (h.version != kStateVersion) return kStateBadVersion;
  const SetShape &r = h.shape;
  if ((r.kind != kStateJoint && r.kind != kStateCartesian) || r.num_dofs < 1 || r.num_dofs > 16 || r.num_samples < 3 ||
      r.num_samples > 8192 || (r.sampling_method != 0 && r.sampling_method != 1) || r.time_step_ns <= 0)
    return kStateBadCount;
  const bool flags_ok = (h.has_path == 0 || h.has_path == 1) && (h.initial_plan == 0 || h.initial_plan == 1) &&
                        (h.planned_to_end == 0 || h.planned_to_end == 1) &&
                        (h.target_reached == 0 || h.target_reached == 1) && h.path_state >= 0 && h.path_state <= 3 &&     // none, new, modified, sampled
                        h.reserved == 0;
  if (!flags_ok) return kStateBadCount;
  if (h.num_points < 0 || h.num_points > kStateMaxPoints || h.history_count < 0 || h.history_count > kStateMaxSamples ||
      h.trajectory_count < 0 || h.trajectory_count > kStateMaxSamples || h.table_rows < 0 ||
      h.table_rows > kStateMaxSamples || h.first_row < 0 || h.first_row > h.table_rows || h.w_lei < 0 ||
      h.w_lei >= r.num_samples)
    return kStateBadCount;
  // what the canonical form rules out
  if (r.kind == kStateJoint && (h.table_rows != 0 || (h.has_path && h.num_points < 3))) return kStateBadCount;
  if (r.kind == kStateCartesian && h.num_points != 0) return kStateBadCount;
  if (!h.has_path && (h.table_rows != 0 || h.num_points != 0)) return kStateBadCount;
  if (!h.initial_plan && h.w_lei != 0) return kStateBadCount;
  const StateLayout L = state_record_layout(h);
  if (h.bytes != L.bytes) return kStateBadSection;
  if (h.bytes > (uint64_t)len) return kStateTruncated;
  if (!state_shape_equal(r, shape)) return kStateShapeMismatch;
  return kStateOk;
}

// ---- one planner's state as pointers: a host planner's own arrays (the host encoder and decoder
// below) or the slots of a planner set (tpamd_state.hip). sec[s] points at the first word of
// section s; the sections that the counts leave empty may be null.
struct StatePlannerView {
  StateRecordHeader head;               // magic, version and bytes are filled in by the encoder
  const uint64_t *sec[kStateSections];
};

// Encodes `v` into out (capacity bytes). Returns the record's byte count; nothing is written when
// it does not fit.
inline uint64_t state_record_encode(const StatePlannerView &v, void *out, size_t capacity) {
  StateRecordHeader h = v.head;
  h.magic = kStateMagic;
  h.version = kStateVersion;
  h.reserved = 0;
  const StateLayout L = state_record_layout(h);
  h.bytes = L.bytes;
  if (!out || L.bytes > (uint64_t)capacity) return L.bytes;
  unsigned char *dst = (unsigned char *)out;
  const unsigned char *hs = (const unsigned char *)&h;
  for (size_t i = 0; i < sizeof h; i++) dst[i] = hs[i];
  for (int s = 0; s < kStateSections; s++) {
    const unsigned char *src = (const unsigned char *)v.sec[s];
    unsigned char *d = dst + L.off[s];
    const uint64_t n = L.words[s] * 8;
    for (uint64_t i = 0; i < n; i++) d[i] = src[i];
    if (L.words[s] & 1)
      for (int i = 0; i < 8; i++) d[n + i] = 0;
  }
  return L.bytes;
}

// The view of a record that state_record_validate has accepted: sec[s] points into the record.
// The record must be 8-byte aligned for the pointers to be read as words.
inline StatePlannerView state_record_decode(const void *record) {
  StatePlannerView v;
  v.head = state_record_header(record);
  const StateLayout L = state_record_layout(v.head);
  for (int s = 0; s < kStateSections; s++)
    v.sec[s] = L.words[s] ? (const uint64_t *)((const unsigned char *)record + L.off[s]) : nullptr;
  return v;
}

#if defined(__HIPCC__)
// ---- records on the device (tpamd_state.hip). Two launches per call for all listed planners: a
// layout kernel, one thread per planner (export: header, sections and status; import:
// state_record_validate, the capacity gate and the scalars), and a copy kernel over
// (planner, section chunk).

// the per-planner statuses (TPAMD_PLAN_* of include/tpamd.h)
enum { kStPlanOk = 0, kStPlanFailedPrecondition = 1, kStPlanInvalidArgument = 3, kStPlanResourceExhausted = 8 };

// tpamd_planner_state_info
struct StateInfoDev {
  long long bytes;
  int num_points, history_count, trajectory_count, table_rows, first_row, has_path, path_state, initial_plan,
      planned_to_end, target_reached, trajectory_first, status;
};
// tpamd_planner_summary
struct StateSummaryDev {
  long long end_time_ns, final_decel_start_ns, start_time_ns;
  int num_samples, target_reached, planned_to_end, windows, path_state, history_count, status, pad;
};
// tpamd_planner_check
struct StateCheckDev {
  int32_t windows, violations, last_window_violations, worst_window, worst_sample, worst_row, first_window, first_sample;
  double worst_excess, worst_parameter;
};
static_assert(sizeof(StateInfoDev) == 56 && sizeof(StateSummaryDev) == 56 && sizeof(StateCheckDev) == 48, "C-ABI layouts");

// what the layout kernel leaves for the copy kernel, per listed planner. A unit is 16 bytes of the
// record behind its header (two words, or a section's last word and its pad): the sections are
// packed back to back, so unit u lies at byte 192 + 16 u and belongs to the section s with
// ustart[s] <= u < ustart[s + 1].
struct StateItem {
  int b, go, t_first, pad;
  uint64_t off[kStateSections], words[kStateSections];
  uint64_t ustart[kStateSections + 2];  // [kStateSections]: all units; the last entry pads to 16 bytes
};

// the arrays of a planner set
struct StateSetView {
  int B, D, N, K, pcap, cap, tcap, table_cap;
  SetShape shape;
  double *knots, *cp, *vmax, *amax, *iv, *delta, *path_end, *vtrans, *vrot;
  int *np, *path_state, *has_path, *count, *initial_plan, *planned_to_end, *target_reached;
  double *path_horizon, *path_start, *path_start_velocity, *path_time_start;
  long long *start_time_ns, *end_time_ns, *final_decel_start_ns;
  double *w_time;
  int *w_lei, *t_first, *t_count;
  double *h[7], *t[7];                  // time, s, sd, sdd, q, qd, qdd
  double *tq, *tJ;                      // Cartesian sets (else null)
  int *rows, *first_row;
  const int *suspended;                 // planners that wait for IK rows; null: nobody can
  StateCheckDev *check;                 // the records of set_checking; null: checking is off
};

// one call; every pointer is device memory
struct StateCall {
  int count;
  const int *ids;                       // [count] or null: planners 0 .. count-1
  unsigned char *blob;                  // 16-byte aligned; null (export only): sizes and info alone
  const long long *offsets;             // [count + 1] bytes, multiples of 16
  int *status;                          // [count] or null
  StateSummaryDev *summary;             // [count] or null (import)
  StateInfoDev *info;                   // [count] or null (export)
  StateItem *items;                     // [count] scratch
};

// copy_blocks: workgroups per listed planner of the copy kernel (the caller sizes it from the
// set's capacities; each workgroup strides over the sections)
void launch_state_export(const StateSetView &v, const StateCall &c, int copy_blocks, hipStream_t st);
void launch_state_import(const StateSetView &v, const StateCall &c, int copy_blocks, hipStream_t st);
#endif

}  // namespace tpamd
