// test_state_record.cc -- the planner state record of csrc/tpamd_state.h on the host: encode,
// validate and decode round trips, canonical padding, and state_record_validate against malformed
// records. Every record under test lives in a heap block of exactly `len` bytes, so that a build
// with -fsanitize=address,undefined (tests/test_state_record_cpu.py) reports any read past `len`.
// Prints "ALL OK" and returns 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_state.h"

using namespace tpamd;

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      failures++;                                                            \
    }                                                                        \
  } while (0)

static uint64_t splitmix(uint64_t *x) {
  uint64_t z = (*x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static SetShape make_shape(int kind, int D, int N, int method) {
  SetShape s{};
  s.kind = kind; s.num_dofs = D; s.num_samples = N; s.sampling_method = method;
  s.time_step_ns = 4000000;
  const double safety = 0.8, err = 1e-2;
  std::memcpy(&s.constraint_safety_bits, &safety, 8);
  std::memcpy(&s.max_initial_velocity_error_bits, &err, 8);
  return s;
}

// one planner with random payload words (NaN patterns among them) for the given counts
struct Planner {
  StatePlannerView view;
  std::vector<std::vector<uint64_t>> data;
};

static Planner make_planner(const SetShape &shape, int np, int hc, int tc, int rows, int first, int has, int planned,
                            uint64_t seed) {
  Planner p;
  StateRecordHeader &h = p.view.head;
  std::memset(&h, 0, sizeof h);
  h.shape = shape;
  h.num_points = np; h.history_count = hc; h.trajectory_count = tc; h.table_rows = rows; h.first_row = first;
  h.has_path = has; h.path_state = has ? 1 : 0;
  h.initial_plan = planned; h.planned_to_end = 1; h.target_reached = 0;
  h.w_lei = planned ? shape.num_samples - 1 : 0;
  h.path_horizon = splitmix(&seed); h.path_start = splitmix(&seed);
  h.path_start_velocity = 0x7FF8000000000123ull;     // a NaN with a payload: it must keep its bits
  h.path_time_start = splitmix(&seed);
  h.start_time_ns = 5; h.end_time_ns = 123456789; h.final_decel_start_ns = 1000;
  h.delta = has ? splitmix(&seed) : 0;
  const StateLayout L = state_record_layout(h);
  p.data.resize(kStateSections);
  for (int s = 0; s < kStateSections; s++) {
    p.data[s].resize(L.words[s]);
    for (auto &w : p.data[s]) w = splitmix(&seed);
    if (!p.data[s].empty()) p.data[s][0] = 0xFFF8DEADBEEF0001ull;      // another NaN pattern
    p.view.sec[s] = p.data[s].empty() ? nullptr : p.data[s].data();
  }
  return p;
}

// the record in a heap block of exactly its size
static std::unique_ptr<unsigned char[]> encode_exact(const Planner &p, uint64_t *bytes) {
  *bytes = state_record_encode(p.view, nullptr, 0);
  std::unique_ptr<unsigned char[]> rec(new unsigned char[*bytes]);
  std::memset(rec.get(), 0xAB, *bytes);              // the encoder writes every byte, pads included
  CHECK(state_record_encode(p.view, rec.get(), *bytes) == *bytes);
  return rec;
}

static int validate_copy(const unsigned char *rec, size_t len, const SetShape &shape) {
  // a block of exactly len bytes: nothing readable past len
  std::unique_ptr<unsigned char[]> tight(new unsigned char[len ? len : 1]);
  if (len) std::memcpy(tight.get(), rec, len);
  const int a = state_record_validate(len ? tight.get() : nullptr, len, shape);
  // the unaligned copy leaves one byte of slack in front, none behind
  std::unique_ptr<unsigned char[]> shifted(new unsigned char[len + 1]);
  if (len) std::memcpy(shifted.get() + 1, rec, len);
  const int b = state_record_validate(shifted.get() + 1, len, shape);
  CHECK(a == b);
  return a;
}

static void round_trip(const SetShape &shape, int np, int hc, int tc, int rows, int first, int has, int planned,
                       uint64_t seed) {
  const Planner p = make_planner(shape, np, hc, tc, rows, first, has, planned, seed);
  uint64_t bytes = 0;
  auto rec = encode_exact(p, &bytes);
  CHECK(bytes % 16 == 0);
  CHECK(validate_copy(rec.get(), bytes, shape) == kStateOk);
  const StatePlannerView back = state_record_decode(rec.get());
  CHECK(back.head.magic == kStateMagic && back.head.version == kStateVersion && back.head.bytes == bytes);
  CHECK(back.head.num_points == np && back.head.history_count == hc && back.head.trajectory_count == tc);
  CHECK(back.head.path_start_velocity == 0x7FF8000000000123ull);
  const StateLayout L = state_record_layout(back.head);
  CHECK(L.bytes == bytes);
  std::vector<char> covered(bytes, 0);
  for (size_t i = 0; i < sizeof(StateRecordHeader); i++) covered[i] = 1;
  for (int s = 0; s < kStateSections; s++) {
    CHECK(L.off[s] % 16 == 0);
    CHECK(L.words[s] == p.data[s].size());
    if (L.words[s]) CHECK(std::memcmp(back.sec[s], p.data[s].data(), L.words[s] * 8) == 0);
    for (uint64_t i = 0; i < L.words[s] * 8; i++) covered[L.off[s] + i] = 1;
  }
  for (uint64_t i = 0; i < bytes; i++)
    if (!covered[i]) CHECK(rec[i] == 0);               // every pad byte is zero
  // decode -> encode gives the same bytes
  std::unique_ptr<unsigned char[]> again(new unsigned char[bytes]);
  CHECK(state_record_encode(back, again.get(), bytes) == bytes);
  CHECK(std::memcmp(again.get(), rec.get(), bytes) == 0);
  // a capacity that is too small writes nothing
  std::vector<unsigned char> small(bytes - 16, 0x5A);
  CHECK(state_record_encode(p.view, small.data(), small.size()) == bytes);
  for (unsigned char c : small) CHECK(c == 0x5A);
}

template <typename F>
static int mutated(const unsigned char *rec, uint64_t bytes, const SetShape &shape, F change) {
  std::vector<unsigned char> m(rec, rec + bytes);
  StateRecordHeader h = state_record_header(m.data());
  change(h);
  std::memcpy(m.data(), &h, sizeof h);
  return validate_copy(m.data(), bytes, shape);
}

static void rejections() {
  const SetShape shape = make_shape(kStateJoint, 7, 33, 0);
  const Planner p = make_planner(shape, 6, 65, 40, 0, 0, 1, 1, 99);
  uint64_t bytes = 0;
  auto rec = encode_exact(p, &bytes);
  const unsigned char *r = rec.get();
  CHECK(validate_copy(r, bytes, shape) == kStateOk);
  CHECK(state_record_validate(nullptr, 0, shape) == kStateTruncated);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.magic ^= 1; }) == kStateBadMagic);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.version = 2; }) == kStateBadVersion);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.version = 0; }) == kStateBadVersion);
  // negative and oversized counts
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.history_count = -1; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.trajectory_count = -5; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.num_points = -3; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.num_points = 2; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.history_count = kStateMaxSamples + 1; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.trajectory_count = INT32_MAX; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.num_points = kStateMaxPoints + 1; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.table_rows = 4; }) == kStateBadCount);      // a joint record
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.first_row = 1; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.w_lei = 33; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.w_lei = -1; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.has_path = 2; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.path_state = 7; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.reserved = 1; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.shape.num_dofs = 0; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.shape.num_dofs = 17; }) == kStateBadCount);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.shape.num_samples = 100000; }) == kStateBadCount);
  // sections that do not agree with the stated length, or lie past the end
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.bytes += 16; }) == kStateBadSection);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.bytes -= 16; }) == kStateBadSection);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.history_count += 1; }) == kStateBadSection);
  CHECK(mutated(r, bytes, shape, [](StateRecordHeader &h) { h.bytes = ~(uint64_t)0; }) == kStateBadSection);
  {   // consistent with itself, but longer than the buffer
    std::vector<unsigned char> m(r, r + bytes);
    StateRecordHeader h = state_record_header(m.data());
    h.trajectory_count = kStateMaxSamples;
    h.bytes = state_record_layout(h).bytes;
    std::memcpy(m.data(), &h, sizeof h);
    CHECK(validate_copy(m.data(), bytes, shape) == kStateTruncated);
  }
  // truncated buffers: every length below the record's
  for (uint64_t len = 0; len < bytes; len += (len < 200 ? 1 : 97))
    CHECK(validate_copy(r, len, shape) == kStateTruncated);
  CHECK(validate_copy(r, bytes - 1, shape) == kStateTruncated);
  // well formed, but for a set of another shape
  for (int which = 0; which < 7; which++) {
    SetShape other = shape;
    if (which == 0) other.kind = kStateCartesian;
    if (which == 1) other.num_dofs = 6;
    if (which == 2) other.num_samples = 65;
    if (which == 3) other.sampling_method = 1;
    if (which == 4) other.time_step_ns = 8000000;
    if (which == 5) other.constraint_safety_bits ^= 1;
    if (which == 6) other.max_initial_velocity_error_bits ^= 1;
    CHECK(validate_copy(r, bytes, other) == kStateShapeMismatch);
  }
  // garbage of every length up to a header and a half never reads past len
  uint64_t seed = 7;
  for (size_t len = 0; len < 300; len++) {
    std::vector<unsigned char> g(len);
    for (auto &c : g) c = (unsigned char)splitmix(&seed);
    if (len >= 8) { const uint32_t m = kStateMagic, v = kStateVersion; std::memcpy(g.data(), &m, 4); std::memcpy(g.data() + 4, &v, 4); }
    CHECK(validate_copy(g.data(), len, shape) != kStateOk);
  }
}

int main() {
  for (int D : {1, 7, 16})
    for (int N : {33, 65})
      for (int method : {0, 1}) {
        const SetShape joint = make_shape(kStateJoint, D, N, method), cart = make_shape(kStateCartesian, D, N, method);
        round_trip(joint, 0, 0, 0, 0, 0, 0, 0, 1);          // no path
        round_trip(joint, 4, 0, 0, 0, 0, 1, 0, 2);          // a new, unplanned path
        round_trip(joint, 16, 64, 101, 0, 0, 1, 1, 3);      // mid-motion
        round_trip(joint, 3, 65, 1, 0, 0, 1, 1, 4);         // odd counts: pads
        round_trip(cart, 0, 33, 12, 0, 0, 0, 1, 5);         // a Cartesian planner that lost its table
        round_trip(cart, 0, 70, 55, 200, 0, 1, 1, 6);       // a whole table
        round_trip(cart, 0, 70, 55, 200, 61, 1, 1, 7);      // after a discard
      }
  rejections();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}
