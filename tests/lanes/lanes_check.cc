// Stand-alone check of the capture-lane hazard tracker (boda-1_amd/csrc/bh_lanes.h), built with
// AddressSanitizer + UBSan by tests/test_lanes_cpu.py. Prints "case <name> ok" per case; any failed
// expectation prints the line and makes the exit status 1.
#include <stdio.h>
#include <string.h>
#include "bh_lanes.h"

using namespace bh_lanes;

static int g_fail = 0;
#define EXPECT(x)                                              \
  do {                                                         \
    if (!(x)) {                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      g_fail = 1;                                              \
    }                                                          \
  } while (0)

// an op reading [r, r + rn) and writing [w, w + wn)
static access op(uint64_t r, uint64_t rn, uint64_t w, uint64_t wn) {
  access a;
  a.read(r, rn);
  a.write(w, wn);
  return a;
}

static void disjoint() {
  tracker t(4);
  bool seen[4] = {false, false, false, false};
  for (int i = 0; i < 4; ++i) {
    placement p = t.place(op(1000 * i, 100, 1000 * i + 500, 100), 3.0);
    EXPECT(p.wait_mask == 0 && !p.join_first);
    EXPECT(p.lane >= 0 && p.lane < 4 && !seen[p.lane]);
    seen[p.lane] = true;
  }
  // a fifth independent op takes the least loaded lane: lane 2 after an uneven load
  tracker u(3);
  EXPECT(u.place(op(0, 10, 100, 10), 5.0).lane == 0);
  EXPECT(u.place(op(200, 10, 300, 10), 4.0).lane == 1);
  EXPECT(u.place(op(400, 10, 500, 10), 1.0).lane == 2);
  placement p = u.place(op(600, 10, 700, 10), 1.0);
  EXPECT(p.lane == 2 && p.wait_mask == 0);
  printf("case disjoint ok\n");
}

// one byte of overlap between a predecessor on lane 0 and an op pinned to lane 1 is one edge
static void one_byte(const char *name, const access &first, const access &second) {
  tracker t(2);
  EXPECT(t.place(first, 1.0).lane == 0);
  placement p = t.place(second, 1.0, 1);
  EXPECT(p.lane == 1 && p.wait_mask == 1u);
  // unpinned, the same op follows its predecessor's lane and waits for nothing
  tracker u(2);
  EXPECT(u.place(first, 1.0).lane == 0);
  p = u.place(second, 1.0);
  EXPECT(p.lane == 0 && p.wait_mask == 0);
  printf("case %s ok\n", name);
}

static void touching_and_empty() {
  tracker t(2);
  EXPECT(t.place(op(0, 100, 100, 100), 1.0).lane == 0);
  // reads end where the predecessor's writes begin, writes begin where they end
  placement p = t.place(op(0, 100, 200, 100), 1.0);
  EXPECT(p.lane == 1 && p.wait_mask == 0);
  printf("case touching ok\n");
  tracker u(2);
  EXPECT(u.place(op(0, 0, 100, 100), 1.0).lane == 0);
  // an empty range inside the predecessor's output conflicts with nothing
  p = u.place(op(150, 0, 150, 0), 1.0);
  EXPECT(p.lane == 1 && p.wait_mask == 0);
  access none;
  EXPECT(!conflict(none, none) && !conflict(none, op(0, 10, 0, 10)));
  range e;
  e.lo = 5;
  e.hi = 5;
  range f;
  f.lo = 0;
  f.hi = 10;
  EXPECT(!overlap(e, f) && !overlap(f, e) && overlap(f, f));
  printf("case empty ok\n");
}

static void follows_predecessor() {
  tracker t(4);
  t.place(op(0, 10, 1000, 10), 1.0);              // lane 0
  t.place(op(20, 10, 2000, 10), 1.0);             // lane 1
  placement a = t.place(op(40, 10, 3000, 10), 1.0);  // lane 2
  EXPECT(a.lane == 2);
  placement p = t.place(op(3000, 10, 4000, 10), 1.0);  // reads lane 2's output
  EXPECT(p.lane == 2 && p.wait_mask == 0);
  printf("case follows ok\n");
}

static void two_predecessors() {
  tracker t(4);
  t.place(op(0, 10, 1000, 10), 1.0);  // lane 0 writes X
  t.place(op(20, 10, 2000, 10), 1.0); // lane 1 writes Y
  t.place(op(40, 10, 3000, 10), 1.0); // lane 2 writes Z
  access a;
  a.read(1000, 10);
  a.read(2000, 10);
  a.read(3000, 10);
  a.write(5000, 10);
  placement p = t.place(a, 1.0);
  EXPECT(p.lane == 2);             // the most recent conflicting predecessor's lane
  EXPECT(p.wait_mask == 0x3u);     // one wait per other lane
  // the lane now runs behind both tails: reading X again costs no second wait
  p = t.place(op(1000, 10, 6000, 10), 1.0, 2);
  EXPECT(p.lane == 2 && p.wait_mask == 0);
  // but new work on lane 0 that it conflicts with is waited for
  t.place(op(1000, 10, 7000, 10), 1.0, 0);
  p = t.place(op(7000, 10, 8000, 10), 1.0, 2);
  EXPECT(p.lane == 2 && p.wait_mask == 1u);
  printf("case two_lanes ok\n");
}

static void join_clears() {
  tracker t(2);
  t.place(op(0, 10, 100, 10), 9.0);
  EXPECT(t.outstanding() == 1);
  t.join();
  EXPECT(t.outstanding() == 0);
  // the same bytes again: no predecessor left, lane 0 (all lanes idle), no wait
  placement p = t.place(op(100, 10, 0, 10), 1.0);
  EXPECT(p.lane == 0 && p.wait_mask == 0 && !p.join_first);
  p = t.place(op(0, 10, 100, 10), 1.0, 1);  // against the new op it is an edge again
  EXPECT(p.lane == 1 && p.wait_mask == 1u);
  printf("case join ok\n");
}

static void cap_joins() {
  tracker t(2, 3);
  for (int i = 0; i < 3; ++i) EXPECT(!t.place(op(0, 10, 100 + 10 * i, 10), 1.0).join_first);
  placement p = t.place(op(100, 10, 0, 10), 1.0);  // conflicts with all three, but they are joined first
  EXPECT(p.join_first && p.wait_mask == 0 && p.lane == 0);
  EXPECT(t.outstanding() == 1);
  printf("case cap ok\n");
}

static void one_lane_chain() {
  tracker t(1);
  for (int i = 0; i < 5; ++i) {
    placement p = t.place(op(1000 * i, 10, 1000 * i + 500, 10), 1.0);
    EXPECT(p.lane == 0 && p.wait_mask == 0);
  }
  tracker clamp(9);
  EXPECT(clamp.lanes() == MAX_LANES);
  tracker low(0);
  EXPECT(low.lanes() == 1);
  printf("case one_lane ok\n");
}

static void scratch_serialises() {
  // two split-K ops on lane 0 share the context's workspace: named as a written range it keeps the
  // second behind the first whatever lane asks
  tracker t(3);
  access a = op(0, 10, 100, 10), b = op(200, 10, 300, 10);
  a.write(9000, 64);
  b.write(9000, 64);
  EXPECT(t.place(a, 1.0, 0).lane == 0);
  placement p = t.place(b, 1.0);
  EXPECT(p.lane == 0 && p.wait_mask == 0);
  p = t.place(b, 1.0, 2);
  EXPECT(p.lane == 2 && p.wait_mask == 1u);
  // more ranges than an op can name: it conflicts with everything
  access big;
  for (int i = 0; i < MAX_RANGES + 1; ++i) big.read(100000 + 100 * i, 10);
  EXPECT(big.overflow);
  p = t.place(big, 1.0, 1);
  EXPECT(p.lane == 1 && p.wait_mask == 0x5u);
  printf("case scratch ok\n");
}

static void fork_threshold() {
  // an idle lane is opened only once every open lane holds fork_us of estimated work
  tracker t(3);
  t.set_fork_us(10.0);
  for (int i = 0; i < 3; ++i) EXPECT(t.place(op(1000 * i, 10, 1000 * i + 500, 10), 3.0).lane == 0);  // 9 us
  EXPECT(t.place(op(5000, 10, 5500, 10), 3.0).lane == 0);   // 9 < 10: still lane 0 (now 12)
  EXPECT(t.place(op(6000, 10, 6500, 10), 3.0).lane == 1);   // 12 >= 10: lane 1 opens (3)
  EXPECT(t.place(op(7000, 10, 7500, 10), 20.0).lane == 1);  // least loaded open lane (23)
  EXPECT(t.place(op(8000, 10, 8500, 10), 1.0).lane == 2);   // both hold >= 10: lane 2 opens
  t.join();                                                 // every lane idle again
  EXPECT(t.place(op(9000, 10, 9500, 10), 3.0).lane == 0);
  EXPECT(t.place(op(9100, 10, 9600, 10), 3.0).lane == 0);
  printf("case fork ok\n");
}

int main() {
  disjoint();
  fork_threshold();
  one_byte("raw", op(0, 10, 100, 10), op(109, 1, 200, 10));    // reads the last byte written
  one_byte("war", op(100, 10, 300, 10), op(0, 10, 109, 1));    // writes the last byte read
  one_byte("waw", op(0, 10, 100, 10), op(50, 10, 109, 5));     // writes the last byte written
  touching_and_empty();
  follows_predecessor();
  two_predecessors();
  join_clears();
  cap_joins();
  one_lane_chain();
  scratch_serialises();
  printf(g_fail ? "lanes check FAILED\n" : "lanes check ok\n");
  return g_fail;
}
