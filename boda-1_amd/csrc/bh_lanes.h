// bh_lanes.h -- hazard tracker of the capture-time lane scheduler (bh_runtime.hip).
//
// Host only, no HIP types: the scheduler's decisions are plain arithmetic on byte ranges and are
// tested by a stand-alone program (tests/test_lanes_cpu.py).
//
// While a step is captured, independent narrow ops are spread over a few streams ("lanes"; lane 0 is
// the context's own stream). The tracker records the ops outstanding since the last join of all lanes
// and answers, for a new op, which lane to take and which other lanes it has to wait for:
//  * a conflict is RAW, WAR or WAW on any byte overlap of half-open ranges [lo, hi); ranges that only
//    touch do not conflict and an empty range conflicts with nothing;
//  * the op takes the lane of its most recent conflicting predecessor (stream order then carries that
//    dependency for free), otherwise the lane with the least estimated outstanding time. Opening a
//    lane that holds no work since the last join costs a fork now and a join later, both cross-stream
//    dependencies: an idle lane is opened only once every open lane holds at least fork_us of
//    estimated work (a short run of ops between two joins stays one chain on lane 0);
//  * a conflict on another lane becomes "wait for that lane's current tail": conservative and simple.
//    A lane that already waited for a tail at or past the predecessor does not wait again;
//  * the list is bounded: at the cap the tracker asks for a join of all lanes and starts empty.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace bh_lanes {

constexpr int MAX_LANES = 4;
constexpr int MAX_RANGES = 8;  // per op and direction
// no op occupies its lane for less than a dependent launch boundary (1.45-1.9 us on the MI355X)
constexpr double MIN_OP_US = 2.0;

struct range {
  uint64_t lo = 0, hi = 0;  // half-open [lo, hi)
};
inline bool overlap(const range &a, const range &b) {
  return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi;
}

struct access {
  range r[MAX_RANGES], w[MAX_RANGES];
  int nr = 0, nw = 0;
  bool overflow = false;  // more ranges than fit: the op conflicts with everything
  void read(uint64_t base, uint64_t bytes) { add(r, nr, base, bytes); }
  void write(uint64_t base, uint64_t bytes) { add(w, nw, base, bytes); }

 private:
  void add(range *v, int &n, uint64_t base, uint64_t bytes) {
    if (!bytes) return;
    if (n == MAX_RANGES) {
      overflow = true;
      return;
    }
    v[n].lo = base;
    v[n].hi = base + bytes;
    ++n;
  }
};
inline bool conflict(const access &a, const access &b) {
  if (a.overflow || b.overflow) return true;
  for (int i = 0; i < a.nw; ++i) {
    for (int j = 0; j < b.nw; ++j)
      if (overlap(a.w[i], b.w[j])) return true;  // WAW
    for (int j = 0; j < b.nr; ++j)
      if (overlap(a.w[i], b.r[j])) return true;  // a writes what b reads
  }
  for (int i = 0; i < a.nr; ++i)
    for (int j = 0; j < b.nw; ++j)
      if (overlap(a.r[i], b.w[j])) return true;  // a reads what b writes
  return false;
}

struct placement {
  int lane = 0;
  uint32_t wait_mask = 0;   // other lanes whose current tail the op waits for
  bool join_first = false;  // the list was full: join every lane, then place (nothing to wait for)
};

class tracker {
 public:
  explicit tracker(int lanes = 1, size_t cap = 256) { reset(lanes, cap); }
  void reset(int lanes, size_t cap = 256) {
    lanes_ = lanes < 1 ? 1 : (lanes > MAX_LANES ? MAX_LANES : lanes);
    cap_ = cap < 1 ? 1 : cap;
    join();
  }
  int lanes() const { return lanes_; }
  void set_fork_us(double us) { fork_us_ = us > 0 ? us : 0; }
  size_t outstanding() const { return ops_.size(); }
  // every lane was joined into lane 0: nothing is outstanding any more
  void join() {
    ops_.clear();
    seq_ = 0;
    for (int k = 0; k < MAX_LANES; ++k) {
      load_[k] = 0;
      tail_[k] = 0;
      open_[k] = k == 0;
      for (int j = 0; j < MAX_LANES; ++j) synced_[k][j] = 0;
    }
  }
  // Place an op. force_lane >= 0 pins it (an op that needs the context's own scratch runs on lane 0);
  // its conflicts on other lanes still become waits.
  placement place(const access &a, double est_us, int force_lane = -1) {
    placement p;
    if (ops_.size() >= cap_) {
      p.join_first = true;
      join();
    }
    uint32_t conf = 0;     // lanes holding a conflicting op
    uint64_t need[MAX_LANES] = {0, 0, 0, 0};  // latest conflicting op per lane
    int recent = -1;
    uint64_t recent_seq = 0;
    for (const rec &o : ops_)
      if (conflict(a, o.a)) {
        conf |= 1u << o.lane;
        if (o.seq > need[o.lane]) need[o.lane] = o.seq;
        if (o.seq > recent_seq) {
          recent_seq = o.seq;
          recent = o.lane;
        }
      }
    if (force_lane >= 0 && force_lane < lanes_) p.lane = force_lane;
    else if (recent >= 0) p.lane = recent;
    else {
      p.lane = 0;  // the least loaded open lane ...
      for (int k = 1; k < lanes_; ++k)
        if (open_[k] && load_[k] < load_[p.lane]) p.lane = k;
      if (load_[p.lane] > 0 && load_[p.lane] >= fork_us_)  // ... unless it holds enough to open another
        for (int k = 1; k < lanes_; ++k)
          if (!open_[k]) {
            p.lane = k;
            break;
          }
    }
    for (int j = 0; j < lanes_; ++j)
      if (j != p.lane && (conf >> j & 1) && need[j] > synced_[p.lane][j]) {
        p.wait_mask |= 1u << j;
        synced_[p.lane][j] = tail_[j];
      }
    rec o;
    o.a = a;
    o.lane = p.lane;
    o.seq = ++seq_;
    ops_.push_back(o);
    tail_[p.lane] = o.seq;
    open_[p.lane] = true;
    load_[p.lane] += est_us > MIN_OP_US ? est_us : MIN_OP_US;
    return p;
  }

 private:
  struct rec {
    access a;
    int lane = 0;
    uint64_t seq = 0;
  };
  std::vector<rec> ops_;
  int lanes_ = 1;
  size_t cap_ = 256;
  uint64_t seq_ = 0;
  double fork_us_ = 0;
  bool open_[MAX_LANES];  // holds work since the last join (lane 0: always)
  double load_[MAX_LANES];
  uint64_t tail_[MAX_LANES];               // seq of the last op placed on the lane
  uint64_t synced_[MAX_LANES][MAX_LANES];  // [k][j]: lane k runs behind lane j's ops up to this seq
};

}  // namespace bh_lanes
