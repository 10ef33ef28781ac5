// bh_common.h -- internal declarations shared by the libboda_hip.so sources.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <algorithm>
#include <dlfcn.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "boda_hip.h"
#include "bh_lanes.h"

namespace bh {
struct op_scope;
}
// Capture-time lane scheduler (bh_runtime.hip, DESIGN.md "Capture lanes"). Lane 0 is the context's lane:
// its stream is bh_ctx::stream and every eager call runs on it; lanes 1.. are the side streams of a
// capture. Each lane has split-K scratch of its own, handed out by bh::scratch alone.
struct bh_lane {
  hipStream_t stream = nullptr;
  void *ws = nullptr;  // split-K workspace of ops on this lane
  size_t ws_bytes = 0;
  void *cnt = nullptr;  // split-K arrival tickets of ops on this lane
  uint64_t cnt_n = 0;
  bool forked = false;  // holds work of the running capture that lane 0 has not joined yet
};
struct bh_sched {
  int lanes = 1;            // BH_CAPTURE_LANES (1: one chain of dependent launches)
  double narrow_us = 0;     // BH_CAPTURE_NARROW_US: ops with a roofline time below this are spread
  bool capturing = false;   // between bh_capture_begin and bh_capture_end
  bh_lane lane[bh_lanes::MAX_LANES];
  std::vector<hipEvent_t> ev;         // timing-disabled events of the forks, joins and cross-lane edges
  size_t ev_used = 0;
  bh_lanes::tracker trk;
  size_t hw_ws = 0;     // high-water marks of the scratch narrow ops asked for in eager calls
  bh::op_scope *scope = nullptr;  // the hot-path call being issued
  uint32_t used_mask = 0;
  uint32_t cur[4] = {0, 0, 0, 0};    // running capture: -, cross-lane edges, joins, ops scoped
  uint32_t stats[4] = {0, 0, 0, 0};  // last finished capture: lanes used, edges, joins, ops scoped
  std::vector<uint32_t> cur_trace, trace;  // per scoped op: lane | wait mask << 8
};

struct bh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;  // sched.lane[0].stream (bh_init)
  hipDeviceProp_t prop{};
  std::vector<hipEvent_t> events;  // pool; ids index into it
  int events_used = 0;
  int ovr_cfg[2] = {-1, -1};  // tuning override per op (0 sgemm, 1 conv); -1 = table/heuristic
  uint32_t ovr_splits[2] = {0, 0};
  int ovr_red[2] = {0, 0};
  int ovr_wt[2] = {-1, -1};  // output store policy override (-1 = the table's / heuristic's)
  std::vector<hipGraphExec_t> graphs;  // captured launch sequences
  void *stamps = nullptr;              // device timestamp slots (bh_stamp)
  hipEvent_t t_start = nullptr;        // bh_time_next_call: events for the next call's
  hipEvent_t t_stop = nullptr;         //   first / last kernel dispatch
  double stamp_hz = 100e6;
  void *wpack = nullptr;  // k-major filter bank for the ring conv kernels, grown on demand
  size_t wpack_bytes = 0;
  // backward conv (bh_bck.hip): overrides of op 2 (input gradient) / op 3 (filter gradient), and the
  // bck pack (transposed-flipped bank + its forward pack) of a call that was given none
  int bck_cfg[2] = {-1, -1};
  int bck_splits[2] = {0, 0};
  void *bckw = nullptr;
  size_t bckw_bytes = 0;
  // outgrown workspaces still referenced by captured graphs: freed with the last graph (or the context)
  // (a graph replays the pointers it was captured with)
  std::vector<void *> retired;
  bh_sched sched;
};

namespace bh {

int fail(int code, const std::string &msg);  // records thread-local message, returns code
int ok();                                    // clears nothing, returns BH_OK

// Kernel launch checks (hipGetLastError after each launch).
int check_launch(const char *what);

// Launch on the context's stream; when bh_time_next_call armed an event pair, the
// first dispatch of the call records the start event and the last one the stop
// event on the kernel's own dispatch (hipExtLaunchKernel).
int launch(bh_ctx *ctx, const void *kernel, dim3 grid, dim3 block, void **args, bool first, bool last,
           const char *what, uint32_t shmem = 0);

// ---- capture lanes. A hot-path entry (sgemm, forward conv) opens an op_scope naming the bytes it reads
// and writes and its roofline time. While the context is capturing, the scope's first launch (or scratch
// request) picks its lane; every kernel of the call then goes to that lane's stream. Launches outside a
// scope and direct uses of the context's stream join all lanes first (barrier).
struct op_scope {
  bh_ctx *c;
  bh_lanes::access acc;
  double est_us = 0;
  bool narrow = false;
  bool resolved = false;
  bool pin0 = false;  // must run on lane 0 (it uses a buffer the context holds once)
  int lane = 0;
  op_scope(bh_ctx *ctx, double flops, double bytes);
  ~op_scope() { c->sched.scope = nullptr; }
  void read(const void *p, uint64_t bytes) {
    if (p) acc.read((uint64_t)(uintptr_t)p, bytes);
  }
  void write(const void *p, uint64_t bytes) {
    if (p) acc.write((uint64_t)(uintptr_t)p, bytes);
  }
};
int lane_resolve(bh_ctx *ctx, size_t ws_need);  // pick the open scope's lane (no-op outside a capture)
int barrier(bh_ctx *ctx);                       // join every lane into the context's stream
// Split-K / stream-K scratch of a call: ws_bytes of workspace and `tickets` zeroed arrival tickets (each
// tile's last arriver resets its own); 0 = not needed, that pointer stays null. Picks the open scope's lane
// (with the workspace need: a narrow op that needs more than a side lane holds runs on lane 0) and hands out
// that lane's buffers; outside a scope, lane 0's. Lane 0 grows on demand, a side lane only in
// bh_capture_begin; nothing grows inside a capture (BH_ERR: run the op once eagerly first).
struct scratch_t {
  float *ws = nullptr;
  uint32_t *cnt = nullptr;
};
int scratch(bh_ctx *ctx, size_t ws_bytes, uint64_t tickets, scratch_t &out);
// The context's one filter-bank pack buffer, grown to `bytes`. Inside a capture the open scope writes then
// reads it, so it is ordered against every other op that repacks and runs on lane 0.
int pack_buffer(bh_ctx *ctx, size_t bytes, float *&out);

// Magic-number unsigned division for 0 <= n < 2^31, 1 <= d < 2^31:
// q = (umulhi(n, m) + n) >> s.
struct fastdiv {
  uint32_t d, m, s;
};
inline fastdiv make_fastdiv(uint32_t d) {
  fastdiv f{d, 0, 0};
  uint32_t s = 0;
  while ((1ull << s) < d) ++s;
  f.s = s;
  f.m = (uint32_t)(((1ull << 32) * ((1ull << s) - d)) / d + 1);
  return f;
}
// the magic number and shift of d into a kernel-argument pair (d == 0 is taken as 1)
inline void set_fd(uint32_t d, uint32_t &m, uint32_t &s) {
  const fastdiv f = make_fastdiv(d ? d : 1);
  m = f.m;
  s = f.s;
}

// blocks of 256 threads that cover n elements, at most cap (grid-stride kernels cover the rest)
inline uint32_t grid_for(uint64_t n, uint32_t cap = 16384) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, cap));
}
inline uint32_t num_cus(const bh_ctx *ctx) {
  return ctx->prop.multiProcessorCount > 0 ? (uint32_t)ctx->prop.multiProcessorCount : 256u;
}
// per-block device-clock marks of the instrumented library (tools/ktrace.py); nothing otherwise
template <class Args>
inline void set_trace(bh_ctx *ctx, Args &p) {
#ifdef BH_KTRACE
  p.trace = (unsigned long long *)ctx->stamps + 65536;
#else
  (void)ctx;
  (void)p;
#endif
}
// blocks of nt threads with lds bytes of dynamic LDS a CU holds at once (1 when the query fails)
inline int occupancy(const void *k, int nt, size_t lds = 0) {
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, nt, lds) != hipSuccess || occ < 1) occ = 1;
  return occ;
}
// let kernel k take lds bytes of dynamic LDS (what: the BH_ERR message when the runtime refuses)
inline int dyn_lds(const void *k, uint32_t lds, const char *what) {
  if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail(BH_ERR, what);
  return BH_OK;
}

}  // namespace bh

#define BH_HIP(x)                                                                      \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) return bh::fail(BH_ERR, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define BH_CHECK_CTX(c) \
  do { if (!(c)) return bh::fail(BH_ERR, "null bh_ctx"); } while (0)

namespace bh {
// Every C-ABI entry that allocates, creates events or launches runs with the context's
// device current (several contexts / host threads may drive several GPUs), restoring the
// caller's device on return.
struct device_scope {
  int prev = -1;
  explicit device_scope(const bh_ctx *c) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != c->device) (void)hipSetDevice(c->device);
  }
  ~device_scope() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};
// A hot-path call consumes the event pair bh_time_next_call armed, whether it launched or
// failed first: a pair left armed by a rejected call must not attach to an unrelated later
// launch.
struct call_scope : device_scope {
  bh_ctx *c;
  explicit call_scope(bh_ctx *ctx) : device_scope(ctx), c(ctx) {}
  ~call_scope() {
    c->t_start = nullptr;
    c->t_stop = nullptr;
  }
};
// Grow a per-context device buffer to at least `want` bytes (+25 % with headroom). Refuses to
// allocate while the context's stream is capturing (a capture records no allocation: run the
// op once eagerly first). The outgrown buffer is kept until the context is destroyed when a
// captured graph may still reference it, freed otherwise.
int grow_buffer(bh_ctx *ctx, void *&buf, size_t &have, size_t want, bool zero, const char *what,
                bool headroom = true);
}  // namespace bh

#define BH_ENTER(c)  \
  BH_CHECK_CTX(c);   \
  bh::device_scope bh_dev_scope_(c)
#define BH_ENTER_CALL(c) \
  BH_CHECK_CTX(c);       \
  bh::call_scope bh_call_scope_(c)

// ---- internal entry points implemented in the kernel sources ----
namespace bh {
int launch_gen_data(bh_ctx *ctx, int kind, float *dst, const uint32_t dims[4], uint32_t mode, float vi);
int launch_sgemm(bh_ctx *ctx, const float *a, const float *b, float *c, uint32_t M, uint32_t N, uint32_t K);
int tune_set_wt(bh_ctx *ctx, int op, int wt);
// One forward conv call: out = act(conv(in, filts) + biases [+ res]).
struct conv_call {
  const float *in, *filts;
  const float *packed;  // the caller's pack of filts (may be null: a route that reads a pack makes its own)
  uint32_t pk_banks;    // the Winograd banks (BH_BANK_*) packed holds behind its k-major bank
  const float *biases, *res;  // may be null; res is laid out like an OC-channel out
  float *out;                 // the first byte written: the call's channel slab in image 0
  uint32_t B, IC, H, W, OC, KY, KX, sy, sx, py, px;
  int relu;
  // channels of the tensor `out` points into (0: OC). Every conv epilogue addresses image i of the
  // output at i * out_ctot * OH * OW, so a conv can write its channel slab of a wider tensor (a
  // Concat's output) in place.
  uint32_t out_ctot;
  uint32_t OH = 0, OW = 0;  // derived by finish()
  void finish() {
    if (!out_ctot) out_ctot = OC;
    OH = (H + 2 * py - KY) / sy + 1;
    OW = (W + 2 * px - KX) / sx + 1;
  }
};
int launch_conv(bh_ctx *ctx, const conv_call &cc);  // cc finished
// packs (bhk::launch_pack_banks): the k-major bank + the Winograd banks of `banks` (BH_BANK_*)
size_t conv_filts_packed_floats(uint32_t OC, uint32_t IC, uint32_t KY, uint32_t KX, uint32_t banks);
int launch_conv_filts_pack(bh_ctx *ctx, const float *filts, float *packed, uint32_t OC, uint32_t IC, uint32_t KY,
                           uint32_t KX, uint32_t banks);
// the Winograd bank (BH_BANK_*, 0: none) the shape's route on ctx reads
uint32_t conv_route_banks(bh_ctx *ctx, const uint32_t *d);
uint32_t pool_out_sz(uint32_t in, uint32_t k, uint32_t s, uint32_t p);
int launch_pool(bh_ctx *ctx, const float *in, float *out, float *out_in_yx, uint32_t B, uint32_t C, uint32_t H,
                uint32_t W, uint32_t KY, uint32_t KX, uint32_t sy, uint32_t sx, uint32_t py, uint32_t px, int avg);
int launch_lrn(bh_ctx *ctx, const float *in, float *out, float *out_scale_base, uint32_t B, uint32_t C, uint32_t H,
               uint32_t W, uint32_t local_size, float alpha, float beta, float k);
int launch_relu(bh_ctx *ctx, float *x, uint64_t n);
int launch_dropout(bh_ctx *ctx, float *x, uint64_t n, float ratio, uint32_t seed);
// first / last: whether this is the first / last dispatch of the C-ABI call (bh_time_next_call)
int launch_softmax(bh_ctx *ctx, const float *in, float *prob, uint32_t B, uint32_t C, uint32_t H, uint32_t W,
                   bool first = true, bool last = true);
int launch_chan_copy(bh_ctx *ctx, const float *in, float *out, uint32_t B, uint32_t HW, uint32_t in_c, uint32_t ic0,
                     uint32_t out_c, uint32_t oc0, uint32_t nc);
int launch_chan_affine(bh_ctx *ctx, const float *in, float *out, const float *scale, const float *shift, uint32_t B,
                       uint32_t C, uint32_t HW, int relu);
int launch_eltwise(bh_ctx *ctx, const float *a, const float *b, float *out, uint64_t n, int op, int relu);
std::string sgemm_variant(uint32_t M, uint32_t N, uint32_t K);
std::string conv_variant(const uint32_t *d);
std::string sgemm_variant_ctx(bh_ctx *ctx, uint32_t M, uint32_t N, uint32_t K);  // with ctx's overrides
std::string conv_variant_ctx(bh_ctx *ctx, const uint32_t *d);
int tune_set(bh_ctx *ctx, int op, int cfg, int splits);
int tune_cfg_name(int op, int cfg, std::string &out);
void jit_release_all(bh_ctx *c);
// backward conv (bh_bck.hip); d = B,IC,H,W,OC,KY,KX,sy,sx,py,px of the forward op
size_t bck_filts_packed_floats(uint32_t OC, uint32_t IC, uint32_t KY, uint32_t KX);
int launch_bck_filts_pack(bh_ctx *ctx, const float *filts, float *packed, uint32_t OC, uint32_t IC, uint32_t KY,
                          uint32_t KX, bool first, bool last);
int launch_bck(bh_ctx *ctx, const float *in, const float *filts, const float *packed, const float *out_grad,
               float *in_grad, float *filts_grad, float *biases_grad, const uint32_t *d);
std::string bck_variant(bh_ctx *ctx, int op, const uint32_t *d);  // op 2 / 3; ctx may be null
int bck_tune_set(bh_ctx *ctx, int op, int cfg, int splits);
int bck_tune_cfg_name(int op, int cfg, std::string &out);
}  // namespace bh
