// bh_runtime.hip -- device context, vars, copies, events and the extern "C"
// surface of libboda_hip.so (declared in include/boda_hip.h).
//
// Mirrors the contract of Boda's nvrtc_compute_t (src/nvrtc_util.cc:174-395):
// one device per context, zero-filled var allocation (:80-84), an event pair
// around every timed call (:289-298, :367-381), durations in milliseconds
// (src/rtc_compute.H:66-71). Unlike the reference (default stream 0), each
// context owns a non-blocking stream so several contexts / host threads can
// drive several GPUs of one node independently.
#include "bh_common.h"
#include <cstdio>
#include <cstring>

namespace {
thread_local std::string g_last_error;

// Device timestamp: one lane writes the constant-rate wall clock (s_memrealtime).
// Usable inside captured graphs, where HIP event timing is not available.
__global__ void stamp_kernel(unsigned long long *t, int slot) {
  if (threadIdx.x == 0) t[slot] = wall_clock64();
}
// bounded busy-wait on the 100 MHz constant clock (every wave exits after us µs)
__global__ void spin_kernel(unsigned long long ticks) {
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
constexpr int STAMP_SLOTS = 1 << 18;
}

namespace bh {
int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}
int ok() { return BH_OK; }
int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BH_ERR, std::string("launch of ") + what + " failed: " + hipGetErrorString(e));
  return BH_OK;
}

int grow_buffer(bh_ctx *ctx, void *&buf, size_t &have, size_t want, bool zero, const char *what, bool headroom) {
  if (have >= want) return BH_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  BH_HIP(hipStreamIsCapturing(ctx->stream, &st));
  if (st != hipStreamCaptureStatusNone)
    return fail(BH_ERR, std::string(what) + ": the per-context workspace must grow (" + std::to_string(want) +
                            " bytes) while the stream is being captured; run this op once eagerly before capturing");
  if (buf) {
    bool live_graph = false;
    for (hipGraphExec_t g : ctx->graphs) live_graph |= g != nullptr;
    if (live_graph) {
      ctx->retired.push_back(buf);  // a captured graph may still replay this pointer
    } else {
      BH_HIP(hipStreamSynchronize(ctx->stream));
      BH_HIP(hipFree(buf));
    }
    buf = nullptr;
    have = 0;
  }
  const size_t sz = headroom ? want + (want >> 2) : want;
  BH_HIP(hipMalloc(&buf, sz));
  if (zero) BH_HIP(hipMemsetAsync(buf, 0, sz, ctx->stream));
  have = sz;
  return BH_OK;
}

// ---- capture lanes (DESIGN.md "Capture lanes") ----
// MI355X peaks, as boda_hip/runner.py's roofline_secs: fp32 matrix 157.3 TFLOP/s, HBM3E 8.0 TB/s
constexpr double PEAK_FP32_FLOPS = 157.3e12, PEAK_HBM_BPS = 8.0e12;
constexpr int DEFAULT_LANES = 4;
constexpr double DEFAULT_NARROW_US = 200.0;  // every conv of the benchmark sets; DESIGN.md has the sweep
constexpr double DEFAULT_FORK_US = 20.0;     // roofline time on every open lane before another is opened

op_scope::op_scope(bh_ctx *ctx, double flops, double bytes) : c(ctx) {
  est_us = std::max(flops / PEAK_FP32_FLOPS, bytes / PEAK_HBM_BPS) * 1e6;
  narrow = est_us < ctx->sched.narrow_us;
  ctx->sched.scope = this;
}

namespace {
int next_event(bh_ctx *ctx, hipEvent_t &ev) {
  bh_sched &sc = ctx->sched;
  if (sc.ev_used == sc.ev.size()) {
    hipEvent_t e;
    BH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    sc.ev.push_back(e);
  }
  ev = sc.ev[sc.ev_used++];
  return BH_OK;
}

// stream `to` runs behind everything issued to stream `from` so far
int order_after(bh_ctx *ctx, hipStream_t from, hipStream_t to) {
  hipEvent_t ev;
  if (int rc = next_event(ctx, ev)) return rc;
  BH_HIP(hipEventRecord(ev, from));
  BH_HIP(hipStreamWaitEvent(to, ev, 0));
  return BH_OK;
}

// Join every side lane that holds un-joined work into the context's stream. The lanes' flags are
// cleared first: after a failure the scheduler stays consistent (the capture itself is then invalid
// and ends in bh_capture_end's error).
int join_streams(bh_ctx *ctx) {
  bh_sched &sc = ctx->sched;
  int rc = BH_OK;
  bool any = false;
  for (int k = 1; k < sc.lanes; ++k) {
    if (!sc.lane[k].forked) continue;
    sc.lane[k].forked = false;
    any = true;
    if (rc == BH_OK) rc = order_after(ctx, sc.lane[k].stream, ctx->stream);
  }
  if (any) ++sc.cur[2];
  return rc;
}
}  // namespace

int barrier(bh_ctx *ctx) {
  bh_sched &sc = ctx->sched;
  if (!sc.capturing || sc.lanes <= 1) return BH_OK;
  sc.trk.join();
  return join_streams(ctx);
}

int lane_resolve(bh_ctx *ctx, size_t ws_need) {
  bh_sched &sc = ctx->sched;
  op_scope *s = sc.scope;
  if (!sc.capturing || !s || s->resolved) return BH_OK;
  s->resolved = true;
  ++sc.cur[3];
  bh_lanes::placement p;
  if (sc.lanes > 1) {
    if (!s->narrow) {  // a wide op has the device to itself, on the context's stream
      if (int rc = barrier(ctx)) return rc;
    } else {
      // scratch never grows inside a capture: an op that needs more than a side lane holds takes lane 0
      p = sc.trk.place(s->acc, s->est_us, (s->pin0 || ws_need > sc.lane[1].ws_bytes) ? 0 : -1);
      if (p.join_first)
        if (int rc = join_streams(ctx)) return rc;
    }
  }
  sc.used_mask |= 1u << p.lane;
  sc.cur_trace.push_back((uint32_t)p.lane | p.wait_mask << 8);
  bh_lane &l = sc.lane[p.lane];
  if (l.stream != ctx->stream && !l.forked) {  // a side lane's first use since the last join: fork
    l.forked = true;
    if (int rc = order_after(ctx, ctx->stream, l.stream)) return rc;
  }
  for (int j = 0; j < sc.lanes; ++j)
    if (p.wait_mask >> j & 1) {
      ++sc.cur[1];
      if (int rc = order_after(ctx, sc.lane[j].stream, l.stream)) return rc;
    }
  s->lane = p.lane;  // from here on the call's launches and scratch are this lane's
  return BH_OK;
}

int scratch(bh_ctx *ctx, size_t ws_bytes, uint64_t tickets, scratch_t &out) {
  bh_sched &sc = ctx->sched;
  if (int rc = lane_resolve(ctx, ws_bytes)) return rc;
  const op_scope *s = sc.scope;
  const int k = s ? s->lane : 0;
  bh_lane &l = sc.lane[k];
  if (k != 0) {
    // a side lane runs inside a capture only, where nothing grows: it holds what bh_capture_begin gave it
    if (ws_bytes > l.ws_bytes)
      return fail(BH_ERR, "split-K workspace: the per-lane workspace must grow (" + std::to_string(ws_bytes) +
                              " bytes) while the stream is being captured; run this op once eagerly before capturing");
    if (tickets > l.cnt_n)
      return fail(BH_ERR, "split-K tickets: the per-lane tickets must grow (" + std::to_string(tickets) +
                              ") while the stream is being captured; run this op once eagerly before capturing");
  } else {
    if (ws_bytes) {
      if (!sc.capturing && s && s->narrow) sc.hw_ws = std::max(sc.hw_ws, ws_bytes);
      if (int rc = grow_buffer(ctx, l.ws, l.ws_bytes, ws_bytes, false, "split-K workspace")) return rc;
    }
    if (tickets) {
      size_t have = l.cnt_n * 4;
      const int rc = grow_buffer(ctx, l.cnt, have, std::max<uint64_t>(tickets, 4096) * 4, true, "split-K tickets");
      l.cnt_n = have / 4;
      if (rc != BH_OK) return rc;
    }
  }
  out.ws = ws_bytes ? (float *)l.ws : nullptr;
  out.cnt = tickets ? (uint32_t *)l.cnt : nullptr;
  return BH_OK;
}

int pack_buffer(bh_ctx *ctx, size_t bytes, float *&out) {
  bh_sched &sc = ctx->sched;
  if (int rc = grow_buffer(ctx, ctx->wpack, ctx->wpack_bytes, bytes, false, "filter-bank pack buffer")) return rc;
  out = (float *)ctx->wpack;
  if (!sc.capturing || !sc.scope) return BH_OK;
  // one pack buffer per context: the op writes then reads it, so it conflicts with every other
  // outstanding op that repacks
  if (sc.scope->resolved) return fail(BH_ERR, "filter-bank pack buffer requested after the call's lane was picked");
  sc.scope->write(ctx->wpack, ctx->wpack_bytes);
  sc.scope->pin0 = true;  // and its other scratch is lane 0's, as its pack buffer
  return BH_OK;
}

int launch(bh_ctx *ctx, const void *kernel, dim3 grid, dim3 block, void **args, bool first, bool last,
           const char *what, uint32_t shmem) {
  hipStream_t stream = ctx->stream;
  if (ctx->sched.capturing) {
    // a scoped call's kernels go to its lane; anything else runs behind all lanes
    if (int rc = ctx->sched.scope ? lane_resolve(ctx, 0) : barrier(ctx)) return rc;
    if (ctx->sched.scope) stream = ctx->sched.lane[ctx->sched.scope->lane].stream;
  }
  hipEvent_t b = first ? ctx->t_start : nullptr, e = last ? ctx->t_stop : nullptr;
  hipError_t r = (b || e) ? hipExtLaunchKernel(kernel, grid, block, args, shmem, stream, b, e, 0)
                          : hipLaunchKernel(kernel, grid, block, args, shmem, stream);
  if (first) ctx->t_start = nullptr;
  if (last) ctx->t_stop = nullptr;
  if (r != hipSuccess) return fail(BH_ERR, std::string("launch of ") + what + " failed: " + hipGetErrorString(r));
  return check_launch(what);
}
}  // namespace bh

namespace {
// Validate the dims of a C-ABI forward conv call (tensors, eleven dims, relu, out_ctot filled in by the
// entry) and derive the rest.
int conv_check(bh::conv_call &cc) {
  if (!cc.in || !cc.filts || !cc.out) return bh::fail(BH_ERR, "null tensor");
  if (!cc.B || !cc.IC || !cc.H || !cc.W || !cc.OC || !cc.KY || !cc.KX || !cc.sy || !cc.sx)
    return bh::fail(BH_UNSUP, "conv: zero-sized dimension or stride");
  if (cc.H + 2 * cc.py < cc.KY || cc.W + 2 * cc.px < cc.KX)
    return bh::fail(BH_UNSUP, "conv: padded input smaller than kernel");
  return BH_OK;
}
// The call writes channels [ofs, ofs + OC) of a tensor of out_ctot channels that cc.out points at.
int conv_slab(bh::conv_call &cc, uint32_t out_ctot, uint32_t ofs) {
  if ((uint64_t)ofs + cc.OC > out_ctot) return bh::fail(BH_ERR, "conv: output channel slab out of range");
  cc.out_ctot = out_ctot;
  cc.finish();
  cc.out += (uint64_t)ofs * cc.OH * cc.OW;
  return BH_OK;
}
// Open the call's op scope (roofline flops / bytes as boda_hip/ops.py's ConvShape; the bytes it touches,
// for the capture lanes: a slab call covers through the end of its slab in the last image) and launch.
int conv_run(bh_ctx *c, bh::conv_call &cc) {
  cc.finish();
  const uint64_t ohw = (uint64_t)cc.OH * cc.OW, wts = (uint64_t)cc.OC * cc.IC * cc.KY * cc.KX;
  bh::op_scope s(c, 2.0 * cc.B * ohw * wts,
                 4.0 * ((double)cc.B * cc.IC * cc.H * cc.W + (double)cc.B * cc.OC * ohw + (double)wts));
  s.read(cc.in, (uint64_t)cc.B * cc.IC * cc.H * cc.W * 4);
  s.read(cc.filts, wts * 4);
  if (cc.packed)
    s.read(cc.packed, (uint64_t)bh::conv_filts_packed_floats(cc.OC, cc.IC, cc.KY, cc.KX, cc.pk_banks) * 4);
  s.read(cc.biases, (uint64_t)cc.OC * 4);
  s.read(cc.res, (uint64_t)cc.B * cc.OC * ohw * 4);
  s.write(cc.out, ((uint64_t)(cc.B - 1) * cc.out_ctot + cc.OC) * ohw * 4);
  return bh::launch_conv(c, cc);
}
}  // namespace

extern "C" {

int bh_abi_version(void) { return BH_ABI_VERSION; }

const char *bh_last_error(void) { return g_last_error.c_str(); }

int bh_device_count(int *count) {
  if (!count) return bh::fail(BH_ERR, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *count = n;
  return BH_OK;
}

int bh_init(int device, bh_ctx **out) {
  if (!out) return bh::fail(BH_ERR, "null ctx out-pointer");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return bh::fail(BH_ERR, "no HIP device available (libboda_hip has no CPU fallback)");
  if (device < 0 || device >= n) return bh::fail(BH_ERR, "device index out of range");
  bh_ctx *c = new bh_ctx();
  c->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipGetDeviceProperties(&c->prop, device);
  if (e == hipSuccess && std::strncmp(c->prop.gcnArchName, "gfx950", 6) != 0) {
    std::string arch = c->prop.gcnArchName;
    delete c;
    return bh::fail(BH_ERR, "device is " + arch + "; libboda_hip is built for gfx950 (MI355X) only");
  }
  if (e == hipSuccess) e = hipMalloc(&c->stamps, STAMP_SLOTS * sizeof(unsigned long long));
  if (e == hipSuccess) {
    int khz = 0;
    e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device);
    c->stamp_hz = khz > 0 ? khz * 1000.0 : 100e6;
  }
  // capture lanes: BH_CAPTURE_LANES streams (1: one chain, as without the scheduler), ops with a
  // roofline time under BH_CAPTURE_NARROW_US spread over them. Replaying a graph with parallel
  // branches needs four hardware queues on this runtime: with fewer configured, one lane.
  bh_sched &sc = c->sched;
  sc.lanes = bh::DEFAULT_LANES;
  sc.narrow_us = bh::DEFAULT_NARROW_US;
  if (const char *v = getenv("BH_CAPTURE_LANES")) sc.lanes = atoi(v);
  if (const char *v = getenv("BH_CAPTURE_NARROW_US")) sc.narrow_us = atof(v);
  double fork_us = bh::DEFAULT_FORK_US;
  if (const char *v = getenv("BH_CAPTURE_FORK_US")) fork_us = atof(v);
  if (const char *v = getenv("GPU_MAX_HW_QUEUES"))
    if (atoi(v) < 4) sc.lanes = 1;
  sc.lanes = std::max(1, std::min(sc.lanes, (int)bh_lanes::MAX_LANES));
  for (int k = 0; k < sc.lanes && e == hipSuccess; ++k)
    e = hipStreamCreateWithFlags(&sc.lane[k].stream, hipStreamNonBlocking);
  c->stream = sc.lane[0].stream;
  sc.trk.reset(sc.lanes);
  sc.trk.set_fork_us(fork_us);
  if (e != hipSuccess) {
    for (bh_lane &l : sc.lane)
      if (l.stream) (void)hipStreamDestroy(l.stream);
    if (c->stamps) (void)hipFree(c->stamps);
    delete c;
    return bh::fail(BH_ERR, std::string("bh_init: ") + hipGetErrorString(e));
  }
  *out = c;
  return BH_OK;
}

int bh_destroy(bh_ctx *c) {
  BH_ENTER(c);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t ev : c->events) (void)hipEventDestroy(ev);
  for (hipGraphExec_t g : c->graphs)
    if (g) (void)hipGraphExecDestroy(g);
  bh::jit_release_all(c);
  for (void *r : c->retired) (void)hipFree(r);
  if (c->wpack) (void)hipFree(c->wpack);
  if (c->bckw) (void)hipFree(c->bckw);
  if (c->stamps) (void)hipFree(c->stamps);
  for (bh_lane &l : c->sched.lane) {
    if (l.stream) (void)hipStreamSynchronize(l.stream);
    if (l.ws) (void)hipFree(l.ws);
    if (l.cnt) (void)hipFree(l.cnt);
    if (l.stream) (void)hipStreamDestroy(l.stream);
  }
  for (hipEvent_t ev : c->sched.ev) (void)hipEventDestroy(ev);
  delete c;
  return BH_OK;
}

int bh_plat_tag(bh_ctx *c, char *buf, size_t n) {
  BH_ENTER(c);
  if (!buf || !n) return bh::fail(BH_ERR, "null buffer");
  // the marketing name comes from libdrm's amdgpu.ids; where that table is missing (some
  // launch environments) HIP reports a generic "AMD Radeon Graphics": gfx950 is MI355X
  const bool named = std::strstr(c->prop.name, "MI3") != nullptr;
  std::snprintf(buf, n, "hip:%s:%s", named ? c->prop.name : "MI355X", c->prop.gcnArchName);
  return BH_OK;
}

int bh_get_stream(bh_ctx *c, void **s) {
  BH_ENTER(c);
  if (!s) return bh::fail(BH_ERR, "null out");
  if (int rc = bh::barrier(c)) return rc;  // the caller's work runs behind every capture lane
  *s = (void *)c->stream;
  return BH_OK;
}

int bh_alloc(bh_ctx *c, size_t bytes, void **p) {
  BH_ENTER(c);
  if (!p) return bh::fail(BH_ERR, "null out");
  *p = nullptr;
  void *d = nullptr;
  BH_HIP(hipMalloc(&d, bytes ? bytes : 16));
  hipError_t e = hipMemsetAsync(d, 0, bytes ? bytes : 16, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return bh::fail(BH_ERR, std::string("bh_alloc zero-fill: ") + hipGetErrorString(e));
  }
  *p = d;
  return BH_OK;
}

int bh_free(bh_ctx *c, void *p) {
  BH_ENTER(c);
  BH_HIP(hipStreamSynchronize(c->stream));
  BH_HIP(hipFree(p));
  return BH_OK;
}

int bh_memset0(bh_ctx *c, void *p, size_t bytes) {
  BH_ENTER(c);
  if (int rc = bh::barrier(c)) return rc;
  BH_HIP(hipMemsetAsync(p, 0, bytes, c->stream));
  return BH_OK;
}

int bh_h2d(bh_ctx *c, void *d, const void *h, size_t bytes) {
  BH_ENTER(c);
  // synchronous w.r.t. the host buffer (caller may free it on return)
  if (int rc = bh::barrier(c)) return rc;
  BH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  BH_HIP(hipStreamSynchronize(c->stream));
  return BH_OK;
}

int bh_d2h(bh_ctx *c, void *h, const void *d, size_t bytes) {
  BH_ENTER(c);
  if (int rc = bh::barrier(c)) return rc;
  BH_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
  BH_HIP(hipStreamSynchronize(c->stream));
  return BH_OK;
}

int bh_sync(bh_ctx *c) {
  BH_ENTER(c);
  BH_HIP(hipStreamSynchronize(c->stream));
  return BH_OK;
}

int bh_event_record(bh_ctx *c, int *id) {
  BH_ENTER(c);
  if (!id) return bh::fail(BH_ERR, "null out");
  if (c->events_used == (int)c->events.size()) {
    hipEvent_t ev;
    BH_HIP(hipEventCreate(&ev));
    c->events.push_back(ev);
  }
  if (int rc = bh::barrier(c)) return rc;
  BH_HIP(hipEventRecord(c->events[c->events_used], c->stream));
  *id = c->events_used++;
  return BH_OK;
}

int bh_time_next_call(bh_ctx *c, int *begin_id, int *end_id) {
  BH_ENTER(c);
  if (!begin_id || !end_id) return bh::fail(BH_ERR, "null out");
  for (int k = 0; k < 2; ++k)
    if (c->events_used + k >= (int)c->events.size()) {
      hipEvent_t ev;
      BH_HIP(hipEventCreate(&ev));
      c->events.push_back(ev);
    }
  *begin_id = c->events_used++;
  *end_id = c->events_used++;
  c->t_start = c->events[*begin_id];
  c->t_stop = c->events[*end_id];
  return BH_OK;
}

int bh_elapsed_ms(bh_ctx *c, int b, int e, float *ms) {
  BH_ENTER(c);
  if (!ms) return bh::fail(BH_ERR, "null out");
  if (b < 0 || e < 0 || b >= c->events_used || e >= c->events_used) return bh::fail(BH_ERR, "bad event id");
  BH_HIP(hipEventSynchronize(c->events[e]));
  BH_HIP(hipEventElapsedTime(ms, c->events[b], c->events[e]));
  return BH_OK;
}

int bh_events_reset(bh_ctx *c) {
  BH_ENTER(c);
  c->events_used = 0;
  return BH_OK;
}

int bh_gen_data(bh_ctx *c, int kind, float *dst, const uint32_t dims[4], uint32_t mode, float vi) {
  BH_ENTER_CALL(c);
  if (!dst || !dims) return bh::fail(BH_ERR, "null argument");
  return bh::launch_gen_data(c, kind, dst, dims, mode, vi);
}

int bh_sgemm_kmajor(bh_ctx *c, const float *a, const float *b, float *cc, uint32_t M, uint32_t N, uint32_t K) {
  BH_ENTER_CALL(c);
  if (!a || !b || !cc) return bh::fail(BH_ERR, "null tensor");
  if (!M || !N || !K) return bh::fail(BH_UNSUP, "sgemm: zero-sized dimension");
  bh::op_scope scope(c, 2.0 * M * N * K, 4.0 * ((double)M * K + (double)K * N + (double)M * N));
  scope.read(a, (uint64_t)K * M * 4);
  scope.read(b, (uint64_t)K * N * 4);
  scope.write(cc, (uint64_t)M * N * 4);
  return bh::launch_sgemm(c, a, b, cc, M, N, K);
}

int bh_conv2d_fwd_nchw_pk(bh_ctx *c, const float *in, const float *filts, const float *packed, const float *biases,
                          float *out, uint32_t B, uint32_t IC, uint32_t H, uint32_t W, uint32_t OC, uint32_t KY,
                          uint32_t KX, uint32_t sy, uint32_t sx, uint32_t py, uint32_t px, int relu) {
  BH_ENTER_CALL(c);
  bh::conv_call cc{in, filts, packed, BH_BANKS_ALL, biases, nullptr, out, B, IC, H, W, OC, KY, KX, sy, sx, py, px, relu, 0};
  if (int rc = conv_check(cc)) return rc;
  return conv_run(c, cc);
}

int bh_conv2d_fwd_nchw_res(bh_ctx *c, const float *in, const float *filts, const float *packed, const float *biases,
                           const float *res, float *out, uint32_t B, uint32_t IC, uint32_t H, uint32_t W, uint32_t OC,
                           uint32_t KY, uint32_t KX, uint32_t sy, uint32_t sx, uint32_t py, uint32_t px, int relu) {
  BH_ENTER_CALL(c);
  bh::conv_call cc{in, filts, packed, BH_BANKS_ALL, biases, res, out, B, IC, H, W, OC, KY, KX, sy, sx, py, px, relu, 0};
  if (int rc = conv_check(cc)) return rc;
  return conv_run(c, cc);
}

int bh_conv2d_fwd_nchw_slab(bh_ctx *c, const float *in, const float *filts, const float *packed,
                            const float *biases, float *out, uint32_t out_chans_total, uint32_t out_chan_ofs,
                            uint32_t B, uint32_t IC, uint32_t H, uint32_t W, uint32_t OC, uint32_t KY, uint32_t KX,
                            uint32_t sy, uint32_t sx, uint32_t py, uint32_t px, int relu) {
  BH_ENTER_CALL(c);
  bh::conv_call cc{in, filts, packed, BH_BANKS_ALL, biases, nullptr, out, B, IC, H, W, OC, KY, KX, sy, sx, py, px, relu, 0};
  if (int rc = conv_check(cc)) return rc;
  if (int rc = conv_slab(cc, out_chans_total, out_chan_ofs)) return rc;
  return conv_run(c, cc);
}

int bh_conv2d_fwd_nchw_pkb(bh_ctx *c, const float *in, const float *filts, const float *packed, uint32_t banks,
                           const float *biases, const float *res, float *out, uint32_t out_chans_total,
                           uint32_t out_chan_ofs, uint32_t B, uint32_t IC, uint32_t H, uint32_t W, uint32_t OC,
                           uint32_t KY, uint32_t KX, uint32_t sy, uint32_t sx, uint32_t py, uint32_t px, int relu) {
  BH_ENTER_CALL(c);
  bh::conv_call cc{in, filts, packed, banks, biases, res, out, B, IC, H, W, OC, KY, KX, sy, sx, py, px, relu, 0};
  if (int rc = conv_check(cc)) return rc;
  if (int rc = conv_slab(cc, out_chans_total ? out_chans_total : OC, out_chan_ofs)) return rc;
  if (res && cc.out_ctot != OC) return bh::fail(BH_ERR, "conv: residual and channel slab together");
  return conv_run(c, cc);
}

int bh_conv2d_fwd_nchw(bh_ctx *c, const float *in, const float *filts, const float *biases, float *out,
                       uint32_t B, uint32_t IC, uint32_t H, uint32_t W, uint32_t OC, uint32_t KY, uint32_t KX,
                       uint32_t sy, uint32_t sx, uint32_t py, uint32_t px, int relu) {
  return bh_conv2d_fwd_nchw_pk(c, in, filts, nullptr, biases, out, B, IC, H, W, OC, KY, KX, sy, sx, py, px, relu);
}

int bh_pool_out_size(uint32_t in, uint32_t k, uint32_t stride, uint32_t pad) {
  if (!k || !stride) return 0;
  return (int)bh::pool_out_sz(in, k, stride, pad);
}

int bh_pool_fwd_nchw(bh_ctx *c, const float *in, float *out, float *out_in_yx, uint32_t B, uint32_t C, uint32_t H,
                     uint32_t W, uint32_t KY, uint32_t KX, uint32_t sy, uint32_t sx, uint32_t py, uint32_t px,
                     int avg) {
  BH_ENTER_CALL(c);
  if (!in || !out) return bh::fail(BH_ERR, "null tensor");
  if (!B || !C || !H || !W || !KY || !KX || !sy || !sx) return bh::fail(BH_UNSUP, "pool: zero-sized dimension");
  if (py >= KY || px >= KX) return bh::fail(BH_UNSUP, "pool: padding must be smaller than the window");
  return bh::launch_pool(c, in, out, out_in_yx, B, C, H, W, KY, KX, sy, sx, py, px, avg ? 1 : 0);
}

int bh_lrn_fwd_nchw(bh_ctx *c, const float *in, float *out, float *out_scale_base, uint32_t B, uint32_t C, uint32_t H,
                    uint32_t W, uint32_t local_size, float alpha, float beta, float k) {
  BH_ENTER_CALL(c);
  if (!in || !out) return bh::fail(BH_ERR, "null tensor");
  if (!B || !C || !H || !W) return bh::fail(BH_UNSUP, "lrn: zero-sized dimension");
  return bh::launch_lrn(c, in, out, out_scale_base, B, C, H, W, local_size, alpha, beta, k);
}

int bh_relu_inplace(bh_ctx *c, float *x, uint64_t n) {
  BH_ENTER_CALL(c);
  if (!x) return bh::fail(BH_ERR, "null tensor");
  if (!n) return BH_OK;
  return bh::launch_relu(c, x, n);
}

int bh_dropout_inplace(bh_ctx *c, float *x, uint64_t n, float ratio, uint32_t det_drop_seed) {
  BH_ENTER_CALL(c);
  if (!x) return bh::fail(BH_ERR, "null tensor");
  if (!n) return BH_OK;
  return bh::launch_dropout(c, x, n, ratio, det_drop_seed);
}

int bh_softmax_chans(bh_ctx *c, const float *in, float *prob, uint32_t B, uint32_t C, uint32_t H, uint32_t W) {
  BH_ENTER_CALL(c);
  if (!in || !prob) return bh::fail(BH_ERR, "null tensor");
  if (!B || !C || !H || !W) return bh::fail(BH_UNSUP, "softmax: zero-sized dimension");
  return bh::launch_softmax(c, in, prob, B, C, H, W);
}

int bh_chan_copy(bh_ctx *c, const float *in, float *out, uint32_t B, uint32_t HW, uint32_t in_c, uint32_t ic0,
                 uint32_t out_c, uint32_t oc0, uint32_t nc) {
  BH_ENTER_CALL(c);
  if (!in || !out) return bh::fail(BH_ERR, "null tensor");
  return bh::launch_chan_copy(c, in, out, B, HW, in_c, ic0, out_c, oc0, nc);
}

int bh_chan_affine(bh_ctx *c, const float *in, float *out, const float *scale, const float *shift, uint32_t B,
                   uint32_t C, uint32_t HW, int relu) {
  BH_ENTER_CALL(c);
  if (!in || !out || !scale || !shift) return bh::fail(BH_ERR, "null tensor");
  return bh::launch_chan_affine(c, in, out, scale, shift, B, C, HW, relu ? 1 : 0);
}

int bh_eltwise(bh_ctx *c, const float *a, const float *b, float *out, uint64_t n, int op, int relu) {
  BH_ENTER_CALL(c);
  if (!a || !b || !out) return bh::fail(BH_ERR, "null tensor");
  if (!n) return BH_OK;
  return bh::launch_eltwise(c, a, b, out, n, op, relu ? 1 : 0);
}

size_t bh_conv_filts_packed_floats(uint32_t OC, uint32_t IC, uint32_t KY, uint32_t KX) {
  return bh::conv_filts_packed_floats(OC, IC, KY, KX, BH_BANKS_ALL);
}

int bh_conv_filts_pack(bh_ctx *c, const float *filts, float *packed, uint32_t OC, uint32_t IC, uint32_t KY,
                       uint32_t KX) {
  return bh_conv_filts_pack_banks(c, filts, packed, OC, IC, KY, KX, BH_BANKS_ALL);
}

size_t bh_conv_filts_packed_floats_banks(uint32_t OC, uint32_t IC, uint32_t KY, uint32_t KX, uint32_t banks) {
  return bh::conv_filts_packed_floats(OC, IC, KY, KX, banks);
}

int bh_conv_filts_pack_banks(bh_ctx *c, const float *filts, float *packed, uint32_t OC, uint32_t IC, uint32_t KY,
                             uint32_t KX, uint32_t banks) {
  BH_ENTER_CALL(c);
  if (!filts || !packed) return bh::fail(BH_ERR, "null tensor");
  if (!OC || !IC || !KY || !KX) return bh::fail(BH_UNSUP, "conv_filts_pack: zero-sized dimension");
  return bh::launch_conv_filts_pack(c, filts, packed, OC, IC, KY, KX, banks);
}

size_t bh_conv_bck_filts_packed_floats(uint32_t OC, uint32_t IC, uint32_t KY, uint32_t KX) {
  return bh::bck_filts_packed_floats(OC, IC, KY, KX);
}

int bh_conv_bck_filts_pack(bh_ctx *c, const float *filts, float *packed, uint32_t OC, uint32_t IC, uint32_t KY,
                           uint32_t KX) {
  BH_ENTER_CALL(c);
  if (!filts || !packed) return bh::fail(BH_ERR, "null tensor");
  if (!OC || !IC || !KY || !KX) return bh::fail(BH_ERR, "conv_bck_filts_pack: zero-sized dimension");
  return bh::launch_bck_filts_pack(c, filts, packed, OC, IC, KY, KX, true, true);
}

// dims of a backward conv are consistent: no zero extent, the padded input holds a window
static int bck_check_dims(const uint32_t *d) {
  for (int i = 0; i < 9; ++i)
    if (!d[i]) return bh::fail(BH_ERR, "bck conv: zero-sized dimension or stride");
  if ((uint64_t)d[2] + 2ull * d[9] < d[5] || (uint64_t)d[3] + 2ull * d[10] < d[6])
    return bh::fail(BH_ERR, "bck conv: padded input smaller than kernel");
  return BH_OK;
}

int bh_conv2d_bck_nchw(bh_ctx *c, const float *in, const float *filts, const float *packed, const float *out_grad,
                       float *in_grad, float *filts_grad, float *biases_grad, uint32_t B, uint32_t IC, uint32_t H,
                       uint32_t W, uint32_t OC, uint32_t KY, uint32_t KX, uint32_t sy, uint32_t sx, uint32_t py,
                       uint32_t px) {
  BH_ENTER_CALL(c);
  if (!in || !filts || !out_grad || !filts_grad || !biases_grad) return bh::fail(BH_ERR, "null tensor");
  const uint32_t d[11] = {B, IC, H, W, OC, KY, KX, sy, sx, py, px};
  if (int rc = bck_check_dims(d)) return rc;
  return bh::launch_bck(c, in, filts, packed, out_grad, in_grad, filts_grad, biases_grad, d);
}

int bh_conv2d_bck_in_nchw(bh_ctx *c, const float *filts, const float *packed, const float *out_grad, float *in_grad,
                          uint32_t B, uint32_t IC, uint32_t H, uint32_t W, uint32_t OC, uint32_t KY, uint32_t KX,
                          uint32_t sy, uint32_t sx, uint32_t py, uint32_t px) {
  BH_ENTER_CALL(c);
  if (!filts || !out_grad || !in_grad) return bh::fail(BH_ERR, "null tensor");
  const uint32_t d[11] = {B, IC, H, W, OC, KY, KX, sy, sx, py, px};
  if (int rc = bck_check_dims(d)) return rc;
  return bh::launch_bck(c, nullptr, filts, packed, out_grad, in_grad, nullptr, nullptr, d);
}

int bh_conv2d_bck_filts_nchw(bh_ctx *c, const float *in, const float *out_grad, float *filts_grad, uint32_t B,
                             uint32_t IC, uint32_t H, uint32_t W, uint32_t OC, uint32_t KY, uint32_t KX, uint32_t sy,
                             uint32_t sx, uint32_t py, uint32_t px) {
  BH_ENTER_CALL(c);
  if (!in || !out_grad || !filts_grad) return bh::fail(BH_ERR, "null tensor");
  const uint32_t d[11] = {B, IC, H, W, OC, KY, KX, sy, sx, py, px};
  if (int rc = bck_check_dims(d)) return rc;
  return bh::launch_bck(c, in, nullptr, nullptr, out_grad, nullptr, filts_grad, nullptr, d);
}

int bh_conv2d_bck_biases(bh_ctx *c, const float *out_grad, float *biases_grad, uint32_t B, uint32_t OC, uint32_t OH,
                         uint32_t OW) {
  BH_ENTER_CALL(c);
  if (!out_grad || !biases_grad) return bh::fail(BH_ERR, "null tensor");
  if (!B || !OC || !OH || !OW) return bh::fail(BH_ERR, "bck conv: zero-sized dimension");
  // a 1x1 stride-1 op of one input channel has exactly this out_grad
  const uint32_t d[11] = {B, 1, OH, OW, OC, 1, 1, 1, 1, 0, 0};
  return bh::launch_bck(c, nullptr, nullptr, nullptr, out_grad, nullptr, nullptr, biases_grad, d);
}

int bh_conv_route_banks(bh_ctx *c, const uint32_t *dims, uint32_t *banks) {
  // c may be NULL: the tuning table's / heuristic's route (no device needed)
  if (!dims || !banks) return bh::fail(BH_ERR, "null argument");
  *banks = bh::conv_route_banks(c, dims);
  return BH_OK;
}

int bh_variant_name(int op, const uint32_t *dims, char *buf, size_t n) {
  if (!dims || !buf || !n) return bh::fail(BH_ERR, "null argument");
  std::string s;
  if (op == 0) s = bh::sgemm_variant(dims[0], dims[1], dims[2]);
  else if (op == 1) s = bh::conv_variant(dims);
  else if (op == 2 || op == 3) s = bh::bck_variant(nullptr, op, dims);
  else return bh::fail(BH_ERR, "unknown op kind");
  std::snprintf(buf, n, "%s", s.c_str());
  return BH_OK;
}

int bh_variant_name_ctx(bh_ctx *c, int op, const uint32_t *dims, char *buf, size_t n) {
  BH_ENTER(c);
  if (!dims || !buf || !n) return bh::fail(BH_ERR, "null argument");
  std::string s;
  if (op == 0) s = bh::sgemm_variant_ctx(c, dims[0], dims[1], dims[2]);
  else if (op == 1) s = bh::conv_variant_ctx(c, dims);
  else if (op == 2 || op == 3) s = bh::bck_variant(c, op, dims);
  else return bh::fail(BH_ERR, "unknown op kind");
  std::snprintf(buf, n, "%s", s.c_str());
  return BH_OK;
}

int bh_stamp(bh_ctx *c, int slot) {
  BH_ENTER(c);
  if (slot < 0 || slot >= STAMP_SLOTS) return bh::fail(BH_ERR, "stamp slot out of range");
  unsigned long long *t = (unsigned long long *)c->stamps;
  void *args[] = {&t, &slot};
  if (int rc = bh::barrier(c)) return rc;
  BH_HIP(hipLaunchKernel((const void *)stamp_kernel, dim3(1), dim3(64), args, 0, c->stream));
  return bh::check_launch("stamp");
}

int bh_spin(bh_ctx *c, int us) {
  BH_ENTER(c);
  if (us < 1 || us > 100000) return bh::fail(BH_ERR, "bh_spin: us out of range 1..100000");
  unsigned long long ticks = (unsigned long long)us * (unsigned long long)(c->stamp_hz / 1e6);
  void *args[] = {&ticks};
  if (int rc = bh::barrier(c)) return rc;
  BH_HIP(hipLaunchKernel((const void *)spin_kernel, dim3(1), dim3(64), args, 0, c->stream));
  return bh::check_launch("spin");
}

int bh_stamps_read(bh_ctx *c, int first, int n, double *us) {
  BH_ENTER(c);
  if (!us || first < 0 || n < 0 || first + n > STAMP_SLOTS) return bh::fail(BH_ERR, "bad stamp range");
  std::vector<unsigned long long> t(n);
  if (int rc = bh::barrier(c)) return rc;
  BH_HIP(hipMemcpyAsync(t.data(), (unsigned long long *)c->stamps + first, n * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost, c->stream));
  BH_HIP(hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) us[i] = (double)(t[i] - t[0]) * 1e6 / c->stamp_hz;
  return BH_OK;
}

int bh_capture_begin(bh_ctx *c) {
  BH_ENTER(c);
  bh_sched &sc = c->sched;
  if (sc.capturing) return bh::fail(BH_ERR, "bh_capture_begin: the context is already capturing");
  // scratch never grows inside a capture: bring every lane up to what eager narrow ops asked for
  // (workspace) and to lane 0's tickets (zero-filled, as lane 0's) now, without headroom. Lane 0 served
  // those eager ops: it holds both already.
  for (int k = 0; k < sc.lanes; ++k) {
    bh_lane &l = sc.lane[k];
    if (int rc = bh::grow_buffer(c, l.ws, l.ws_bytes, sc.hw_ws, false, "split-K workspace", false)) return rc;
    size_t have = l.cnt_n * 4;
    int rc = bh::grow_buffer(c, l.cnt, have, sc.lane[0].cnt_n * 4, true, "split-K tickets", false);
    l.cnt_n = have / 4;
    if (rc != BH_OK) return rc;
    l.forked = false;
  }
  BH_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  sc.capturing = true;
  sc.trk.join();
  sc.ev_used = 0;
  sc.used_mask = 0;
  sc.cur_trace.clear();
  for (uint32_t &v : sc.cur) v = 0;
  return BH_OK;
}

int bh_capture_end(bh_ctx *c, int *graph_id) {
  BH_ENTER(c);
  if (!graph_id) return bh::fail(BH_ERR, "null out");
  hipGraph_t g = nullptr;
  bh_sched &sc = c->sched;
  // whatever happened inside the capture, the scheduler leaves it here: all lanes joined, nothing
  // outstanding (a join that fails means the capture is invalid; hipStreamEndCapture reports that)
  const int jrc = bh::barrier(c);
  const std::string jmsg = jrc == BH_OK ? std::string() : std::string(bh_last_error());
  sc.capturing = false;
  sc.trk.join();
  for (bh_lane &l : sc.lane) l.forked = false;
  BH_HIP(hipStreamEndCapture(c->stream, &g));
  if (jrc != BH_OK) {
    if (g) (void)hipGraphDestroy(g);
    return bh::fail(BH_ERR, "bh_capture_end: joining the capture lanes failed: " + jmsg);
  }
  sc.stats[0] = (uint32_t)__builtin_popcount(sc.used_mask);
  for (int i = 1; i < 4; ++i) sc.stats[i] = sc.cur[i];
  sc.trace = sc.cur_trace;
  hipGraphExec_t ge = nullptr;
  hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return bh::fail(BH_ERR, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
  c->graphs.push_back(ge);
  *graph_id = (int)c->graphs.size() - 1;
  return BH_OK;
}

int bh_capture_stats(bh_ctx *c, uint32_t out[4]) {
  BH_CHECK_CTX(c);
  if (!out) return bh::fail(BH_ERR, "null out");
  for (int i = 0; i < 4; ++i) out[i] = c->sched.stats[i];
  return BH_OK;
}

int bh_capture_trace(bh_ctx *c, uint32_t *out, uint32_t cap, uint32_t *n) {
  BH_CHECK_CTX(c);
  if (!n || (cap && !out)) return bh::fail(BH_ERR, "null out");
  *n = (uint32_t)c->sched.trace.size();
  for (uint32_t i = 0; i < cap && i < *n; ++i) out[i] = c->sched.trace[i];
  return BH_OK;
}

int bh_graph_launch(bh_ctx *c, int graph_id) {
  BH_ENTER(c);
  if (graph_id < 0 || graph_id >= (int)c->graphs.size() || !c->graphs[graph_id]) return bh::fail(BH_ERR, "bad graph id");
  BH_HIP(hipGraphLaunch(c->graphs[graph_id], c->stream));
  return BH_OK;
}

int bh_graph_destroy(bh_ctx *c, int graph_id) {
  BH_ENTER(c);
  if (graph_id < 0 || graph_id >= (int)c->graphs.size() || !c->graphs[graph_id]) return bh::fail(BH_ERR, "bad graph id");
  BH_HIP(hipStreamSynchronize(c->stream));
  BH_HIP(hipGraphExecDestroy(c->graphs[graph_id]));
  c->graphs[graph_id] = nullptr;
  // outgrown workspaces were kept for the graphs that captured them: free them with the last one
  bool live_graph = false;
  for (hipGraphExec_t g : c->graphs) live_graph |= g != nullptr;
  if (!live_graph) {
    for (void *r : c->retired) BH_HIP(hipFree(r));
    c->retired.clear();
  }
  return BH_OK;
}

int bh_tune_set(bh_ctx *c, int op, int cfg_index, int splits) {
  BH_ENTER(c);
  if (op == 2 || op == 3) return bh::bck_tune_set(c, op, cfg_index, splits);
  return bh::tune_set(c, op, cfg_index, splits);
}

int bh_tune_set_policy(bh_ctx *c, int op, int wt) {
  BH_ENTER(c);
  return bh::tune_set_wt(c, op, wt);
}

int bh_tune_cfg_name(int op, int cfg_index, char *buf, size_t n) {
  if (!buf || !n) return bh::fail(BH_ERR, "null buffer");
  std::string s;
  int rc = (op == 2 || op == 3) ? bh::bck_tune_cfg_name(op, cfg_index, s) : bh::tune_cfg_name(op, cfg_index, s);
  if (rc == BH_OK) std::snprintf(buf, n, "%s", s.c_str());
  return rc;
}

}  // extern "C"
