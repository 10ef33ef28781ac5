// bh_bckops.hip -- the backward pass of the non-conv layers of Boda's net executor (add_bck_ops:
// coi src/conv_util.cc:40-64, emitted at src/rtc_fwd.cc:345-404) as gfx950 kernels: Spreading (the
// backward of Pooling), BckLRN, ZeroIfNonPos (the backward of ReLU), Reduce (the sum of a fan-out node's
// partial gradients) and SoftmaxWithLoss's gradient / loss pair. BckDropout is bh_dropout_inplace and
// Split is bh_chan_copy (bh_fwdops.hip). All are HBM-bound: one pass, coalesced along x (or the flat
// index), no atomics, a fixed summation order -- two calls on the same inputs give the same bits.
// Every entry has two forms: 0 the production kernel, 1 "ref64" (one thread per output element, double
// accumulation over the true terms, rounded once): the known-good tune of ops-prof sweeps, never routed.
#include "bh_common.h"

#include <cfloat>
#include <cmath>

namespace {

// 8 blocks of 256 per CU at the most; the kernels stride over the rest
uint32_t grid_for(const bh_ctx *ctx, uint64_t n) { return bh::grid_for(n, bh::num_cus(ctx) * 8); }

// Spreading (test/rtc/spreading.cucl): one thread per in_grad element, lanes along x. The windows that
// cover input pixel (y, x) are oy in [ceil((y + py - KY + 1) / sy), floor((y + py) / sy)] clipped to
// [0, OH), likewise ox: at most ceil(KY / sy) * ceil(KX / sx) of them, summed oy-major, ox-minor.
// max: a window contributes its out_grad iff its out_in_yx names this pixel. avg: it contributes
// out_grad / (its in-image tap count, from the window bounds): the exact adjoint of pool_kernel.
// KY_/KX_/S_ > 0: window and stride are compile-time constants (the fixed pools of the reference nets),
// so the window loop unrolls into ceil(K/S)^2 unguarded loads issued together; a window past the
// covering range loads element 0 (always valid) and is then ignored.
template <int KY_, int KX_, int S_, typename ACC>
__global__ __launch_bounds__(256) void spreading_kernel(const float *__restrict__ og, const float *__restrict__ oyx,
                                                        float *__restrict__ in_grad, uint32_t total, uint32_t H,
                                                        uint32_t W, uint32_t OH, uint32_t OW, uint32_t KY_rt,
                                                        uint32_t KX_rt, uint32_t sy_rt, uint32_t sx_rt, uint32_t py,
                                                        uint32_t px, int avg, uint32_t w_m, uint32_t w_s,
                                                        uint32_t h_m, uint32_t h_s) {
  const uint32_t KY = KY_ > 0 ? (uint32_t)KY_ : KY_rt, KX = KX_ > 0 ? (uint32_t)KX_ : KX_rt;
  const uint32_t sy = S_ > 0 ? (uint32_t)S_ : sy_rt, sx = S_ > 0 ? (uint32_t)S_ : sx_rt;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    // i -> (nc, y, x) with multiply-shift division (nc = img * C + chan)
    const uint32_t t = (__umulhi(i, w_m) + i) >> w_s, x = i - t * W;
    const uint32_t nc = (__umulhi(t, h_m) + t) >> h_s, y = t - nc * H;
    const size_t obase = (size_t)nc * OH * OW;
    const uint32_t ay = y + py, ax = x + px;
    const int oy_lo = ay >= KY ? (int)((ay - KY) / sy + 1) : 0, oy_hi = min((int)(ay / sy), (int)OH - 1);
    const int ox_lo = ax >= KX ? (int)((ax - KX) / sx + 1) : 0, ox_hi = min((int)(ax / sx), (int)OW - 1);
    const float me = (float)(y * W + x);
    ACC acc = 0;
    auto win = [&](int oy, int ox, bool ok) {
      const size_t o = ok ? obase + (size_t)oy * OW + ox : 0;
      const float g = og[o];
      if (avg) {
        const int iy0 = oy * (int)sy - (int)py, ix0 = ox * (int)sx - (int)px;
        const int rows = min((int)H, iy0 + (int)KY) - max(0, iy0), cols = min((int)W, ix0 + (int)KX) - max(0, ix0);
        acc += ok ? (ACC)g / (ACC)(float)(rows * cols) : (ACC)0;
      } else {
        acc += (ok && oyx[o] == me) ? (ACC)g : (ACC)0;
      }
    };
    if constexpr (KY_ > 0 && KX_ > 0 && S_ > 0) {
      constexpr int NY = (KY_ + S_ - 1) / S_, NX = (KX_ + S_ - 1) / S_;
#pragma unroll
      for (int j = 0; j < NY; ++j)
#pragma unroll
        for (int k = 0; k < NX; ++k) win(oy_lo + j, ox_lo + k, oy_lo + j <= oy_hi && ox_lo + k <= ox_hi);
    } else {
      for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int ox = ox_lo; ox <= ox_hi; ++ox) win(oy, ox, true);
    }
    in_grad[i] = (float)acc;
  }
}

// BckLRN (test/rtc/bck_lrn.cucl). With t[c] = out_grad[c] * out[c] / scale_base[c] per pixel:
//   in_grad[c] = out_grad[c] * scale_base[c]^-beta + in[c] * coef * sum of t over the window of c,
//   coef = -2 * beta * alpha / local_size.
// As lrn_kernel, a thread owns BLRN_CH output channels of one pixel (threads of a wave: adjacent pixels,
// coalesced), so ops with few pixels and many channels still fill the device. It builds its
// BLRN_CH + LS - 1 terms in registers -- a chunk re-reads the LS/2 channels on either side, so its
// windows hold the true neighbouring terms (zeros outside [0, C)) -- and each output sums its own LS
// terms in ascending channel order: the sum does not depend on where the chunks are cut.
constexpr int BLRN_CH = 8;
template <int LS>
__global__ __launch_bounds__(256) void lrn_bck_kernel(const float *__restrict__ in, const float *__restrict__ out,
                                                      const float *__restrict__ sb, const float *__restrict__ og,
                                                      float *__restrict__ in_grad, uint32_t npix, uint32_t C,
                                                      uint32_t HW, float coef, float beta, uint32_t total) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const uint32_t chunk = t / npix, i = t - chunk * npix;
  const uint32_t img = i / HW, pix = i - img * HW;
  const size_t base = (size_t)img * C * HW + pix;
  constexpr int hls = LS >> 1, NI = BLRN_CH + 2 * hls;
  const int c0 = (int)chunk * BLRN_CH;  // first output channel
  float term[NI], g[BLRN_CH], s[BLRN_CH];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int c = c0 - hls + j;
    const bool ok = c >= 0 && c < (int)C;
    const size_t off = base + (size_t)(ok ? c : 0) * HW;  // channel 0 is always there
    const float a = og[off], b = out[off], d = sb[off];
    term[j] = ok ? a * b / d : 0.0f;
    if (j >= hls && j < hls + BLRN_CH) {
      g[j - hls] = a;
      s[j - hls] = d;
    }
  }
#pragma unroll
  for (int j = 0; j < BLRN_CH; ++j) {
    const int oc = c0 + j;
    if (oc < (int)C) {
      float sum = 0.0f;
#pragma unroll
      for (int w = 0; w < LS; ++w) sum += term[j + w];
      const size_t off = base + (size_t)oc * HW;
      // scale_base^-beta on the hardware transcendentals, as lrn_kernel computes it
      in_grad[off] = g[j] * __builtin_amdgcn_exp2f(-beta * __builtin_amdgcn_logf(s[j])) + in[off] * coef * sum;
    }
  }
}

__global__ __launch_bounds__(256) void lrn_bck_ref64_kernel(const float *__restrict__ in,
                                                            const float *__restrict__ out,
                                                            const float *__restrict__ sb,
                                                            const float *__restrict__ og,
                                                            float *__restrict__ in_grad, uint32_t C, uint32_t HW,
                                                            int hls, double coef, double beta, uint32_t total) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const uint32_t c = (i / HW) % C;
  const size_t base = (size_t)i - (size_t)c * HW;  // channel 0 of this pixel
  double sum = 0.0;
  for (int cc = max(0, (int)c - hls); cc <= min((int)C - 1, (int)c + hls); ++cc) {
    const size_t off = base + (size_t)cc * HW;
    sum += (double)og[off] * (double)out[off] / (double)sb[off];
  }
  in_grad[i] = (float)((double)og[i] * pow((double)sb[i], -beta) + (double)in[i] * coef * sum);
}

// ZeroIfNonPos (test/rtc/ZeroIfNonPos.cucl): out = cond > 0 ? in : 0 as a select, so a NaN cond gives 0
// and a NaN in under cond <= 0 gives 0. 16-byte accesses with an element tail (relu_kernel's shape);
// out may alias in, so neither is __restrict__.
__global__ __launch_bounds__(256) void zero_if_non_pos_kernel(const float *in, const float *__restrict__ cond,
                                                              float *out, uint64_t n, int vec) {
  const uint64_t n4 = vec ? n / 4 : 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * 256) {
    const float4 c = ((const float4 *)cond)[i];
    float4 v = ((const float4 *)in)[i];
    v.x = c.x > 0.0f ? v.x : 0.0f;
    v.y = c.y > 0.0f ? v.y : 0.0f;
    v.z = c.z > 0.0f ? v.z : 0.0f;
    v.w = c.w > 0.0f ? v.w : 0.0f;
    ((float4 *)out)[i] = v;
  }
  // the tail (everything when the pointers are not 16-byte aligned)
  for (uint64_t i = n4 * 4 + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    out[i] = cond[i] > 0.0f ? in[i] : 0.0f;
}

// Reduce (test/rtc/reduce.cucl): out = ((0 + ins_0) + ins_1) + ..., in that order. The inputs arrive as
// one by-value kernel argument; N is a compile-time constant so the loop unrolls over it.
struct reduce_ins {
  const float *p[8];
};
template <int N, typename ACC>
__global__ __launch_bounds__(256) void reduce_kernel(reduce_ins ins, float *out, uint64_t n, int vec) {
  const uint64_t n4 = vec ? n / 4 : 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * 256) {
    float4 v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((const float4 *)ins.p[k])[i];
    ACC a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      a0 += (ACC)v[k].x;
      a1 += (ACC)v[k].y;
      a2 += (ACC)v[k].z;
      a3 += (ACC)v[k].w;
    }
    ((float4 *)out)[i] = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
  }
  for (uint64_t i = n4 * 4 + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    ACC a = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) a += (ACC)ins.p[k][i];
    out[i] = (float)a;
  }
}

// sm_grad_and_loss (test/rtc/sm_grad_and_loss.cucl), with l = (int)label[n][y][x]:
//   loss_per_pel[n][y][x] = -log(max(prob[n][l][y][x], FLT_MIN)),  in_grad = (prob - [c == l]) / B.
// A pixel-per-thread form has B threads at the 1x1 maps this op runs on, each striding through C. Here
// a block takes one image and a run of PL pixels (PL a power of two <= 64, lanes along the pixels) and
// spreads the channel loop over its 256 / PL channel lanes: at HW = 1 adjacent lanes hold adjacent
// channels, at HW >= 64 adjacent pixels; both are contiguous in memory.
// A label outside [0, C) (or NaN) reads nothing: that pixel's loss and gradient column become NaN.
template <typename ACC>
__global__ __launch_bounds__(256) void sm_grad_and_loss_kernel(const float *__restrict__ prob,
                                                               const float *__restrict__ label,
                                                               float *__restrict__ in_grad,
                                                               float *__restrict__ loss_per_pel, uint32_t B,
                                                               uint32_t C, uint32_t HW, uint32_t PL, uint32_t runs) {
  const uint32_t img = blockIdx.x / runs, run = blockIdx.x - img * runs;
  const uint32_t pl = threadIdx.x & (PL - 1), cl = threadIdx.x / PL, CL = 256 / PL;
  const uint32_t pix = run * PL + pl;
  if (pix >= HW) return;
  const float lab = label[(size_t)img * HW + pix];
  const bool valid = lab >= 0.0f && lab < (float)C;  // false for NaN, and for (-1, 0)
  const uint32_t l = valid ? (uint32_t)(int)lab : 0u;
  const size_t base = (size_t)img * C * HW + pix;
  const float nan = __builtin_nanf("");
  for (uint32_t c = cl; c < C; c += CL) {
    const size_t off = base + (size_t)c * HW;
    const ACC v = ((ACC)prob[off] - (c == l ? (ACC)1 : (ACC)0)) / (ACC)B;
    in_grad[off] = valid ? (float)v : nan;
  }
  if (cl == 0) {
    const float p = fmaxf(prob[base + (size_t)l * HW], FLT_MIN);
    float loss;
    if constexpr (sizeof(ACC) == 8) loss = (float)-log((double)p);
    else loss = -logf(p);
    loss_per_pel[(size_t)img * HW + pix] = valid ? loss : nan;
  }
}

// sum_loss_over_imgs (test/rtc/sum_loss_over_imgs.cucl): loss[y][x] = (sum over n ascending of
// loss_per_pel[n][y][x]) / B. One thread per pixel.
template <typename ACC>
__global__ __launch_bounds__(256) void sum_loss_over_imgs_kernel(const float *__restrict__ loss_per_pel,
                                                                 float *__restrict__ loss, uint32_t B, uint32_t HW) {
  const uint32_t pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  ACC s = 0;
  for (uint32_t n = 0; n < B; ++n) s += (ACC)loss_per_pel[(size_t)n * HW + pix];
  loss[pix] = (float)(s / (ACC)B);
}

int check_form(int form) {
  if (form != 0 && form != 1) return bh::fail(BH_UNSUP, "backward op: form must be 0 (production) or 1 (ref64)");
  return BH_OK;
}

int launch_spreading(bh_ctx *ctx, const float *og, const float *oyx, float *in_grad, uint32_t B, uint32_t C,
                     uint32_t H, uint32_t W, uint32_t KY, uint32_t KX, uint32_t sy, uint32_t sx, uint32_t py,
                     uint32_t px, int avg, int form) {
  uint32_t OH = bh::pool_out_sz(H, KY, sy, py), OW = bh::pool_out_sz(W, KX, sx, px);
  const uint64_t total = (uint64_t)B * C * H * W;
  if (total >= (1ull << 31) || (uint64_t)B * C * OH * OW >= (1ull << 31))
    return bh::fail(BH_UNSUP, "spreading: tensor too large");
  // out_in_yx holds y*W+x as a float (the forward's format): exact only below 2^24
  if (!avg && (uint64_t)H * W > (1ull << 24)) return bh::fail(BH_UNSUP, "spreading: plane too large for out_in_yx");
  uint32_t tot = (uint32_t)total, w_m, w_s, h_m, h_s;
  bh::set_fd(W, w_m, w_s);
  bh::set_fd(H, h_m, h_s);
  void *args[] = {&og, &oyx, &in_grad, &tot, &H, &W, &OH, &OW, &KY, &KX, &sy, &sx, &py, &px, &avg, &w_m, &w_s, &h_m, &h_s};
  const void *kern = (const void *)spreading_kernel<0, 0, 0, float>;
  if (form == 1) kern = (const void *)spreading_kernel<0, 0, 0, double>;
  else if (KY == 3 && KX == 3 && sy == 2 && sx == 2) kern = (const void *)spreading_kernel<3, 3, 2, float>;
  else if (KY == 3 && KX == 3 && sy == 1 && sx == 1) kern = (const void *)spreading_kernel<3, 3, 1, float>;
  else if (KY == 2 && KX == 2 && sy == 2 && sx == 2) kern = (const void *)spreading_kernel<2, 2, 2, float>;
  return bh::launch(ctx, kern, dim3(grid_for(ctx, total)), dim3(256), args, true, true, "spreading");
}

int launch_lrn_bck(bh_ctx *ctx, const float *in, const float *out, const float *sb, const float *og, float *in_grad,
                   uint32_t B, uint32_t C, uint32_t H, uint32_t W, uint32_t local_size, float alpha, float beta,
                   float k, int form) {
  (void)k;  // out_scale_base carries it
  if (!(local_size & 1) || local_size > 11) return bh::fail(BH_UNSUP, "lrn_bck: local_size must be odd and <= 11");
  const uint64_t np = (uint64_t)B * H * W;
  if (np * C >= (1ull << 31)) return bh::fail(BH_UNSUP, "lrn_bck: tensor too large");
  uint32_t npix = (uint32_t)np, HW = H * W;
  const double coef64 = -2.0 * (double)beta * (double)alpha / (double)local_size;
  if (form == 1) {
    uint32_t total = npix * C;
    int hls = (int)(local_size >> 1);
    double beta64 = beta, c64 = coef64;
    void *args[] = {&in, &out, &sb, &og, &in_grad, &C, &HW, &hls, &c64, &beta64, &total};
    return bh::launch(ctx, (const void *)lrn_bck_ref64_kernel, dim3((total + 255) / 256), dim3(256), args, true, true,
                      "lrn_bck_ref64");
  }
  uint32_t total = npix * ((C + BLRN_CH - 1) / BLRN_CH);  // threads: pixels x channel chunks (< 2^31)
  float coef = (float)coef64;
  void *args[] = {&in, &out, &sb, &og, &in_grad, &npix, &C, &HW, &coef, &beta, &total};
  const void *kern = nullptr;
  switch (local_size) {
    case 1: kern = (const void *)lrn_bck_kernel<1>; break;
    case 3: kern = (const void *)lrn_bck_kernel<3>; break;
    case 5: kern = (const void *)lrn_bck_kernel<5>; break;
    case 7: kern = (const void *)lrn_bck_kernel<7>; break;
    case 9: kern = (const void *)lrn_bck_kernel<9>; break;
    default: kern = (const void *)lrn_bck_kernel<11>; break;
  }
  return bh::launch(ctx, kern, dim3((total + 255) / 256), dim3(256), args, true, true, "lrn_bck");
}

template <typename ACC>
const void *reduce_kern(uint32_t n_ins) {
  switch (n_ins) {
    case 1: return (const void *)reduce_kernel<1, ACC>;
    case 2: return (const void *)reduce_kernel<2, ACC>;
    case 3: return (const void *)reduce_kernel<3, ACC>;
    case 4: return (const void *)reduce_kernel<4, ACC>;
    case 5: return (const void *)reduce_kernel<5, ACC>;
    case 6: return (const void *)reduce_kernel<6, ACC>;
    case 7: return (const void *)reduce_kernel<7, ACC>;
    default: return (const void *)reduce_kernel<8, ACC>;
  }
}

int launch_sm_grad_and_loss(bh_ctx *ctx, const float *prob, const float *label, float *in_grad, float *loss_per_pel,
                            uint32_t B, uint32_t C, uint32_t H, uint32_t W, int form, bool first, bool last) {
  uint32_t HW = H * W, PL = 1;
  while (PL < 64 && PL < HW) PL *= 2;
  uint32_t runs = (HW + PL - 1) / PL;
  const uint64_t blocks = (uint64_t)B * runs;
  if (blocks >= (1ull << 31)) return bh::fail(BH_UNSUP, "sm_grad_and_loss: tensor too large");
  void *args[] = {&prob, &label, &in_grad, &loss_per_pel, &B, &C, &HW, &PL, &runs};
  const void *kern = form == 1 ? (const void *)sm_grad_and_loss_kernel<double> : (const void *)sm_grad_and_loss_kernel<float>;
  return bh::launch(ctx, kern, dim3((uint32_t)blocks), dim3(256), args, first, last, "sm_grad_and_loss");
}

int launch_sum_loss_over_imgs(bh_ctx *ctx, const float *loss_per_pel, float *loss, uint32_t B, uint32_t HW, int form,
                              bool first, bool last) {
  void *args[] = {&loss_per_pel, &loss, &B, &HW};
  const void *kern = form == 1 ? (const void *)sum_loss_over_imgs_kernel<double> : (const void *)sum_loss_over_imgs_kernel<float>;
  return bh::launch(ctx, kern, dim3((HW + 255) / 256), dim3(256), args, first, last, "sum_loss_over_imgs");
}

// B x C x H x W with no zero extent, below 2^31 elements
int check_nchw(const char *what, uint32_t B, uint32_t C, uint32_t H, uint32_t W) {
  if (!B || !C || !H || !W) return bh::fail(BH_UNSUP, std::string(what) + ": zero-sized dimension");
  if ((uint64_t)B * C * H * W >= (1ull << 31) || (uint64_t)H * W >= (1ull << 31))
    return bh::fail(BH_UNSUP, std::string(what) + ": tensor too large");
  return BH_OK;
}

}  // namespace

// ---- C-ABI entries (include/boda_hip.h). None opens an op_scope: inside a capture they are barriers,
// as bh_pool_fwd_nchw / bh_lrn_fwd_nchw are.

int bh_spreading_nchw(bh_ctx *c, const float *out_grad, const float *out_in_yx, float *in_grad, uint32_t B,
                      uint32_t C, uint32_t H, uint32_t W, uint32_t KY, uint32_t KX, uint32_t sy, uint32_t sx,
                      uint32_t py, uint32_t px, int avg, int form) {
  BH_ENTER_CALL(c);
  if (!out_grad || !in_grad || (!avg && !out_in_yx)) return bh::fail(BH_ERR, "null tensor");
  if (!B || !C || !H || !W || !KY || !KX || !sy || !sx) return bh::fail(BH_UNSUP, "spreading: zero-sized dimension");
  if (py >= KY || px >= KX) return bh::fail(BH_UNSUP, "spreading: padding must be smaller than the window");
  if (int rc = check_form(form)) return rc;
  return launch_spreading(c, out_grad, out_in_yx, in_grad, B, C, H, W, KY, KX, sy, sx, py, px, avg ? 1 : 0, form);
}

int bh_lrn_bck_nchw(bh_ctx *c, const float *in, const float *out, const float *out_scale_base, const float *out_grad,
                    float *in_grad, uint32_t B, uint32_t C, uint32_t H, uint32_t W, uint32_t local_size, float alpha,
                    float beta, float k, int form) {
  BH_ENTER_CALL(c);
  if (!in || !out || !out_scale_base || !out_grad || !in_grad) return bh::fail(BH_ERR, "null tensor");
  if (!B || !C || !H || !W) return bh::fail(BH_UNSUP, "lrn_bck: zero-sized dimension");
  if (int rc = check_form(form)) return rc;
  return launch_lrn_bck(c, in, out, out_scale_base, out_grad, in_grad, B, C, H, W, local_size, alpha, beta, k, form);
}

int bh_zero_if_non_pos(bh_ctx *c, const float *in, const float *cond, float *out, uint64_t n, int form) {
  BH_ENTER_CALL(c);
  if (!in || !cond || !out) return bh::fail(BH_ERR, "null tensor");
  if (!n) return bh::fail(BH_UNSUP, "zero_if_non_pos: zero-sized tensor");
  if (int rc = check_form(form)) return rc;
  // form 1 is the element-per-thread loop alone
  int vec = form == 0 && !((uintptr_t)in % 16 || (uintptr_t)cond % 16 || (uintptr_t)out % 16);
  void *args[] = {&in, &cond, &out, &n, &vec};
  return bh::launch(c, (const void *)zero_if_non_pos_kernel, dim3(grid_for(c, vec ? n / 4 + 1 : n)), dim3(256), args,
                    true, true, "zero_if_non_pos");
}

int bh_reduce_sum(bh_ctx *c, const float *const *ins, uint32_t n_ins, float *out, uint64_t n, int form) {
  BH_ENTER_CALL(c);
  if (!ins || !out) return bh::fail(BH_ERR, "null tensor");
  if (n_ins < 1 || n_ins > 8) return bh::fail(BH_UNSUP, "reduce: 1 to 8 inputs");
  if (!n) return bh::fail(BH_UNSUP, "reduce: zero-sized tensor");
  if (int rc = check_form(form)) return rc;
  reduce_ins p{};
  int vec = form == 0 && (uintptr_t)out % 16 == 0;
  for (uint32_t k = 0; k < n_ins; ++k) {
    if (!ins[k]) return bh::fail(BH_ERR, "null tensor");
    p.p[k] = ins[k];
    vec = vec && (uintptr_t)ins[k] % 16 == 0;
  }
  void *args[] = {&p, &out, &n, &vec};
  const void *kern = form == 1 ? reduce_kern<double>(n_ins) : reduce_kern<float>(n_ins);
  return bh::launch(c, kern, dim3(grid_for(c, vec ? n / 4 + 1 : n)), dim3(256), args, true, true, "reduce");
}

int bh_sm_grad_and_loss(bh_ctx *c, const float *prob, const float *label, float *in_grad, float *loss_per_pel,
                        uint32_t B, uint32_t C, uint32_t H, uint32_t W, int form) {
  BH_ENTER_CALL(c);
  if (!prob || !label || !in_grad || !loss_per_pel) return bh::fail(BH_ERR, "null tensor");
  if (int rc = check_nchw("sm_grad_and_loss", B, C, H, W)) return rc;
  if (int rc = check_form(form)) return rc;
  return launch_sm_grad_and_loss(c, prob, label, in_grad, loss_per_pel, B, C, H, W, form, true, true);
}

int bh_sum_loss_over_imgs(bh_ctx *c, const float *loss_per_pel, float *loss, uint32_t B, uint32_t HW, int form) {
  BH_ENTER_CALL(c);
  if (!loss_per_pel || !loss) return bh::fail(BH_ERR, "null tensor");
  if (int rc = check_nchw("sum_loss_over_imgs", B, 1, 1, HW)) return rc;
  if (int rc = check_form(form)) return rc;
  return launch_sum_loss_over_imgs(c, loss_per_pel, loss, B, HW, form, true, true);
}

int bh_softmax_with_loss(bh_ctx *c, const float *in, const float *label, float *prob, float *in_grad,
                         float *loss_per_pel, float *loss, uint32_t B, uint32_t C, uint32_t H, uint32_t W, int form) {
  BH_ENTER_CALL(c);
  if (!in || !label || !prob || !in_grad || !loss_per_pel || !loss) return bh::fail(BH_ERR, "null tensor");
  if (int rc = check_nchw("softmax_with_loss", B, C, H, W)) return rc;
  if (int rc = check_form(form)) return rc;
  // softmax has one form; the gradient, the loss and the image sum take `form`
  if (int rc = bh::launch_softmax(c, in, prob, B, C, H, W, true, false)) return rc;
  if (int rc = launch_sm_grad_and_loss(c, prob, label, in_grad, loss_per_pel, B, C, H, W, form, false, false)) return rc;
  return launch_sum_loss_over_imgs(c, loss_per_pel, loss, B, H * W, form, false, true);
}
