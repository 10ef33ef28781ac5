// bh_bck.hip -- backward convolution: Boda's BckConv (coi src/conv_util.cc:65, planned
// src/cnn_op.cc:80-160, emitted as BckConv_{in,filts,biases}_grad_loss, src/rtc_fwd.cc:378-400).
// Dense fp32 NCHW, ogl = out_grad_loss B x OC x OH x OW:
//   in_grad[n][ic][y][x]       = sum_{oc,ky,kx : oy*sy+ky-py == y, ox*sx+kx-px == x} ogl[n][oc][oy][ox] * filts[oc][ic][ky][kx]
//   filts_grad[oc][ic][ky][kx] = sum_{n,oy,ox} ogl[n][oc][oy][ox] * in[n][ic][oy*sy+ky-py][ox*sx+kx-px]  (in-image taps)
//   biases_grad[oc]            = sum_{n,oy,ox} ogl[n][oc][oy][ox]
// Routes:
//   - input gradient, stride 1 and pad <= K-1: the forward conv of ogl with the bank transposed (oc <-> ic)
//     and flipped in ky, kx at pad (KY-1-py, KX-1-px), through launch_conv: every tuned forward route serves
//     it. The only device code here is the transpose-flip (xflip_kernel), the head of the bck pack.
//   - input gradient otherwise (bcki_kernel): the reference's phase decomposition. Pixels with
//     (y+py) mod sy == ry, (x+px) mod sx == rx see only the taps ky = ry + sy*j, kx = rx + sx*i, at
//     oy = (y+py)/sy - j, ox = (x+px)/sx - i: per phase a stride-1 implicit GEMM, M = IC, N = the phase's
//     pixels over the batch, K = OC * taps of the phase. Grid z = phase. A phase without taps has K = 0 and
//     stores zeros; a tap outside the output is a load that misses.
//   - filter gradient (bckf_kernel): C[OC][IC*KY*KX] = A * X^T over r = (n, oy, ox), A = ogl, X = the im2col
//     of in. The reduction is split over grid z; every split stores its partial tile to the context
//     workspace and bckf_reduce_kernel adds the splits in the order 0..S-1 (never by arrival).
//   - bias gradient (bckb_kernel): one block per output channel, lanes along pixels, fixed-order tree.
//   - "ref64" forms of all three: one thread per output, double accumulation, rounded once.
// All MFMA is __builtin_amdgcn_mfma_f32_32x32x2f32: lane l holds A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31]; accumulator r of lane l is row (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), column l & 31.
#include "bh_gemm_dev.h"

namespace bhk {
namespace {

struct BckArgs {
  const float *in, *filts, *ogl;
  float *in_grad, *filts_grad, *biases_grad, *ws;
  uint32_t B, IC, H, W, OC, KY, KX, sy, sx, py, px, OH, OW;
  uint32_t OHW, HW, KYX, Q, R;  // Q = IC*KY*KX (filter-gradient columns), R = B*OH*OW (its reduction)
  uint32_t in_bytes, ogl_bytes, filts_bytes;
  uint32_t ohw_m, ohw_s, ow_m, ow_s, kyx_m, kyx_s, kx_m, kx_s;
  uint32_t cps, S, ocp, qp;  // bckf: 64-deep chunks per split, splits, padded partial extents
};

// ---- filter gradient -------------------------------------------------------------------------------
// Block tile BM (oc) x BN (q = (ic, ky, kx)), one 32 x 32 MFMA tile per wave, the reduction in chunks of
// 64 r. Both operands are read from global memory with the lanes along r (ogl is contiguous in (oy, ox)
// for one (n, oc); the im2col of in is contiguous in ox at stride 1), one row per wave instruction, and
// staged in LDS as [row][r] with a row stride of LD = 65 floats:
//   write: a wave stores one row, lane = r: 64 consecutive floats, 64 banks, conflict-free;
//   read:  lane l = (i = l & 31, h = l >> 5) takes [i][32 h + kk] for MFMA step kk (the k order inside a
//          chunk is free as long as A and X agree): word 65 i + 32 h + kk = bank (i + 32 h + kk) mod 64,
//          distinct for the 64 (i, h). An even stride would put rows i and i + 32/gcd on one bank.
template <int BM, int BN>
__global__ __launch_bounds__((BM / 32) * (BN / 32) * 64) void bckf_kernel(BckArgs p) {
  constexpr int WN = BN / 32, NW = (BM / 32) * WN, LD = 65, RA = BM / NW, RX = BN / NW;
  __shared__ float sa[BM * LD];
  __shared__ float sx[BN * LD];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t wm = wave / WN, wn = wave % WN, li = lane & 31u, lh = lane >> 5;
  const uint32_t oc0 = blockIdx.y * BM, q0 = blockIdx.x * BN, s = blockIdx.z;
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.ogl, p.ogl_bytes), rx = make_rsrc(p.in, p.in_bytes);
  const uint32_t nch = (p.R + 63u) / 64u, c0 = s * p.cps, c1 = min(nch, c0 + p.cps);
  float ga[RA], gx[RX];
  auto load = [&](uint32_t c) {
    const uint32_t r = c * 64u + lane;
    const uint32_t n = fdiv(r, p.ohw_m, p.ohw_s), pix = r - n * p.OHW;
    const uint32_t oy = fdiv(pix, p.ow_m, p.ow_s), ox = pix - oy * p.OW;
    const bool rok = r < p.R;
    const uint32_t abase = n * p.OC * p.OHW + pix;
#pragma unroll
    for (int j = 0; j < RA; ++j) {
      const uint32_t oc = oc0 + wave * RA + j;
      ga[j] = ld1(ra, oob_unless(rok & (oc < p.OC), (abase + oc * p.OHW) * 4u));
    }
    const uint32_t iy0 = oy * p.sy - p.py, ix0 = ox * p.sx - p.px, xbase = n * p.IC * p.HW;
#pragma unroll
    for (int j = 0; j < RX; ++j) {
      const uint32_t q = q0 + wave * RX + j;  // wave-uniform: the tap decomposition is scalar work
      const uint32_t ic = fdiv(q, p.kyx_m, p.kyx_s), t = q - ic * p.KYX;
      const uint32_t ky = fdiv(t, p.kx_m, p.kx_s), kx = t - ky * p.KX;
      const uint32_t iy = iy0 + ky, ix = ix0 + kx;  // a tap above / left of the image wraps past H / W
      const bool ok = rok & (q < p.Q) & (iy < p.H) & (ix < p.W);
      gx[j] = ld1(rx, oob_unless(ok, (xbase + ic * p.HW + iy * p.W + ix) * 4u));
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if (c0 < c1) load(c0);
  for (uint32_t c = c0; c < c1; ++c) {
#pragma unroll
    for (int j = 0; j < RA; ++j) sa[(wave * RA + j) * LD + lane] = ga[j];
#pragma unroll
    for (int j = 0; j < RX; ++j) sx[(wave * RX + j) * LD + lane] = gx[j];
    __syncthreads();
    if (c + 1 < c1) load(c + 1);  // in flight under this chunk's MFMAs
    const float *pa = &sa[(wm * 32u + li) * LD + lh * 32u], *pb = &sx[(wn * 32u + li) * LD + lh * 32u];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
    __syncthreads();
  }
  // the split's partial tile: ws[s][ocp][qp] (padded to whole tiles: no bounds here)
  float *w = p.ws + ((size_t)s * p.ocp + oc0 + wm * 32u) * p.qp + q0 + wn * 32u + li;
#pragma unroll
  for (int r = 0; r < 16; ++r) w[(size_t)((r & 3) + 8 * (r >> 2) + 4 * (int)lh) * p.qp] = acc[r];
}

// the splits of one output summed in the order 0..S-1
__global__ __launch_bounds__(256) void bckf_reduce_kernel(BckArgs p) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= p.OC * p.Q) return;
  const uint32_t oc = e / p.Q, q = e - oc * p.Q;
  const float *w = p.ws + (size_t)oc * p.qp + q;
  const size_t slab = (size_t)p.ocp * p.qp;
  float sum = 0.0f;
  for (uint32_t s = 0; s < p.S; ++s) sum += w[s * slab];
  p.filts_grad[e] = sum;
}

// ---- strided input gradient ------------------------------------------------------------------------
// Block: 4 waves, each a 32 (ic) x 32*TN (pixels of the phase) tile; K in steps of BK = 16. The filter
// taps of a step are staged in LDS as [k][32 ic] (written with 32 consecutive lanes per k row, read as
// word 32 (2 kk + h) + i: 64 distinct banks) together with the step's (oc, j, i) decomposition; the ogl
// operand is loaded straight into MFMA operand order, lanes along the phase's pixels (consecutive ox).
template <int TN>
__global__ __launch_bounds__(256) void bcki_kernel(BckArgs p) {
  constexpr int BK = 16;
  constexpr uint32_t NOTAP = 0x40000000u;  // a tap index that puts oy, ox outside any output
  __shared__ float sa[BK * 32];
  __shared__ uint32_t sk_off[BK], sk_j[BK], sk_i[BK];
  const uint32_t ry = blockIdx.z / p.sx, rx = blockIdx.z - ry * p.sx;
  const uint32_t y0 = (ry + p.sy - p.py % p.sy) % p.sy, x0 = (rx + p.sx - p.px % p.sx) % p.sx;
  const uint32_t nyp = y0 < p.H ? (p.H - 1u - y0) / p.sy + 1u : 0u, nxp = x0 < p.W ? (p.W - 1u - x0) / p.sx + 1u : 0u;
  const uint32_t npp = nyp * nxp, Np = p.B * npp;
  if (blockIdx.x * (128u * TN) >= Np) return;  // block-uniform, before any barrier
  const uint32_t nty = ry < p.KY ? (p.KY - 1u - ry) / p.sy + 1u : 0u, ntx = rx < p.KX ? (p.KX - 1u - rx) / p.sx + 1u : 0u;
  const uint32_t ntaps = nty * ntx, Kp = p.OC * ntaps;
  const uint32_t ty0 = (y0 + p.py) / p.sy, tx0 = (x0 + p.px) / p.sx;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, li = lane & 31u, lh = lane >> 5;
  const uint32_t ic0 = blockIdx.y * 32u;
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.ogl, p.ogl_bytes), rf = make_rsrc(p.filts, p.filts_bytes);
  uint32_t ty[TN], tx[TN], ob[TN];
  size_t ib[TN];
  bool valid[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const uint32_t col = blockIdx.x * (128u * TN) + wave * (32u * TN) + t * 32u + li;
    valid[t] = col < Np;
    const uint32_t img = col / npp, rem = col - img * npp, tyi = rem / nxp, txi = rem - tyi * nxp;
    ty[t] = ty0 + tyi;
    tx[t] = tx0 + txi;
    ob[t] = img * p.OC * p.OHW;
    ib[t] = ((size_t)img * p.IC * p.H + (y0 + p.sy * tyi)) * p.W + (x0 + p.sx * txi);
  }
  f32x16 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
  for (uint32_t k0 = 0; k0 < Kp; k0 += BK) {
    __syncthreads();  // the previous step's LDS reads are done
#pragma unroll
    for (int u = 0; u < BK * 32 / 256; ++u) {
      const uint32_t e = tid + 256u * u, kk = e >> 5, i = e & 31u, k = k0 + kk;
      const uint32_t oc = k / ntaps, tap = k - oc * ntaps, tj = tap / ntx, ti = tap - tj * ntx;
      const bool ok = (k < Kp) & (ic0 + i < p.IC);
      sa[e] = ld1(rf, oob_unless(ok, (((oc * p.IC + ic0 + i) * p.KY + ry + p.sy * tj) * p.KX + rx + p.sx * ti) * 4u));
      if (i == 0) {
        sk_off[kk] = oc * p.OHW;
        sk_j[kk] = k < Kp ? tj : NOTAP;
        sk_i[kk] = ti;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k2 = 0; k2 < BK / 2; ++k2) {
      const uint32_t kk = 2u * k2 + lh;
      const float a = sa[kk * 32u + li];
      const uint32_t off = sk_off[kk], tj = sk_j[kk], ti = sk_i[kk];
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const uint32_t oy = ty[t] - tj, ox = tx[t] - ti;  // below 0 wraps past OH / OW
        const bool ok = valid[t] & (oy < p.OH) & (ox < p.OW);
        const float b = ld1(ro, oob_unless(ok, (ob[t] + off + oy * p.OW + ox) * 4u));
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < TN; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t ic = ic0 + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * lh;
      if (valid[t] && ic < p.IC) p.in_grad[ib[t] + (size_t)ic * p.HW] = acc[t][r];
    }
}

// ---- bias gradient: a block per output channel; thread t adds r = t, t + 256, ... in that order, then
// a fixed tree over the 256 partial sums. ACC = double: the ref64 form. -----------------------------------
template <class ACC>
__global__ __launch_bounds__(256) void bckb_kernel(BckArgs p) {
  __shared__ ACC part[256];
  const uint32_t oc = blockIdx.x, tid = threadIdx.x;
  ACC sum = 0;
  for (uint32_t r = tid; r < p.R; r += 256u) {
    const uint32_t n = fdiv(r, p.ohw_m, p.ohw_s), pix = r - n * p.OHW;
    sum += (ACC)p.ogl[((size_t)n * p.OC + oc) * p.OHW + pix];
  }
  part[tid] = sum;
  __syncthreads();
  for (uint32_t h = 128; h > 0; h >>= 1) {
    if (tid < h) part[tid] += part[tid + h];
    __syncthreads();
  }
  if (tid == 0) p.biases_grad[oc] = (float)part[0];
}

// ---- ref64: one thread per output, double accumulation, rounded once, reference layouts ---------------
__global__ __launch_bounds__(256) void ref64_bck_in_kernel(BckArgs p) {
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (e >= (uint64_t)p.B * p.IC * p.HW) return;
  const uint32_t x = (uint32_t)(e % p.W), y = (uint32_t)((e / p.W) % p.H);
  const uint32_t ic = (uint32_t)((e / p.HW) % p.IC), n = (uint32_t)(e / ((uint64_t)p.HW * p.IC));
  double acc = 0.0;
  for (uint32_t oc = 0; oc < p.OC; ++oc)
    for (uint32_t ky = 0; ky < p.KY; ++ky) {
      const int u = (int)(y + p.py) - (int)ky;
      if (u < 0 || u % (int)p.sy || u / (int)p.sy >= (int)p.OH) continue;
      for (uint32_t kx = 0; kx < p.KX; ++kx) {
        const int v = (int)(x + p.px) - (int)kx;
        if (v < 0 || v % (int)p.sx || v / (int)p.sx >= (int)p.OW) continue;
        acc += (double)p.ogl[((uint64_t)n * p.OC + oc) * p.OHW + (uint32_t)(u / (int)p.sy) * p.OW + (uint32_t)(v / (int)p.sx)] *
               (double)p.filts[(((uint64_t)oc * p.IC + ic) * p.KY + ky) * p.KX + kx];
      }
    }
  p.in_grad[e] = (float)acc;
}

__global__ __launch_bounds__(256) void ref64_bck_filts_kernel(BckArgs p) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= p.OC * p.Q) return;
  const uint32_t kx = e % p.KX, ky = (e / p.KX) % p.KY, ic = (e / p.KYX) % p.IC, oc = e / p.Q;
  double acc = 0.0;
  for (uint32_t n = 0; n < p.B; ++n)
    for (uint32_t oy = 0; oy < p.OH; ++oy) {
      const int iy = (int)(oy * p.sy + ky) - (int)p.py;
      if (iy < 0 || iy >= (int)p.H) continue;
      for (uint32_t ox = 0; ox < p.OW; ++ox) {
        const int ix = (int)(ox * p.sx + kx) - (int)p.px;
        if (ix < 0 || ix >= (int)p.W) continue;
        acc += (double)p.ogl[((uint64_t)n * p.OC + oc) * p.OHW + oy * p.OW + ox] *
               (double)p.in[((uint64_t)n * p.IC + ic) * p.HW + (uint32_t)iy * p.W + (uint32_t)ix];
      }
    }
  p.filts_grad[e] = (float)acc;
}

// ---- the head of the bck pack: wt[ic][oc][KY-1-ky][KX-1-kx] = filts[oc][ic][ky][kx] -------------------
__global__ __launch_bounds__(256) void xflip_kernel(const float *w, float *wt, uint32_t OC, uint32_t IC, uint32_t KY,
                                                    uint32_t KX) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x, KYX = KY * KX;
  if (e >= OC * IC * KYX) return;
  const uint32_t kx = e % KX, ky = (e / KX) % KY, oc = (e / KYX) % OC, ic = e / (KYX * OC);
  wt[e] = w[((oc * IC + ic) * KY + (KY - 1u - ky)) * KX + (KX - 1u - kx)];
}

// configurations (bh_tune_cfg_name / bh_tune_set of op 2 and op 3); the last of each is ref64
const char *const BCKI_NAMES[] = {"32x128", "32x256", "ref64"};
const char *const BCKF_NAMES[] = {"32x32", "64x64", "ref64"};
constexpr int NBCK = 3, BCK_REF64 = 2;

struct bck_dims {
  uint32_t B, IC, H, W, OC, KY, KX, sy, sx, py, px, OH, OW;
  explicit bck_dims(const uint32_t *d)
      : B(d[0]), IC(d[1]), H(d[2]), W(d[3]), OC(d[4]), KY(d[5]), KX(d[6]), sy(d[7]), sx(d[8]), py(d[9]), px(d[10]),
        OH((d[2] + 2 * d[9] - d[5]) / d[7] + 1), OW((d[3] + 2 * d[10] - d[6]) / d[8] + 1) {}
  // the input gradient is a forward conv of out_grad
  bool fwd_route() const { return sy == 1 && sx == 1 && py <= KY - 1 && px <= KX - 1; }
  void twin(uint32_t *t) const {
    const uint32_t v[11] = {B, OC, OH, OW, IC, KY, KX, 1, 1, KY - 1 - py, KX - 1 - px};
    std::copy(v, v + 11, t);
  }
};

// op 2: the wider pixel tile once a phase holds a whole one
int bcki_cfg(bh_ctx *ctx, const bck_dims &s) {
  if (ctx && ctx->bck_cfg[0] >= 0) return ctx->bck_cfg[0];
  const uint64_t npp = (uint64_t)s.B * ((s.H + s.sy - 1) / s.sy) * ((s.W + s.sx - 1) / s.sx);
  return npp >= 256 ? 1 : 0;
}
// op 3: 64 x 64 tiles when both extents of the output exceed one MFMA tile
int bckf_cfg(bh_ctx *ctx, const bck_dims &s) {
  if (ctx && ctx->bck_cfg[1] >= 0) return ctx->bck_cfg[1];
  return (s.OC > 32 && (uint64_t)s.IC * s.KY * s.KX > 32) ? 1 : 0;
}
// splits of the filter gradient's reduction: blocks for twice the CUs, at least two 64-deep chunks each
uint32_t bckf_splits(bh_ctx *ctx, const bck_dims &s, int cfg, uint32_t &cps) {
  const uint32_t bm = cfg ? 64 : 32;
  const uint64_t Q = (uint64_t)s.IC * s.KY * s.KX, R = (uint64_t)s.B * s.OH * s.OW;
  const uint64_t tiles = ((s.OC + bm - 1) / bm) * ((Q + bm - 1) / bm);
  const uint32_t nch = (uint32_t)((R + 63) / 64), ncu = ctx ? bh::num_cus(ctx) : 256u;
  uint32_t S = ctx && ctx->bck_splits[1] > 0 ? (uint32_t)ctx->bck_splits[1]
                                             : (uint32_t)std::min<uint64_t>((2ull * ncu + tiles - 1) / tiles, 64);
  if (!(ctx && ctx->bck_splits[1] > 0)) S = std::min(S, std::max(1u, nch / 2));
  S = std::max(1u, std::min(S, nch));
  cps = (nch + S - 1) / S;
  return (nch + cps - 1) / cps;  // none empty
}

int launch_bias(bh_ctx *ctx, BckArgs &p, bool ref64, bool last) {
  void *args[] = {&p};
  const void *k = ref64 ? (const void *)bckb_kernel<double> : (const void *)bckb_kernel<float>;
  return bh::launch(ctx, k, dim3(p.OC), dim3(256), args, true, last, "bck_biases");
}

int launch_filts(bh_ctx *ctx, BckArgs &p, const bck_dims &s, bool last) {
  const int cfg = bckf_cfg(ctx, s);
  void *args[] = {&p};
  const uint32_t nout = (p.OC * p.Q + 255u) / 256u;
  if (cfg == BCK_REF64)
    return bh::launch(ctx, (const void *)ref64_bck_filts_kernel, dim3(nout), dim3(256), args, true, last, "bck_filts_ref64");
  const uint32_t bm = cfg ? 64 : 32, tm = (p.OC + bm - 1) / bm, tn = (p.Q + bm - 1) / bm;
  p.S = bckf_splits(ctx, s, cfg, p.cps);
  p.ocp = tm * bm;
  p.qp = tn * bm;
  if (tm > 65535 || p.S > 65535) return bh::fail(BH_UNSUP, "bck conv: filter-gradient grid too large");
  bh::scratch_t sc;
  int rc = bh::scratch(ctx, (size_t)p.S * p.ocp * p.qp * 4, 0, sc);
  if (rc != BH_OK) return rc;
  p.ws = sc.ws;
  const void *k = cfg ? (const void *)bckf_kernel<64, 64> : (const void *)bckf_kernel<32, 32>;
  rc = bh::launch(ctx, k, dim3(tn, tm, p.S), dim3(cfg ? 256 : 64), args, true, false, "bck_filts");
  if (rc != BH_OK) return rc;
  return bh::launch(ctx, (const void *)bckf_reduce_kernel, dim3(nout), dim3(256), args, false, last, "bck_filts_reduce");
}

int launch_in(bh_ctx *ctx, BckArgs &p, const bck_dims &s, const float *packed) {
  const int forced = ctx->bck_cfg[0];
  void *args[] = {&p};
  if (forced == BCK_REF64) {
    const uint64_t n = ((uint64_t)p.B * p.IC * p.HW + 255) / 256;
    return bh::launch(ctx, (const void *)ref64_bck_in_kernel, dim3((uint32_t)n), dim3(256), args, true, true, "bck_in_ref64");
  }
  if (forced < 0 && s.fwd_route()) {
    const size_t tf = ((size_t)p.OC * p.Q + 3) & ~(size_t)3;
    const float *wt = packed, *fpk = packed ? packed + tf : nullptr;
    if (!packed) {  // the transposed-flipped bank in the context's buffer; launch_conv packs it if its route reads a pack
      int rc = bh::grow_buffer(ctx, ctx->bckw, ctx->bckw_bytes, tf * 4, false, "bck filter bank");
      if (rc == BH_OK) rc = bh::launch_bck_filts_pack(ctx, p.filts, nullptr, p.OC, p.IC, p.KY, p.KX, true, false);
      if (rc != BH_OK) return rc;
      wt = (const float *)ctx->bckw;
    }
    bh::conv_call cc{p.ogl, wt, fpk, BANKS_ALL, nullptr, nullptr, p.in_grad, p.B, p.OC, p.OH, p.OW, p.IC, p.KY, p.KX,
                     1, 1, p.KY - 1 - p.py, p.KX - 1 - p.px, 0, 0};
    cc.finish();
    return bh::launch_conv(ctx, cc);
  }
  const int cfg = bcki_cfg(ctx, s);
  const uint32_t bn = cfg ? 256 : 128;
  const uint64_t npp = (uint64_t)p.B * ((p.H + p.sy - 1) / p.sy) * ((p.W + p.sx - 1) / p.sx);  // the largest phase
  const uint32_t tiles_n = (uint32_t)((npp + bn - 1) / bn), tiles_m = (p.IC + 31) / 32, phases = p.sy * p.sx;
  if (tiles_m > 65535 || phases > 65535) return bh::fail(BH_UNSUP, "bck conv: input-gradient grid too large");
  const void *k = cfg ? (const void *)bcki_kernel<2> : (const void *)bcki_kernel<1>;
  return bh::launch(ctx, k, dim3(tiles_n, tiles_m, phases), dim3(256), args, true, true, "bck_in");
}

}  // namespace
}  // namespace bhk

namespace bh {
using namespace bhk;

size_t bck_filts_packed_floats(uint32_t OC, uint32_t IC, uint32_t KY, uint32_t KX) {
  return (((size_t)OC * IC * KY * KX + 3) & ~(size_t)3) + conv_filts_packed_floats(IC, OC, KY, KX, BANKS_ALL);
}

// packed == nullptr: only the transposed-flipped bank, into the context's buffer (already grown)
int launch_bck_filts_pack(bh_ctx *ctx, const float *filts, float *packed, uint32_t OC, uint32_t IC, uint32_t KY,
                          uint32_t KX, bool first, bool last) {
  const uint64_t n = (uint64_t)OC * IC * KY * KX;
  if (!fits_buffer(n * 4)) return fail(BH_UNSUP, "bck conv: filter bank larger than 2 GiB");
  float *wt = packed ? packed : (float *)ctx->bckw;
  void *args[] = {&filts, &wt, &OC, &IC, &KY, &KX};
  int rc = launch(ctx, (const void *)xflip_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), args, first,
                  last && !packed, "bck_xflip");
  if (rc != BH_OK || !packed) return rc;
  return launch_pack_banks(ctx, wt, packed + ((n + 3) & ~(uint64_t)3), IC, OC, KY, KX, BANKS_ALL, false, last);
}

int launch_bck(bh_ctx *ctx, const float *in, const float *filts, const float *packed, const float *out_grad,
               float *in_grad, float *filts_grad, float *biases_grad, const uint32_t *d) {
  const bck_dims s(d);
  const uint64_t in_b = (uint64_t)s.B * s.IC * s.H * s.W * 4, og_b = (uint64_t)s.B * s.OC * s.OH * s.OW * 4;
  const uint64_t f_b = (uint64_t)s.OC * s.IC * s.KY * s.KX * 4;
  if (!fits_buffer(in_b) || !fits_buffer(og_b) || !fits_buffer(f_b))
    return fail(BH_UNSUP, "bck conv: a tensor of 2 GiB or more cannot be addressed through a buffer resource");
  if ((uint64_t)s.B * s.OH * s.OW >= (1u << 31) - 64) return fail(BH_UNSUP, "bck conv: reduction extent too large");
  BckArgs p{};
  p.in = in; p.filts = filts; p.ogl = out_grad;
  p.in_grad = in_grad; p.filts_grad = filts_grad; p.biases_grad = biases_grad;
  p.B = s.B; p.IC = s.IC; p.H = s.H; p.W = s.W; p.OC = s.OC; p.KY = s.KY; p.KX = s.KX;
  p.sy = s.sy; p.sx = s.sx; p.py = s.py; p.px = s.px; p.OH = s.OH; p.OW = s.OW;
  p.OHW = s.OH * s.OW; p.HW = s.H * s.W; p.KYX = s.KY * s.KX; p.Q = s.IC * p.KYX; p.R = s.B * p.OHW;
  p.in_bytes = (uint32_t)in_b; p.ogl_bytes = (uint32_t)og_b; p.filts_bytes = (uint32_t)f_b;
  set_fd(p.OHW, p.ohw_m, p.ohw_s);
  set_fd(p.OW, p.ow_m, p.ow_s);
  set_fd(p.KYX, p.kyx_m, p.kyx_s);
  set_fd(p.KX, p.kx_m, p.kx_s);
  // the input gradient goes last: the forward route's final dispatch records the call's stop event
  int rc = BH_OK;
  if (biases_grad) rc = launch_bias(ctx, p, ctx->bck_cfg[1] == BCK_REF64, !filts_grad && !in_grad);
  if (rc == BH_OK && filts_grad) rc = launch_filts(ctx, p, s, !in_grad);
  if (rc == BH_OK && in_grad) rc = launch_in(ctx, p, s, packed);
  return rc;
}

std::string bck_variant(bh_ctx *ctx, int op, const uint32_t *d) {
  for (int i = 0; i < 9; ++i)
    if (!d[i]) return "unsupported";
  if ((uint64_t)d[2] + 2ull * d[9] < d[5] || (uint64_t)d[3] + 2ull * d[10] < d[6]) return "unsupported";
  const bck_dims s(d);
  if (op == 2) {
    const int forced = ctx ? ctx->bck_cfg[0] : -1;
    if (forced == BCK_REF64) return "ref64_bck_in_double";
    if (forced < 0 && s.fwd_route()) {
      uint32_t t[11];
      s.twin(t);
      return "bck_in_fwd:" + (ctx ? conv_variant_ctx(ctx, t) : conv_variant(t));
    }
    return std::string("mfma32_bcki_") + BCKI_NAMES[bcki_cfg(ctx, s)];
  }
  const int cfg = bckf_cfg(ctx, s);
  if (cfg == BCK_REF64) return "ref64_bck_filts_double";
  uint32_t cps = 0;
  return std::string("mfma32_bckf_") + BCKF_NAMES[cfg] + "_s" + std::to_string(bckf_splits(ctx, s, cfg, cps));
}

int bck_tune_set(bh_ctx *ctx, int op, int cfg, int splits) {
  if (cfg >= NBCK) return fail(BH_UNSUP, "tune_set: no such config");
  ctx->bck_cfg[op - 2] = cfg < 0 ? -1 : cfg;
  ctx->bck_splits[op - 2] = splits < 0 ? -splits : splits;  // op 3: splits of the reduction (0: planned)
  return BH_OK;
}

int bck_tune_cfg_name(int op, int cfg, std::string &out) {
  if (cfg < 0 || cfg >= NBCK) return fail(BH_UNSUP, "no such config");
  out = op == 2 ? BCKI_NAMES[cfg] : BCKF_NAMES[cfg];
  return BH_OK;
}

}  // namespace bh
