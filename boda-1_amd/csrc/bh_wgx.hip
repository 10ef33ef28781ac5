// bh_wgx.hip -- Winograd convolutions with the transformed-domain positions split over the waves of a
// block, two waves per SIMD: F(4x4, 3x3) and F(2x2, 5x5) on 6x6 input patches, and F(2x2, 3x3) on
// 4x4 patches in the same skeleton.
//
// Why a second Winograd kernel (bh_wino.hip's wgp_kernel stays for the shapes the tuner keeps it on):
//  * wgp gives each wave all 16 positions of F(2x2, 3x3) (256 accumulator registers), so a SIMD runs
//    ONE wave, and whatever that wave issues besides its MFMAs -- the input transform, the operand
//    loads, the stage barrier, the tile epilogue -- adds to the stage time nearly serially (its
//    diagnostic builds); at 6x6 patches (36 positions) one wave cannot even hold a
//    32x32 tile of every position;
//  * here a wave owns 32 output channels x 32 tiles x PPG positions (9 of 36, or 8 of 16): 144 / 128
//    accumulators, so two waves share each SIMD and one wave's MFMAs run while the other waits or
//    transforms; the 8 waves of a block are NOG channel groups x NPG position groups, all sharing
//    the block's input strip and transformed input V;
//  * F(4x4, 3x3) computes 16 outputs from 36 products per channel pair (4x fewer MFMA flops than the
//    direct form, 1.78x fewer than F(2x2, 3x3)); F(2x2, 5x5) 4 outputs from 36 (2.78x fewer than
//    direct). Their fp32 transforms lose more precision than F(2x2, 3x3): the launcher refuses
//    IC > 512 (rel-L2 error grows ~ sqrt(IC); at 512 it is ~4e-6, within the tests' 1e-5).
//
//   U = G g G^T (filters, N x N per (oc, ic)), V = B^T d B (input patch), M = sum_ic U . V,
//   Y = A^T M A (MO x MO outputs); points 0, 1, -1, 2, -2 (and infinity) for the 6x6 forms:
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   A^T (F43) = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1], A^T (F25) = its rows 0, 1
//   with the last column of row 1 = 1. The pack kernel (wx_pack_kernel) makes G and G g G^T in double
//   and rounds once.
//
// Structure (one fused kernel, nothing of U, V or M goes to HBM; a unit is OCT = 32 NOG output
// channels x TT = 32 Winograd tiles of the flattened (image, tile row, tile column) space; one block
// per unit, or -- the wx*k configurations -- a resident stream-K grid dealing the (unit, stage)
// iterations, a unit cut between blocks summed after the output transform by its last arriver):
//  * U (the pack, untimed like Boda's xpose_filts, src/rtc_prof.cc:93-99) goes from L2 straight into
//    registers, one stage ahead, group by group after the MFMAs that freed the registers;
//  * the stage's input strip [4 channels][RIN virtual rows][WPM] (rows img*VH + iy + pad, columns
//    x + pad: a patch of tile column tx starts at column MO*tx) arrives by dword LDS-DMA, misses
//    for the padding, so the zeros are exact and no masks are needed; two strip slots: stage it+2's
//    strip is issued at the top of stage it;
//  * stage it+1's patches are transformed during stage it into the other V buffer by the 256
//    threads of waves 0-3 (two per patch, wave-uniform halves: each half makes 3 (2) columns
//    (rows) of V from the whole patch); V [NPG][4][TT][PS], a position group's PPG values contiguous
//    per (channel, tile), pitch PS (conflict-free 16-B reads for 8 consecutive lanes);
//  * at the end of the unit the accumulators go through LDS in rounds: every (channel, tile) pair's
//    P values meet in one thread, which applies A^T M A, bias, residual and ReLU and stores.
#include "bh_gemm_dev.h"

namespace bhk {
static int launch_wgx(bh_ctx *ctx, const cfg_t &c, const bh::conv_call &cc, GemmArgs &p, const route_t &r);

struct WxArgs {
  const float *u;    // 6x6: [IC4][OC32][36], positions in (group, slot) order; 4x4: bh_wino.hip's bank
  const float *in;   // B x IC x H x W
  float *out;        // image stride OCOHW (channel slabs)
  const float *bias; // OC or null
  const float *res;  // laid out like out, or null
  uint32_t u_bytes, in_bytes, out_bytes;
  uint32_t OC, OC32, IC, B, H, W, pad, OH, OW, OHW, HW, ICHW, OCOHW;
  uint32_t TW, TPI, VH, T;    // tiles per tile row / per image, virtual rows per image, tiles in all
  uint32_t WPM, RW;           // strip pitch, RIN * WPM
  uint32_t tw_m, tw_s, tpi_m, tpi_s, vh_m, vh_s, wpm_m, wpm_s, rw_m, rw_s;
  uint32_t ngr, ngr_m, ngr_s; // tile groups (+ fastdiv)
  uint32_t ipt, ipt_m, ipt_s; // stages per unit (IC / 4) (+ fastdiv)
  uint32_t ipb, total_it;     // stream-K: iterations per block, in all
  float *ws;                  // stream-K slabs, two per block
  uint32_t *cnt;              // arrival tickets, one per unit
  int relu, wt;
  int vst;                    // OW % MO == 0 and out / res MO-float aligned: a tile row per store
  int sepc;                   // stream-K: cut units summed by wx_combine_kernel after the grid
#ifdef BH_KTRACE
  unsigned long long *trace;  // per-block device-clock marks (tools/ktrace.py)
#endif
};

namespace {

constexpr int XC = 4;    // input channels per stage (two k steps of v_mfma_f32_32x32x2_f32)
constexpr int XTT = 32;  // tiles per unit

// NW waves per block: 8 (one block per CU, two waves per SIMD) or 4 (two blocks per CU)
template <int MO, int R, int NW>
struct wx_geom {
  static constexpr int N = MO + R - 1, P = N * N, NT = 64 * NW;
  static constexpr int NPG = N == 6 ? 4 : 2, PPG = P / NPG, NOG = NW / NPG, OCT = 32 * NOG;
  static constexpr int PS = N == 6 ? 12 : 8;  // V pitch per (channel, tile): PPG values + pad
  // exchange pitch per (channel, tile) pair: NPG slots of PS, padded so that 8 consecutive pairs'
  // 16-B accesses fall on disjoint banks
  static constexpr int XS = N == 6 ? 52 : 20;
  static constexpr int ECH = NT / (NOG * 64);  // accumulator elements per exchange round
  static_assert((N == 4 || N == 6) && NOG >= 1 && NPG * NOG == NW, "4x4 or 6x6 patches, whole wave groups");
};

// position (i, j) of the N x N grid <-> (group, slot): 6x6 -- quadrants (i / 3, j / 3), slot
// (i % 3) * 3 + j % 3; 4x4 -- row pairs i / 2, slot (i % 2) * 4 + j
template <int N>
__host__ __device__ constexpr int wx_group(int i, int j) { return N == 6 ? (i / 3) * 2 + j / 3 : i / 2; }
template <int N>
__host__ __device__ constexpr int wx_slot(int i, int j) { return N == 6 ? (i % 3) * 3 + j % 3 : (i % 2) * 4 + j; }

// The 6x6 forms' interpolation points: 0, +-p, +-q, infinity with p = 2/3, q = 3/2 (not the usual
// 0, +-1, +-2). In fp32 the transformed-domain sum M = sum_ic U V dominates the error, and the output
// transform turns it into absolute error on near-zero outputs, which Boda's element metric
// (min_sig_mag_rel_diff, src/boda_base.cc:140-153) reads. tools/wino_acc.py simulates the kernel's
// arithmetic over symmetric sets {0, +-p, +-q}: error falls ~2.2x (rms) / 3-5x (max element) from
// {1, 2} to {2/3, 3/2}, on both forms. A symmetric set keeps the factored transform:
// rows +-p = (x4 - q^2 x2) +- p (x3 - q^2 x1), rows +-q likewise with p^2, 12 FMAs per 6-vector.
namespace wxp {
constexpr float P = (float)(2.0 / 3.0), P2 = (float)(4.0 / 9.0), P3 = (float)(8.0 / 27.0);
constexpr float Q = 1.5f, Q2 = 2.25f, Q3 = 3.375f;
constexpr float S = (float)(97.0 / 36.0);  // p^2 + q^2 (p^2 q^2 = 1)
}  // namespace wxp

// 6-point transform B^T x: outputs o0 .. o0 + 2 (o0 = 0 or 3)
template <int O0>
__device__ __forceinline__ void bt6_half(const float (&x)[6], float (&t)[3]) {
  using namespace wxp;
  if constexpr (O0 == 0) {
    const float u = fmaf(-Q2, x[2], x[4]), v = fmaf(-Q2, x[1], x[3]);
    t[0] = fmaf(-S, x[2], x[0] + x[4]);
    t[1] = fmaf(P, v, u);
    t[2] = fmaf(-P, v, u);
  } else {
    const float u = fmaf(-P2, x[2], x[4]), v = fmaf(-P2, x[1], x[3]);
    t[0] = fmaf(Q, v, u);
    t[1] = fmaf(-Q, v, u);
    t[2] = fmaf(-S, x[3], x[1] + x[5]);
  }
}
__device__ __forceinline__ void bt6(const float (&x)[6], float (&t)[6]) {
  float a[3], b[3];
  bt6_half<0>(x, a);
  bt6_half<3>(x, b);
  t[0] = a[0], t[1] = a[1], t[2] = a[2], t[3] = b[0], t[4] = b[1], t[5] = b[2];
}
// A^T x: F(4,3) rows (6 -> 4), F(2,5) rows (6 -> 2) over the points above; F(2,3) rows (4 -> 2)
template <int MO, int N>
__device__ __forceinline__ void at_row(const float *x, float *y) {
  if constexpr (N == 6) {
    using namespace wxp;
    const float s1 = x[1] + x[2], d1 = x[1] - x[2], s2 = x[3] + x[4], d2 = x[3] - x[4];
    y[0] = x[0] + s1 + s2;
    if constexpr (MO == 4) {
      y[1] = fmaf(Q, d2, P * d1);
      y[2] = fmaf(Q2, s2, P2 * s1);
      y[3] = fmaf(Q3, d2, P3 * d1) + x[5];
    } else {
      y[1] = fmaf(Q, d2, P * d1) + x[5];
    }
  } else {
    y[0] = x[0] + x[1] + x[2];
    y[1] = x[1] - x[2] - x[3];
  }
}

// DBG (diagnostic builds in the instrumented library only; wrong results by design): bit 0 = no input
// transform in the stage loop, 1 = no MFMA, 2 = no strip DMA, 3 = no U loads, 4 = no V fragment
// loads, 5 = no stage barrier
// SK = 0: one block per unit (whole units); SK = 1: a persistent stream-K grid dealing the (unit, stage)
// iterations equally between the blocks; a unit cut between blocks is summed after the output
// transform (linear) by its last-arriving block in block order (bitwise reproducible)
// SK = 2: whole units in full rounds of resident blocks, the last partial round's units split into S
// pieces along the stages (the same slab hand-off), so the tail runs S times shorter; SK = 3: the
// tail units split by channel group instead (NOG pieces, each a whole unit's stages for 32 output
// channels: no partial sums, one MFMA-issuing wave per SIMD)
template <int MO, int R, int SP, int NW, int SK, int DBG = 0>
__global__ __launch_bounds__(64 * NW, 2) void wgx_kernel(WxArgs p) {
  using G = wx_geom<MO, R, NW>;
  constexpr int N = G::N, P = G::P, NPG = G::NPG, PPG = G::PPG, NOG = G::NOG, OCT = G::OCT, PS = G::PS;
  constexpr int XNT = G::NT;
  constexpr int SCAP = SP * XNT;                // strip floats per slot
  constexpr int VSZ = NPG * XC * XTT * PS;      // floats of one V buffer
  constexpr int NLU = N == 6 ? 3 : 2;           // U loads per lane and k step (9 floats: 4 + 4 + 1; 8: 4 + 4)
  constexpr int ECH = G::ECH, XS = G::XS, NR = 16 / ECH, MM = MO * MO;
  constexpr int FLAG = (2 * SCAP + 2 * VSZ > XNT * XS ? 2 * SCAP + 2 * VSZ : XNT * XS);  // LDS word: last arriver
  static_assert(SP >= 1 && SP + 2 * NLU <= 63, "vmcnt range");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *const vbase = smem + 2 * SCAP;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pg = wave % NPG, og = wave / NPG;
  KT(0);
  const int li = lane & 31, kh = lane >> 5;
  // (SK 2: the hardware's dispatch order itself -- the whole units go out first, spread over all
  // XCDs, and the tail pieces fill the CUs as they free; the XCD-contiguous remap would hand some XCDs
  // only whole units and others only pieces)
  // (each XCD a contiguous run of units: the same OC tiles' U slices in its L2)
  const uint32_t lb = SK >= 2 ? blockIdx.x : xcd_contig(blockIdx.x, gridDim.x);
  // SK 3: a tail piece computes only channel group `piece` of its unit (the other waves transform,
  // load and synchronise as usual but issue no MFMA and no U load, and store nothing)
  const int piece = (SK == 3 && lb >= p.ipb) ? (int)((lb - p.ipb) % p.total_it) : -1;
  const bool active = piece < 0 || og == piece;  // wave-uniform
  const uint32_t ipt = p.ipt;
  // this block's iterations: SK -- [lb * ipb, + ipb); else unit lb. OC tile slowest in the unit order:
  // an XCD's run of units shares few OC tiles' U slices
  const uint32_t it0 = SK == 1 ? lb * p.ipb : lb * ipt;
  const uint32_t it1 = SK == 1 ? min(p.total_it, it0 + p.ipb) : it0 + ipt;

  auto tpos = [&](uint32_t tg, uint32_t &v, uint32_t &x) {  // virtual row, strip column of tile tg's patch
    const uint32_t img = fdiv(tg, p.tpi_m, p.tpi_s), rem = tg - img * p.TPI;
    const uint32_t ty = fdiv(rem, p.tw_m, p.tw_s), tx = rem - ty * p.TW;
    v = img * p.VH + MO * ty;
    x = MO * tx;
  };

  const __amdgpu_buffer_rsrc_t rsi = make_rsrc(p.in, p.in_bytes);
  const __amdgpu_buffer_rsrc_t rsu = make_rsrc(p.u, p.u_bytes);

  // ---- per-unit state (setup_unit): the unit's OC tile and tile group, the strip DMA plan (per
  // lane: element f = j * NT + tid of the [4][RIN][WPM] image; the stage's first channel enters as
  // the scalar soffset), the U offsets, the patch offset; sb = the end of the stages run now
  uint32_t oc0 = 0, g0 = 0, sb = 0, xoff = 0;
  uint32_t svo[SP];
  uint32_t uoff[2][NLU];
  const uint32_t xpatch = (uint32_t)tid & 127u, xh = __builtin_amdgcn_readfirstlane((uint32_t)tid >> 7);
  const uint32_t xc = xpatch / XTT, xtt = xpatch % XTT;
  auto setup_unit = [&](uint32_t t) {
    const uint32_t oct = fdiv(t, p.ngr_m, p.ngr_s);
    oc0 = oct * OCT;
    g0 = (t - oct * p.ngr) * XTT;
    uint32_t v0, x0u;
    tpos(g0, v0, x0u);
#pragma unroll
    for (int j = 0; j < SP; ++j) {
      const uint32_t f = (uint32_t)(j * XNT + tid);
      const uint32_t c = fdiv(f, p.rw_m, p.rw_s), rr = f - c * p.RW;
      const uint32_t s = fdiv(rr, p.wpm_m, p.wpm_s), col = rr - s * p.WPM;
      const uint32_t v = v0 + s;
      const uint32_t img = fdiv(v, p.vh_m, p.vh_s);
      const uint32_t iy = v - img * p.VH - p.pad;  // wraps (misses) in the top padding
      const uint32_t ix = col - p.pad;             // wraps (misses) in the left padding
      const bool ok = (c < (uint32_t)XC) & (ix < p.W) & (iy < p.H) & (img < p.B);
      svo[j] = oob_unless(ok, (img * p.ICHW + c * p.HW + iy * p.W + ix) * 4u);
    }
    // U of stage it: lane (li, kh) holds (input channel 4 it + 2 s + kh, output channel oc0 + 32 og +
    // li), this wave's PPG positions
    const uint32_t ocl = oc0 + (uint32_t)(32 * og + li);
    const uint32_t rot = (ocl >> 2) & 3u;  // 4x4 bank: chunk x (row i) at ((x + rot) & 3) * 4
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint32_t row = (uint32_t)(2 * s + kh) * p.OC32 + ocl;
      if constexpr (N == 6) {
        const uint32_t b = (row * 36u + (uint32_t)(PPG * pg)) * 4u;
        uoff[s][0] = oob_unless(ocl < p.OC32, b);
        uoff[s][1] = oob_unless(ocl < p.OC32, b + 16u);
        uoff[s][2] = oob_unless(ocl < p.OC32, b + 32u);
      } else {
#pragma unroll
        for (int x = 0; x < 2; ++x)
          uoff[s][x] = oob_unless(ocl < p.OC32, (row * 16u + ((2u * pg + x + rot) & 3u) * 4u) * 4u);
      }
    }
    xoff = 0;  // float offset of this thread's patch in a strip slot
    const uint32_t tg = g0 + xtt;
    if (tg < p.T) {
      uint32_t v, x;
      tpos(tg, v, x);
      xoff = xc * p.RW + (v - v0) * p.WPM + x;
    }
  };
  auto issue_strip = [&](int slot, uint32_t it) {  // stage it's strip (dead past the run: no memory touched)
    // Everything here is scalar: a dead stage reads through a descriptor with no records (selecting
    // between two descriptor variables instead put both in scratch and reloaded one per stage; a
    // per-lane miss mask cost one VALU op per DMA), and the LDS destination is the wave's base (a
    // per-lane address costs a VALU add and a readfirstlane per DMA)
    const bool live = it < sb;
    const uint32_t ss = live ? it * XC * p.HW * 4u : 0u;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.in, live ? p.in_bytes : 0u);
#pragma unroll
    for (int j = 0; j < SP; ++j) dma4s(rs, smem + slot * SCAP + j * XNT + wave * 64, svo[j], ss);
  };
  float ur[2][PPG];
  auto load_u = [&](int s, uint32_t it) {
    const uint32_t su = (it < sb && active) ? it * (uint32_t)XC * p.OC32 * (uint32_t)(P * 4) : 0x7fffff00u;  // dead: misses
    const f32x4v a = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rsu, uoff[s][0], su, 0));
    const f32x4v b = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rsu, uoff[s][1], su, 0));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ur[s][e] = a[e];
      ur[s][4 + e] = b[e];
    }
    if constexpr (N == 6) ur[s][8] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsu, uoff[s][2], su, 0));
  };

  // ---- V fragments of k step s from buffer vb: (channel 2 s + kh, tile li), this group's slots
  float vf[2][PPG];
  auto load_vf = [&](int vb, int s) {
    const float *const src = vbase + vb * VSZ + ((pg * XC + 2 * s + kh) * XTT + li) * PS;
    const f32x4v a = *(const f32x4v *)src, b = *(const f32x4v *)(src + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      vf[s][e] = a[e];
      vf[s][4 + e] = b[e];
    }
    if constexpr (N == 6) vf[s][8] = src[8];
  };

  // ---- input transform (threads 0..255: patch tid % 128 = (channel, tile), half tid / 128), in
  // three phases, so that the patch reads land under MFMAs instead of in front of them: tx_read(h)
  // reads patch rows 3h .. 3h + 2 (4x4: all four rows at h = 0), tx_e(h) makes their E = d B values,
  // tx_v makes V = B^T E from the whole E and writes it (NW = 8 leaves waves 4..7 without patches;
  // the callers test xf, which is wave-uniform)
  const bool xf = wave < 4;  // (uniform: a branch, not an exec mask)
  constexpr int NRD = N == 6 ? 3 : 4, NCE = N == 6 ? 3 : 4;
  float dr[NRD][N];
  float e[N][NCE];
  auto tx_read = [&](int slot, int h) {
    const float *const s = smem + slot * SCAP + xoff + (uint32_t)(h * NRD) * p.WPM;
#pragma unroll
    for (int r = 0; r < NRD; ++r) {
      if constexpr (N == 6 && MO == 4) {  // patch starts at a multiple of 4 floats
        const f32x4v a = *(const f32x4v *)(s + r * p.WPM);
        const f32x2v b = *(const f32x2v *)(s + r * p.WPM + 4);
        dr[r][0] = a[0]; dr[r][1] = a[1]; dr[r][2] = a[2]; dr[r][3] = a[3]; dr[r][4] = b[0]; dr[r][5] = b[1];
      } else {  // multiple of 2
#pragma unroll
        for (int q = 0; q < N / 2; ++q) {
          const f32x2v a = *(const f32x2v *)(s + r * p.WPM + 2 * q);
          dr[r][2 * q] = a[0];
          dr[r][2 * q + 1] = a[1];
        }
      }
    }
  };
  auto tx_e = [&](int h) {
#pragma unroll
    for (int r = 0; r < NRD; ++r) {
      if constexpr (N == 6) {
        if (xh) bt6_half<3>(dr[r], e[h * NRD + r]);
        else bt6_half<0>(dr[r], e[h * NRD + r]);
      } else {  // E[r] = B^T d_r: (d0 - d2, d1 + d2, d2 - d1, d1 - d3)
        e[r][0] = dr[r][0] - dr[r][2];
        e[r][1] = dr[r][1] + dr[r][2];
        e[r][2] = dr[r][2] - dr[r][1];
        e[r][3] = dr[r][1] - dr[r][3];
      }
    }
  };
  auto tx_v = [&](int vb) {
    float *const vd = vbase + vb * VSZ + (xc * XTT + xtt) * PS;
    if constexpr (N == 6) {
      // this half's three columns c = 3 xh + c' of E; V[i][c] = (B^T E[:, c])[i]; groups (gi, xh),
      // slot (i % 3) * 3 + c'
      float vcol[3][6];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float col[6] = {e[0][c], e[1][c], e[2][c], e[3][c], e[4][c], e[5][c]};
        bt6(col, vcol[c]);
      }
#pragma unroll
      for (int gi = 0; gi < 2; ++gi) {
        float *const dst = vd + (size_t)(2 * gi) * XC * XTT * PS + xh * XC * XTT * PS;
        float w[9];
#pragma unroll
        for (int il = 0; il < 3; ++il)
#pragma unroll
          for (int c = 0; c < 3; ++c) w[il * 3 + c] = vcol[c][3 * gi + il];
        *(f32x4v *)dst = f32x4v{w[0], w[1], w[2], w[3]};
        *(f32x4v *)(dst + 4) = f32x4v{w[4], w[5], w[6], w[7]};
        dst[8] = w[8];
      }
    } else {
      // F(2x2, 3x3): V rows 2 xh, 2 xh + 1 (group xh)
      float w[8];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (xh) {
          w[c] = e[2][c] - e[1][c];
          w[4 + c] = e[1][c] - e[3][c];
        } else {
          w[c] = e[0][c] - e[2][c];
          w[4 + c] = e[1][c] + e[2][c];
        }
      }
      float *const dst = vd + xh * XC * XTT * PS;
      *(f32x4v *)dst = f32x4v{w[0], w[1], w[2], w[3]};
      *(f32x4v *)(dst + 4) = f32x4v{w[4], w[5], w[6], w[7]};
    }
  };
  auto transform = [&](int slot, int vb) {  // all phases at once (the prologue)
    if (!xf) return;
    tx_read(slot, 0);
    tx_e(0);
    if constexpr (N == 6) {
      tx_read(slot, 1);
      tx_e(1);
    }
    tx_v(vb);
  };

  // ---- epilogue pieces: pair (og, e, lane) of an exchange round meets its P values in thread
  // pair = (og * ECH + e_local) * 64 + lane; store_y adds bias, residual and ReLU and stores
  float *const xb = smem;
  const __amdgpu_buffer_rsrc_t rso = make_rsrc(p.out, p.out_bytes);
  const __amdgpu_buffer_rsrc_t rsr = make_rsrc(p.res, p.res ? p.out_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rsb = make_rsrc(p.bias, p.bias ? p.OC * 4u : 0u);
  const uint32_t rog = (uint32_t)tid / (ECH * 64), rel = ((uint32_t)tid / 64) % ECH, rlane = (uint32_t)tid & 63u;
  auto store_y = [&](int r, const float (&y)[MO][MO], float bb, bool tvalid, uint32_t obase, uint32_t oy0,
                     uint32_t ox0) {
    const uint32_t ee = (uint32_t)(r * ECH) + rel;
    const uint32_t oc = oc0 + rog * 32u + 8u * (ee >> 2) + 4u * (rlane >> 5) + (ee & 3u);
    const bool ok = tvalid & (oc < p.OC) & (piece < 0 || rog == (uint32_t)piece);
    const uint32_t ob = obase + oc * p.OHW;
#pragma unroll
    for (int yy = 0; yy < MO; ++yy) {
      if (p.vst) {  // uniform: OW % MO == 0 and MO-float aligned tensors -- a tile row is one store
        typedef __attribute__((ext_vector_type(MO))) uint32_t uv_t;
        const uint32_t off = oob_unless(ok & (oy0 + yy < p.OH), (ob + yy * p.OW) * 4u);
        float z[MO];
        // (whole-vector bit casts only: hipcc miscompiles a bit cast of one vector component,
        // DESIGN.md §3.11)
        typedef __attribute__((ext_vector_type(MO))) float fv_t;
        fv_t rv = {};
        if (p.res) {
          if constexpr (MO == 4) rv = __builtin_bit_cast(fv_t, __builtin_amdgcn_raw_buffer_load_b128(rsr, off, 0, 0));
          else rv = __builtin_bit_cast(fv_t, __builtin_amdgcn_raw_buffer_load_b64(rsr, off, 0, 0));
        }
        fv_t zv;
#pragma unroll
        for (int x = 0; x < MO; ++x) {
          z[x] = y[yy][x] + bb;
          if (p.res) z[x] += rv[x];
          z[x] = (p.relu && z[x] < 0.0f) ? 0.0f : z[x];
          zv[x] = z[x];
        }
        const uv_t v = __builtin_bit_cast(uv_t, zv);
        if constexpr (MO == 4) {
          if (p.wt) __builtin_amdgcn_raw_buffer_store_b128(v, rso, off, 0, AUX_SC1);
          else __builtin_amdgcn_raw_buffer_store_b128(v, rso, off, 0, AUX_OUT);
        } else {
          if (p.wt) __builtin_amdgcn_raw_buffer_store_b64(v, rso, off, 0, AUX_SC1);
          else __builtin_amdgcn_raw_buffer_store_b64(v, rso, off, 0, AUX_OUT);
        }
        continue;
      }
#pragma unroll
      for (int x = 0; x < MO; ++x) {
        const bool in = ok & (oy0 + yy < p.OH) & (ox0 + x < p.OW);
        const uint32_t off = oob_unless(in, (ob + yy * p.OW + x) * 4u);
        float z = y[yy][x] + bb;
        if (p.res) z += ld1(rsr, off);
        z = (p.relu && z < 0.0f) ? 0.0f : z;
        if (p.wt) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, z), rso, off, 0, AUX_SC1);
        else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, z), rso, off, 0, AUX_OUT);
      }
    }
  };

  f32x16 acc[PPG];
  const uint32_t tfirst = fdiv(it0, p.ipt_m, p.ipt_s);  // the block's first unit (slab slot 0)
  // one run: stages sa .. sb - 1 of unit t (SK = 0: the whole unit, once)
  auto run = [&](uint32_t t, uint32_t sa, bool first_run) {
    setup_unit(t);
#pragma unroll
    for (int q = 0; q < PPG; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;

    // ---- prologue: strips of stages sa and sa + 1, then U(sa) (still in flight while V(sa) is made:
    // the loop's first waits count on exactly the steady state's [strip][U k0][U k1] order)
    issue_strip(0, sa);
    issue_strip(1, sa + 1);
    load_u(0, sa);
    load_u(1, sa);
    vm_wait<2 * NLU>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // (also: every wave past the previous run's last LDS reads)
    asm volatile("" ::: "memory");
    transform(0, 0);
    if (first_run) KT(1);

    // per stage and lane, VMEM in issue order: strip(it + 2) (SP DMAs) right after the barrier, then
    // U(it + 1) k step 0 (NLU loads) after the k-step-0 MFMAs, U(it + 1) k step 1 (NLU) at the end.
    // Top of stage it: strip(it + 1) must have landed -> vmcnt(2 NLU); before k step 0's MFMAs U(it)
    // step 0 -> vmcnt(NLU + SP); before k step 1's, U(it) step 1 -> vmcnt(SP + NLU)
    for (uint32_t s = sa; s < sb; ++s) {
      const int vb = (int)((s - sa) & 1u);
      vm_wait<2 * NLU>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if constexpr ((DBG & 32) == 0) __builtin_amdgcn_s_barrier();  // V(s) written, strip(s + 1) landed, strip(s)'s slot free
      asm volatile("" ::: "memory");
      if constexpr ((DBG & 4) == 0) issue_strip(vb, s + 2);
      else if constexpr ((DBG & 64) == 0) issue_strip(vb, sb);  // dead: the same VMEM count, no memory touched
      if constexpr ((DBG & 16) == 0) {
        load_vf(vb, 0);
        load_vf(vb, 1);
      }
      // strip(s + 1) -> V(s + 1) in three phases around the MFMA groups (its reads land under them)
      constexpr bool XF = (DBG & 1) == 0;
      if (XF && xf) tx_read(vb ^ 1, 0);
      __builtin_amdgcn_sched_barrier(0);
      vm_wait<NLU + SP>();
#pragma unroll
      for (int q = 0; q < PPG; ++q) {
        if constexpr ((DBG & 2) == 0) {
          if (SK != 3 || active) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ur[0][q], vf[0][q], acc[q], 0, 0, 0);
        }
        else asm volatile("" ::"v"(ur[0][q]), "v"(vf[0][q]));
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr ((DBG & 8) == 0) load_u(0, s + 1);
      else if constexpr ((DBG & 128) == 0) load_u(0, sb);  // dead loads (misses): the same VMEM count
      if (XF && xf) {
        tx_e(0);
        if constexpr (N == 6) tx_read(vb ^ 1, 1);
      }
      __builtin_amdgcn_sched_barrier(0);
      vm_wait<SP + NLU>();
#pragma unroll
      for (int q = 0; q < PPG; ++q) {
        if constexpr ((DBG & 2) == 0) {
          if (SK != 3 || active) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ur[1][q], vf[1][q], acc[q], 0, 0, 0);
        }
        else asm volatile("" ::"v"(ur[1][q]), "v"(vf[1][q]));
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr ((DBG & 8) == 0) load_u(1, s + 1);
      else if constexpr ((DBG & 128) == 0) load_u(1, sb);
      if (XF && xf) {
        if constexpr (N == 6) tx_e(1);
        tx_v(vb ^ 1);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    vm_wait<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave done with the strips and V: the LDS is the exchange now
    asm volatile("" ::: "memory");
    if (first_run) KT(2);

    // ---- epilogue: rounds of ECH accumulator elements
    const bool whole = !SK || (sa == 0 && sb == ipt);  // uniform
    const uint32_t rtile = g0 + (rlane & 31u);
    const bool tvalid = rtile < p.T;
    // this thread's bias values of every round, loaded before the first round (one memory latency,
    // not one per round)
    float rbias[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const uint32_t ee = (uint32_t)(r * ECH) + rel;
      const uint32_t oc = oc0 + rog * 32u + 8u * (ee >> 2) + 4u * (rlane >> 5) + (ee & 3u);
      rbias[r] = ld1(rsb, oob_unless(oc < p.OC, oc * 4u));
    }
    uint32_t obase = 0, oy0 = 0, ox0 = 0;
    {
      const uint32_t tg = tvalid ? rtile : 0u;
      const uint32_t img = fdiv(tg, p.tpi_m, p.tpi_s), rem = tg - img * p.TPI;
      const uint32_t ty = fdiv(rem, p.tw_m, p.tw_s), tx = rem - ty * p.TW;
      oy0 = MO * ty;
      ox0 = MO * tx;
      obase = img * p.OCOHW + oy0 * p.OW + ox0;
    }
    // a cut unit's partial outputs (after the transform, before the bias) go to this block's slab:
    // slot 0 for its first unit, 1 for its last ([round][thread][MO x MO], write-through)
    const uint32_t sl = SK == 2 || t == tfirst ? 0u : 1u;  // (SK 2: one unit per block)
    const __amdgpu_buffer_rsrc_t rws =
        make_rsrc(p.ws + ((size_t)lb * 2 + sl) * (size_t)(NR * XNT * MM), NR * XNT * MM * 4);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int r0 = r * ECH;
      // write: this wave's PPG values of elements r0 .. r0 + ECH - 1
#pragma unroll
      for (int el = 0; el < ECH; ++el) {
        float m[PPG];
#pragma unroll
        for (int q = 0; q < PPG; ++q) m[q] = acc[q][r0 + el];
        float *const dst = xb + ((og * ECH + el) * 64 + lane) * XS + pg * PS;
        *(f32x4v *)dst = f32x4v{m[0], m[1], m[2], m[3]};
        *(f32x4v *)(dst + 4) = f32x4v{m[4], m[5], m[6], m[7]};
        if constexpr (N == 6) dst[8] = m[8];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // read: the pair's N x N values, A^T M A, then store (or the partial to the slab)
      {
        float mm[N][N];
        const float *const src = xb + (size_t)tid * XS;
#pragma unroll
        for (int g = 0; g < NPG; ++g) {
          float m[PPG];
          const f32x4v a = *(const f32x4v *)(src + g * PS), b = *(const f32x4v *)(src + g * PS + 4);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            m[q] = a[q];
            m[4 + q] = b[q];
          }
          if constexpr (N == 6) m[8] = src[g * PS + 8];
#pragma unroll
          for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j)
              if (wx_group<N>(i, j) == g) mm[i][j] = m[wx_slot<N>(i, j)];
        }
        float tt[N][MO];  // T = M A (each row of M through A^T)
#pragma unroll
        for (int i = 0; i < N; ++i) at_row<MO, N>(mm[i], tt[i]);
        float y[MO][MO];  // Y = A^T T (each column of T)
#pragma unroll
        for (int x = 0; x < MO; ++x) {
          float col[N], o[MO];
#pragma unroll
          for (int i = 0; i < N; ++i) col[i] = tt[i][x];
          at_row<MO, N>(col, o);
#pragma unroll
          for (int yy = 0; yy < MO; ++yy) y[yy][x] = o[yy];
        }
        if (whole) {
          store_y(r, y, rbias[r], tvalid, obase, oy0, ox0);
        } else if constexpr (SK) {
#pragma unroll
          for (int q = 0; q < MM; q += 4) {
            const f32x4v v = {y[q / MO][q % MO], y[(q + 1) / MO][(q + 1) % MO], y[(q + 2) / MO][(q + 2) % MO],
                              y[(q + 3) / MO][(q + 3) % MO]};
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) uint32_t, v),
                                                   rws, (uint32_t)(((r * XNT + tid) * MM + q) * 4), 0, AUX_SC1);
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every reader done before the next round's writes
      asm volatile("" ::: "memory");
    }
    if constexpr (SK) {
      if (!whole && !(SK == 1 && p.sepc)) {  // (sepc: summed by wx_combine_kernel)
        // the unit's blocks b0 .. b1 (in block order); the last to arrive sums their partials
        // (SK 2: tail unit t's S = total_it parts are blocks ipb + (t - ipb) S ..)
        const uint32_t b0 = SK == 2 ? p.ipb + (t - p.ipb) * p.total_it : (t * ipt) / p.ipb;
        const uint32_t b1 = SK == 2 ? b0 + p.total_it - 1u : (t * ipt + ipt - 1) / p.ipb;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        uint32_t *const flag = (uint32_t *)(smem + FLAG);
        if (tid == 0) {
          const uint32_t old = __hip_atomic_fetch_add(&p.cnt[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint32_t last = old == b1 - b0 ? 1u : 0u;
          if (last) __hip_atomic_store(&p.cnt[t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          *flag = last;
        }
        __syncthreads();
        if (*flag) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler-only: keep the loads below the ticket
          const __amdgpu_buffer_rsrc_t rall = make_rsrc(p.ws, 0x7fffff00u);
          float ys[NR][MM];
#pragma unroll
          for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int q = 0; q < MM; ++q) ys[r][q] = 0.0f;
          for (uint32_t b = b0; b <= b1; ++b) {  // block order = k order: bitwise reproducible
            const uint32_t s2 = (SK == 1 && b == b0 && t != fdiv(b * p.ipb, p.ipt_m, p.ipt_s)) ? 1u : 0u;
            const uint32_t base = (b * 2 + s2) * (uint32_t)(NR * XNT * MM * 4);
            f32x4v x[NR][MM / 4];
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
              for (int q = 0; q < MM / 4; ++q)
                x[r][q] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(
                                                         rall, base + (uint32_t)(((r * XNT + tid) * MM + 4 * q) * 4), 0,
                                                         AUX_SC1));
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
              for (int q = 0; q < MM / 4; ++q)
#pragma unroll
                for (int c = 0; c < 4; ++c) ys[r][4 * q + c] += x[r][q][c];
          }
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            float y[MO][MO];
#pragma unroll
            for (int q = 0; q < MM; ++q) y[q / MO][q % MO] = ys[r][q];
            store_y(r, y, rbias[r], tvalid, obase, oy0, ox0);
          }
        }
      }
    }
  };
  if constexpr (SK == 3) {
    // whole units in full rounds; a tail unit as total_it (= NOG) pieces, one channel group each
    sb = ipt;
    run(lb < p.ipb ? lb : p.ipb + (lb - p.ipb) / p.total_it, 0u, true);
  } else if constexpr (SK == 2) {
    // data-parallel rounds + a split tail: blocks below ipb take their unit whole; the rest take
    // part j of S = total_it of a tail unit (stages [j ipt / S, (j + 1) ipt / S)), so the last,
    // partly filled round of units runs as S times as many shorter pieces
    if (lb < p.ipb) {
      sb = ipt;
      run(lb, 0u, true);
    } else {
      const uint32_t j = lb - p.ipb, S = p.total_it, part = j % S;
      sb = (part + 1) * ipt / S;
      run(p.ipb + j / S, part * ipt / S, true);
    }
  } else if constexpr (SK == 1) {
    bool first_run = true;
    for (uint32_t it = it0; it < it1;) {
      const uint32_t t = fdiv(it, p.ipt_m, p.ipt_s);
      sb = min(ipt, it1 - t * ipt);
      run(t, it - t * ipt, first_run);
      first_run = false;
      it = t * ipt + sb;
    }
  } else {
    sb = ipt;
    run(lb, 0u, true);
  }
  vm_wait<0>();
  KT(4);
}

// wx_combine_kernel: the cut units of a stream-K wgx grid (p.sepc, SK 1), summed after it instead of
// by their last arrivers (whose extra ~5-11 us of slab reads and stores end the grid while the
// pieces' other CUs idle, profiles/r05/ktrace_streamk_routes.log). One block per (unit, exchange
// round r), the grid's thread layout: thread tid sums element r of its (channel, tile) pair over the
// unit's slabs in block order (the last arriver's order: bitwise the same output) and stores as
// the grid's epilogue does.
template <int MO, int R, int NW>
__global__ __launch_bounds__(64 * NW) void wx_combine_kernel(WxArgs p) {
  using G = wx_geom<MO, R, NW>;
  constexpr int XNT = G::NT, OCT = G::OCT, ECH = G::ECH, NR = 16 / ECH, MM = MO * MO;
  const uint32_t t = blockIdx.x / NR, r = blockIdx.x % NR;
  const uint32_t ipt = p.ipt, b0 = (t * ipt) / p.ipb, b1 = (t * ipt + ipt - 1) / p.ipb;
  if (b0 == b1) return;  // uniform: a whole unit, stored by the grid
  const uint32_t tid = threadIdx.x;
  const uint32_t rog = tid / (ECH * 64), rel = (tid / 64) % ECH, rlane = tid & 63u;
  const uint32_t oct = fdiv(t, p.ngr_m, p.ngr_s), oc0 = oct * OCT, g0 = (t - oct * p.ngr) * XTT;
  const uint32_t rtile = g0 + (rlane & 31u);
  const bool tvalid = rtile < p.T;
  uint32_t obase, oy0, ox0;
  {
    const uint32_t tg = tvalid ? rtile : 0u;
    const uint32_t img = fdiv(tg, p.tpi_m, p.tpi_s), rem = tg - img * p.TPI;
    const uint32_t ty = fdiv(rem, p.tw_m, p.tw_s), tx = rem - ty * p.TW;
    oy0 = MO * ty;
    ox0 = MO * tx;
    obase = img * p.OCOHW + oy0 * p.OW + ox0;
  }
  const uint32_t ee = r * ECH + rel;
  const uint32_t oc = oc0 + rog * 32u + 8u * (ee >> 2) + 4u * (rlane >> 5) + (ee & 3u);
  const __amdgpu_buffer_rsrc_t rso = make_rsrc(p.out, p.out_bytes);
  const __amdgpu_buffer_rsrc_t rsr = make_rsrc(p.res, p.res ? p.out_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rsb = make_rsrc(p.bias, p.bias ? p.OC * 4u : 0u);
  const __amdgpu_buffer_rsrc_t rall = make_rsrc(p.ws, 0x7fffff00u);
  const float bb = ld1(rsb, oob_unless(oc < p.OC, oc * 4u));
  float ys[MM];
#pragma unroll
  for (int q = 0; q < MM; ++q) ys[q] = 0.0f;
  // slabs in groups of 4, all their loads in flight
  for (uint32_t bg = b0; bg <= b1; bg += 4) {
    f32x4v x[4][MM / 4];
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
      const uint32_t b = bg + (uint32_t)sb;
      const uint32_t s2 = (b == b0 && t != fdiv(b * p.ipb, p.ipt_m, p.ipt_s)) ? 1u : 0u;
      const uint32_t base = (b * 2 + s2) * (uint32_t)(NR * XNT * MM * 4);
#pragma unroll
      for (int q = 0; q < MM / 4; ++q)
        x[sb][q] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(
                                                  rall, oob_unless(b <= b1, base + ((r * XNT + tid) * MM + 4 * q) * 4), 0,
                                                  AUX_SC1));
    }
#pragma unroll
    for (int sb = 0; sb < 4; ++sb)
      if (bg + (uint32_t)sb <= b1) {  // block order = k order
#pragma unroll
        for (int q = 0; q < MM / 4; ++q)
#pragma unroll
          for (int c = 0; c < 4; ++c) ys[4 * q + c] += x[sb][q][c];
      }
  }
  const bool ok = tvalid & (oc < p.OC);
  const uint32_t ob = obase + oc * p.OHW;
#pragma unroll
  for (int yy = 0; yy < MO; ++yy) {
    if (p.vst) {  // uniform: OW % MO == 0 and MO-float aligned tensors -- a tile row is one store
      typedef __attribute__((ext_vector_type(MO))) uint32_t uv_t;
      typedef __attribute__((ext_vector_type(MO))) float fv_t;
      const uint32_t off = oob_unless(ok & (oy0 + yy < p.OH), (ob + yy * p.OW) * 4u);
      fv_t rv = {};
      if (p.res) {
        if constexpr (MO == 4) rv = __builtin_bit_cast(fv_t, __builtin_amdgcn_raw_buffer_load_b128(rsr, off, 0, 0));
        else rv = __builtin_bit_cast(fv_t, __builtin_amdgcn_raw_buffer_load_b64(rsr, off, 0, 0));
      }
      fv_t zv;
#pragma unroll
      for (int x = 0; x < MO; ++x) {
        float z = ys[yy * MO + x] + bb;
        if (p.res) z += rv[x];
        zv[x] = (p.relu && z < 0.0f) ? 0.0f : z;
      }
      const uv_t v = __builtin_bit_cast(uv_t, zv);
      if constexpr (MO == 4) {
        if (p.wt) __builtin_amdgcn_raw_buffer_store_b128(v, rso, off, 0, AUX_SC1);
        else __builtin_amdgcn_raw_buffer_store_b128(v, rso, off, 0, AUX_OUT);
      } else {
        if (p.wt) __builtin_amdgcn_raw_buffer_store_b64(v, rso, off, 0, AUX_SC1);
        else __builtin_amdgcn_raw_buffer_store_b64(v, rso, off, 0, AUX_OUT);
      }
      continue;
    }
#pragma unroll
    for (int x = 0; x < MO; ++x) {
      const bool in = ok & (oy0 + yy < p.OH) & (ox0 + x < p.OW);
      const uint32_t off = oob_unless(in, (ob + yy * p.OW + x) * 4u);
      float z = ys[yy * MO + x] + bb;
      if (p.res) z += ld1(rsr, off);
      z = (p.relu && z < 0.0f) ? 0.0f : z;
      if (p.wt) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, z), rso, off, 0, AUX_SC1);
      else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, z), rso, off, 0, AUX_OUT);
    }
  }
}

template <int MO, int R, int SP, int NW, int DBG = 0, int SK = 0>
cfg_t wgx_cfg(const char *name) {
  using G = wx_geom<MO, R, NW>;
  cfg_t c{name, G::OCT, XTT, XC, G::NT, {}, 1};
  c.k[A_KVEC][B_DIRECT][0] = (kern_t)(void *)wgx_kernel<MO, R, SP, NW, SK, DBG>;
  if constexpr (SK == 1) c.k[A_KVEC][B_DIRECT][1] = (kern_t)(void *)wx_combine_kernel<MO, R, NW>;
  c.family = F_WGX;
  c.launch = launch_wgx;
  c.ky = R;
  c.kx = R;
  c.mo = MO;
  c.bank = R == 5 ? (MO == 2 ? BANK_W25 : 0u) : (MO == 4 ? BANK_W43 : BANK_W23);
  c.sk = SK;
  c.sp = SP;
  return c;
}

// Filter transform of the 6x6 forms: u[ic][oc][(group, slot)] = G g G^T (double, rounded once)
template <int R>
__global__ __launch_bounds__(256) void wx_pack_kernel(const float *__restrict__ w, float *__restrict__ u, uint32_t OC,
                                                      uint32_t IC, uint32_t OC32, uint32_t IC4) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;  // ic * OC32 + oc
  if (e >= IC4 * OC32) return;
  const uint32_t ic = e / OC32, oc = e - ic * OC32;
  const bool ok = oc < OC && ic < IC;
  // G (6 x R) for points 0, p, -p, q, -q, infinity (wxp: p = 2/3, q = 3/2): row k =
  // (q_k^0 .. q_k^{R-1}) / prod_{l != k} (q_k - q_l)
  const double q[5] = {0.0, 2.0 / 3.0, -2.0 / 3.0, 1.5, -1.5};
  double g[6][R];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double den = 1.0;
#pragma unroll
    for (int l = 0; l < 5; ++l)
      if (l != k) den *= q[k] - q[l];
    double pw = 1.0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      g[k][j] = pw / den;
      pw *= q[k];
    }
  }
#pragma unroll
  for (int j = 0; j < R; ++j) g[5][j] = j == R - 1 ? 1.0 : 0.0;
  double f[R][R];
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int b = 0; b < R; ++b) f[a][b] = ok ? (double)w[((size_t)oc * IC + ic) * (R * R) + a * R + b] : 0.0;
  double t[6][R];  // G f
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int b = 0; b < R; ++b) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < R; ++a) s += g[i][a] * f[a][b];
      t[i][b] = s;
    }
  float *const dst = u + (size_t)e * 36;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < R; ++b) s += t[i][b] * g[j][b];
      dst[wx_group<6>(i, j) * 9 + wx_slot<6>(i, j)] = (float)s;
    }
}

}  // namespace

std::vector<cfg_t> wgx_cfgs() {
  // <MO, R, SP, NW>: output tile MO x MO, filter R x R (patch MO + R - 1), SP dword strip DMAs per
  // lane and stage (the strip [4][RIN][WPM] must fit SP * 64 NW floats), NW waves per block
  return {
      // (a dead DMA instruction costs about what a live one does: SP close to the strip's need)
      wgx_cfg<4, 3, 4, 8>("wx43s4"),   wgx_cfg<4, 3, 8, 8>("wx43s8"),   wgx_cfg<4, 3, 9, 8>("wx43s9"),
      wgx_cfg<4, 3, 10, 8>("wx43s10"), wgx_cfg<4, 3, 12, 8>("wx43s12"),
      wgx_cfg<2, 5, 3, 8>("wx25s3"),   wgx_cfg<2, 5, 4, 8>("wx25s4"),   wgx_cfg<2, 5, 5, 8>("wx25s5"),
      wgx_cfg<2, 5, 6, 8>("wx25s6"),   wgx_cfg<2, 5, 10, 8>("wx25s10"),
      wgx_cfg<2, 3, 2, 8>("wx23s2"),   wgx_cfg<2, 3, 3, 8>("wx23s3"),   wgx_cfg<2, 3, 4, 8>("wx23s4"),
      wgx_cfg<2, 3, 6, 8>("wx23s6"),   wgx_cfg<2, 3, 10, 8>("wx23s10"),
      // four waves (OC tile 32 / 64): twice the units, two blocks per CU -- the small-batch shapes
      wgx_cfg<4, 3, 8, 4>("wx43s8w4"), wgx_cfg<4, 3, 12, 4>("wx43s12w4"), wgx_cfg<4, 3, 16, 4>("wx43s16w4"),
      wgx_cfg<2, 5, 6, 4>("wx25s6w4"), wgx_cfg<2, 5, 8, 4>("wx25s8w4"), wgx_cfg<2, 5, 12, 4>("wx25s12w4"),
      wgx_cfg<2, 3, 4, 4>("wx23s4w4"), wgx_cfg<2, 3, 6, 4>("wx23s6w4"), wgx_cfg<2, 3, 8, 4>("wx23s8w4"),
      wgx_cfg<2, 3, 12, 4>("wx23s12w4"),
      // stream-K grids: a cut unit's partial outputs (MO x MO floats per channel-tile pair) go through a slab
      wgx_cfg<2, 3, 2, 8, 0, 1>("wx23s2k"), wgx_cfg<2, 3, 3, 8, 0, 1>("wx23s3k"), wgx_cfg<2, 3, 4, 8, 0, 1>("wx23s4k"),
      wgx_cfg<2, 3, 6, 8, 0, 1>("wx23s6k"),
      wgx_cfg<2, 3, 4, 4, 0, 1>("wx23s4w4k"), wgx_cfg<2, 3, 6, 4, 0, 1>("wx23s6w4k"), wgx_cfg<2, 3, 8, 4, 0, 1>("wx23s8w4k"),
      // (F(4x4, 3x3) stream-K forms, measured and not kept: ~45 VGPRs spilled outside the stage loop,
      // 98 against 81 us on 20x64x56^2->192)
      // whole units + a split tail round (SK 2). Measured: 1x96x63^2->256 5x5 37.4 -> 33.1 us, the
      // batch-20 5x5 ops -1 %; F(4x4, 3x3) 20x64x56^2->192 80 -> 100 us (a tail piece writes and the
      // last arriver reads a whole 16-float-per-pair partial output through the write-through slab),
      // F(2x2, 3x3) no gain: those forms are not built
      wgx_cfg<2, 5, 4, 8, 0, 2>("wx25s4t"), wgx_cfg<2, 5, 6, 8, 0, 2>("wx25s6t"),
      // whole units + a tail split by channel group (SK 3)
      wgx_cfg<4, 3, 10, 8, 0, 3>("wx43s10g"), wgx_cfg<4, 3, 12, 8, 0, 3>("wx43s12g"),
      wgx_cfg<2, 5, 4, 8, 0, 3>("wx25s4g"), wgx_cfg<2, 5, 6, 8, 0, 3>("wx25s6g"),
      // (the F(2x2, 5x5) forms spill ~20 loop-invariant VGPRs, reloaded once per unit run)
      wgx_cfg<2, 5, 3, 8, 0, 1>("wx25s3k"), wgx_cfg<2, 5, 4, 8, 0, 1>("wx25s4k"), wgx_cfg<2, 5, 6, 8, 0, 1>("wx25s6k"),
      wgx_cfg<2, 5, 6, 4, 0, 1>("wx25s6w4k"), wgx_cfg<2, 5, 8, 4, 0, 1>("wx25s8w4k"), wgx_cfg<2, 5, 12, 4, 0, 1>("wx25s12w4k"),
#ifdef BH_KTRACE
      // diagnostic builds of wx43s12 / wx25s6 (wrong results by design): one part of the stage dropped
      wgx_cfg<4, 3, 12, 8, 1>("xwx43_noxf"), wgx_cfg<4, 3, 12, 8, 2>("xwx43_nomfma"),
      wgx_cfg<4, 3, 12, 8, 4>("xwx43_nodma"), wgx_cfg<4, 3, 12, 8, 8>("xwx43_nou"),
      wgx_cfg<4, 3, 12, 8, 16>("xwx43_novf"), wgx_cfg<4, 3, 12, 8, 32>("xwx43_nobar"),
      wgx_cfg<4, 3, 12, 8, 29>("xwx43_onlymfma"), wgx_cfg<4, 3, 12, 8, 30>("xwx43_onlyxf"),
      // 6 bit: no strip DMA instructions at all, 7 bit: no U load instructions at all
      wgx_cfg<4, 3, 12, 8, 29 + 64 + 128>("xwx43_puremfma"), wgx_cfg<4, 3, 12, 8, 29 + 64 + 128 + 32>("xwx43_puremfma_nobar"),
      wgx_cfg<4, 3, 12, 8, 4 + 64>("xwx43_nodmaissue"),
      wgx_cfg<2, 5, 6, 8, 1>("xwx25_noxf"), wgx_cfg<2, 5, 6, 8, 2>("xwx25_nomfma"),
      wgx_cfg<2, 5, 6, 8, 8>("xwx25_nou"), wgx_cfg<2, 5, 6, 8, 29>("xwx25_onlymfma"),
#endif
  };
}

size_t wx_bank_floats(uint32_t OC, uint32_t IC) { return (size_t)((IC + 3) & ~3u) * ((OC + 31) & ~31u) * 36; }

int launch_wx_pack(bh_ctx *ctx, const float *filts, float *u, uint32_t OC, uint32_t IC, uint32_t R, bool first,
                   bool last) {
  uint32_t OC32 = (OC + 31) & ~31u, IC4 = (IC + 3) & ~3u;
  const uint64_t n = (uint64_t)OC32 * IC4;
  void *args[] = {(void *)&filts, (void *)&u, (void *)&OC, (void *)&IC, (void *)&OC32, (void *)&IC4};
  const void *k = R == 3 ? (const void *)wx_pack_kernel<3> : (const void *)wx_pack_kernel<5>;
  return bh::launch(ctx, k, dim3((uint32_t)((n + 255) / 256)), dim3(256), args, first, last, "wx_pack");
}

// Launch a position-split Winograd configuration: UNSUP unless a stride-1 R x R conv (R = the
// configuration's) with pad <= R / 2, IC % 4 == 0, IC <= 64 for F(4x4,3x3) and <= 96 for F(2x2,5x5)
// (their fp32 element error), whose strips fit the configuration's slot. r.bank: the bank of the configuration's
// form (6x6: wx_pack; 4x4: bh_wino.hip's). One block per unit (whole units), or (cfg_t::sk) a resident
// stream-K grid over the (unit, stage) iterations.
static int launch_wgx(bh_ctx *ctx, const cfg_t &c, const bh::conv_call &cc, GemmArgs &, const route_t &r) {
  if (!r.bank) return bh::fail(BH_UNSUP, std::string("conv: ") + c.name + " is for other kernel sizes");
  const uint32_t B = cc.B, IC = cc.IC, H = cc.H, W = cc.W, OC = cc.OC, py = cc.py, px = cc.px, out_ctot = cc.out_ctot;
  const float *const res = cc.res;
  float *const out = cc.out;
  const uint32_t R = (uint32_t)c.ky, MO = (uint32_t)c.mo, N = MO + R - 1;
  if (cc.KY != R || cc.KX != R || cc.sy != 1 || cc.sx != 1 || py != px || py > R / 2)
    return bh::fail(BH_UNSUP, std::string("conv: ") + c.name + " is for stride-1 square-padded convs of its kernel size");
  if (IC % XC) return bh::fail(BH_UNSUP, std::string("conv: ") + c.name + " needs IC % 4 == 0");
  // the 6x6 forms' element error grows as sqrt(IC) (the transformed-domain sum dominates it): measured
  // against float64 with Boda's element metric, F(4x4,3x3) reaches 1.1e-3 at IC 64 and 2.2e-3 at
  // IC 256 (2.15e-3 already at IC 128 on 20 x 128 x 28^2 -> 192, round 5's ops-prof sweep),
  // F(2x2,5x5) 0.8e-3 at IC 32 and 1.1-2.1e-3 at IC 96; the caps keep a forced
  // configuration near Boda's Winograd tolerance (2e-3, src/rtc_prof.cc:314-319), the tuner routes
  // only ops measured inside it
  const uint32_t ic_cap = N == 4 ? 0u : (MO == 4 ? 64u : 96u);
  if (ic_cap && IC > ic_cap)
    return bh::fail(BH_UNSUP, std::string("conv: ") + c.name + " keeps IC <= " + std::to_string(ic_cap) +
                                  " (fp32 element error of the 6x6 transforms)");
  const uint32_t pad = py;
  const uint32_t OH = H + 2 * pad - R + 1, OW = W + 2 * pad - R + 1;
  const uint32_t TH = (OH + MO - 1) / MO, TW = (OW + MO - 1) / MO, TPI = TH * TW;
  const uint64_t T64 = (uint64_t)B * TPI;
  const uint32_t VH = std::max(H + 2 * pad, MO * (TH - 1) + N);
  const uint32_t WPM = (std::max(W + 2 * pad, MO * (TW - 1) + N) + 3) & ~3u;
  if (T64 >= (1u << 30) || (uint64_t)B * VH >= (1u << 30)) return bh::fail(BH_UNSUP, "conv: too many Winograd tiles");
  const uint32_t T = (uint32_t)T64, ngroups = (T + XTT - 1) / XTT;
  auto vrow = [&](uint32_t tg) { return (tg / TPI) * VH + MO * ((tg % TPI) / TW); };
  uint32_t rin = 0;
  for (uint32_t gi = 0; gi < ngroups; ++gi) {
    const uint32_t a = gi * XTT, b = std::min(T, a + XTT) - 1;
    rin = std::max(rin, vrow(b) + N - vrow(a));
  }
  const uint32_t SP = (uint32_t)c.sp, XNT = (uint32_t)c.NT;
  if ((uint64_t)XC * rin * WPM > (uint64_t)SP * XNT)
    return bh::fail(BH_UNSUP, std::string("conv: input strip too large for ") + c.name);
  // (smaller strips than a configuration's slot are left to the configurations with fewer DMAs)
  const uint64_t out_bytes = (uint64_t)B * out_ctot * OH * OW * 4;
  if (out_bytes >= 0x7fffff00ull || (uint64_t)B * IC * H * W * 4 >= 0x7fffff00ull)
    return bh::fail(BH_UNSUP, "conv: tensors too large for the Winograd kernel");
  const uint32_t OC32 = (OC + 31) & ~31u, P = N * N;
  const uint64_t ubytes = (uint64_t)((IC + 3) & ~3u) * OC32 * P * 4;
  if (ubytes >= 0x7fffff00ull) return bh::fail(BH_UNSUP, "conv: Winograd bank too large");
  WxArgs p{};
  p.u = r.bank; p.in = cc.in; p.out = out; p.bias = cc.biases; p.res = res;
  p.u_bytes = (uint32_t)ubytes;
  p.in_bytes = (uint32_t)((uint64_t)B * IC * H * W * 4);
  p.out_bytes = (uint32_t)out_bytes;
  p.OC = OC; p.OC32 = OC32; p.IC = IC; p.B = B; p.H = H; p.W = W; p.pad = pad;
  p.OH = OH; p.OW = OW; p.OHW = OH * OW; p.HW = H * W; p.ICHW = IC * H * W; p.OCOHW = out_ctot * OH * OW;
  p.TW = TW; p.TPI = TPI; p.VH = VH; p.T = T; p.WPM = WPM; p.RW = rin * WPM;
  bh::set_fd(TW, p.tw_m, p.tw_s);
  bh::set_fd(TPI, p.tpi_m, p.tpi_s);
  bh::set_fd(VH, p.vh_m, p.vh_s);
  bh::set_fd(WPM, p.wpm_m, p.wpm_s);
  bh::set_fd(p.RW, p.rw_m, p.rw_s);
  p.ngr = ngroups;
  bh::set_fd(ngroups, p.ngr_m, p.ngr_s);
  p.ipt = IC / XC;
  bh::set_fd(p.ipt, p.ipt_m, p.ipt_s);
  p.relu = cc.relu;
  p.wt = r.wt;
  p.vst = (OW % MO == 0 && ((uintptr_t)out % (4 * MO)) == 0 && ((uintptr_t)res % (4 * MO)) == 0) ? 1 : 0;
  const uint32_t OCT = (uint32_t)c.BM, octiles = (OC + OCT - 1) / OCT;
  const uint64_t units = (uint64_t)ngroups * octiles;
  if (units >= (1u << 31)) return bh::fail(BH_UNSUP, "conv: too many Winograd units");
  // dynamic LDS: two strip slots + two V buffers, or the epilogue's exchange (NT pairs x pitch); then
  // the stream-K ticket flag
  const uint32_t NPG = N == 6 ? 4 : 2, PS = N == 6 ? 12 : 8, XS = N == 6 ? 52 : 20;
  const uint32_t lds = (std::max(2 * SP * XNT + 2 * NPG * XC * XTT * PS, XNT * XS) + 4) * 4;
  if (lds > 160 * 1024) return bh::fail(BH_UNSUP, std::string("conv: LDS too small for ") + c.name);
  const void *k = (const void *)c.k[A_KVEC][B_DIRECT][0];
  if (int rc = bh::dyn_lds(k, lds, "conv: Winograd LDS attribute")) return rc;
  uint32_t G = (uint32_t)units;
  bh::scratch_t sc;
  // blocks resident at once (the split forms' rounds)
  const uint64_t C = c.sk ? (uint64_t)bh::num_cus(ctx) * (uint32_t)std::min(bh::occupancy(k, (int)XNT, (size_t)lds), 2) : 0;
  if (c.sk == 3) {
    // whole units in full rounds of the resident blocks; the tail round's T units as NOG pieces each,
    // when they fit one round
    const uint32_t NOG = XNT / 64 / NPG;
    const uint64_t R = units / C, T = units - R * C;
    p.ipb = (uint32_t)units;
    p.total_it = 1;
    if (T && NOG > 1 && T * NOG <= C) {
      p.ipb = (uint32_t)(R * C);
      p.total_it = NOG;
      G = (uint32_t)(R * C + T * NOG);
    }
  } else if (c.sk == 2) {
    // whole units in full rounds of the resident blocks; the tail round's T units in S pieces each
    const uint64_t R = units / C, T = units - R * C;
    const uint32_t S = T ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(p.ipt, C / T)) : 1u;
    if (S == 1) {
      p.ipb = (uint32_t)units;  // nothing to split: every block takes a whole unit
      p.total_it = 1;
    } else {
      p.ipb = (uint32_t)(R * C);
      p.total_it = S;
      G = (uint32_t)(R * C + T * S);
      const size_t slab = (size_t)(16 / (XNT / ((XNT / 64 / NPG) * 64))) * XNT * MO * MO;
      if (int rc = bh::scratch(ctx, (size_t)2 * G * slab * 4, units, sc)) return rc;
    }
  } else if (c.sk) {
    // stream-K: as many blocks as are resident at once, the (unit, stage) iterations dealt equally
    const uint64_t total = units * p.ipt;
    if (total >= (1u << 31)) return bh::fail(BH_UNSUP, "conv: too many Winograd iterations");
    p.ipb = (uint32_t)((total + C - 1) / C);
    G = (uint32_t)((total + p.ipb - 1) / p.ipb);
    p.total_it = (uint32_t)total;
    const size_t slab = (size_t)(16 / (XNT / ((XNT / 64 / NPG) * 64))) * XNT * MO * MO;  // NR * NT * MO^2 floats
    if (int rc = bh::scratch(ctx, (size_t)2 * G * slab * 4, units, sc)) return rc;
  }
  p.ws = sc.ws;  // null where the form cuts no unit
  p.cnt = sc.cnt;
  bh::set_trace(ctx, p);
  void *args[] = {&p};
  // splits 20 on a stream-K configuration: the cut units summed by wx_combine_kernel (a second launch)
  p.sepc = (c.sk == 1 && r.splits == 20) ? 1 : 0;
  if (!p.sepc) return bh::launch(ctx, k, dim3(G, 1, 1), dim3(XNT), args, r.first, true, "conv_wgx", lds);
  int rc = bh::launch(ctx, k, dim3(G, 1, 1), dim3(XNT), args, r.first, false, "conv_wgx", lds);
  if (rc != BH_OK) return rc;
  const uint32_t NR = 16 / (XNT / ((XNT / 64 / NPG) * 64));
  return bh::launch(ctx, (const void *)c.k[A_KVEC][B_DIRECT][1], dim3((uint32_t)units * NR, 1, 1), dim3(XNT), args,
                    false, true, "conv_wgx_combine");
}

}  // namespace bhk
