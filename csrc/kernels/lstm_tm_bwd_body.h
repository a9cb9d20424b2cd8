// Device body of the time-major LSTM backward recurrence, shared by the per-layer backward kernels
// (lstm_tm_bwd.hip) and by the launch that runs a recurrence next to weight-gradient jobs
// (lstm_grads_jobs.hip lstm_tm_bwd_dual_kernel). One workgroup = one 16-sequence tile for all T steps;
// the template flags pick what leaves the recurrence: dz (DZ), dx (DX), the tile's weight-gradient
// split record (WG), and how the gates arrive (saved, or recomputed: RG).
#pragma once
#include "common.h"

#include <type_traits>
#include "lstm_tm_common.h"

namespace gq {

// backward recurrence. Per reverse step: cell phase (dz_t of the lane's own cells), then
// dh_{t-1} = U dz_t on MFMA (the serial chain) and, off the chain,
//   DZ: the dz_t tile -> HBM (fp32 [T+1][Mp][4H]); the weight gradients and dx are then ONE
//       parallel pass over all T*Mp rows (lstm_grads_rows): folding them into this kernel
//       lengthens every step of the serial chain and pushes H = 32 past the VGPR budget.
//   DX: dx^T = W dz_t^T tile -> HBM (frozen-weight input gradients, e.g. integrated gradients).
// dhout: [T][Mp][H] (or [Mp][H] for the last step only). Skipped stores go to time row T.
#ifndef TMW_D16
#define TMW_D16 4        // ring depth (reverse steps) of lstm_tm_bwd_wg_kernel's streams, H = 16
#endif
#ifndef TMW_D32
#define TMW_D32 6        // H = 32 (T = 337 micro: 642 -> 555 us from 4 to 6)
#endif
// (backward: the dz / x images go to LDS with 16-bit stores. They conflict 2-way, but packing dwords
// after a lane-pair exchange cost more: SoilNet 3.29 vs 3.14 ms, IG 5.86 vs 5.67 ms per call,
// profiles/r6_packed_z_ab.txt)
#ifndef TMB_ZSWZ
#define TMB_ZSWZ 1       // swizzled dz tile in the backward (A/B: 0)
#endif

// WG (H <= 32 layers of many tiles, e.g. SoilNet's 418): the weight gradients ride in the
// recurrence instead of a separate pass over the dz / x / h streams. Per reverse step and wave w
// (gate rows 16w .. 16w + 15):
//   dW^T | db += dz_t^T [x_t | 1]   and   dU^T += dz_t^T h_{t-1}
// as v_mfma_f32_16x16x32_bf16 over a PAIR of steps (K = 2 x the tile's 16 sequences; issued every
// other step, which halved their cost on the serial step against one 16x16x16 MFMA per step): dz^T
// comes from a column-major copy of the step's dz tile the cell phase writes next to the row-major
// one, x_t and h_{t-1} are streamed through the same kind of register ring as the saved state and
// staged transposed (bf16) beside it; four image buffers (step & 3), since the pair's older step is
// read while the faster waves already write the next one. The partial tiles stay in VGPRs for all T steps and leave once per workgroup as one
// split record of the weight-gradient pass's layout (lstm_grads_body.h: [tile][cb][DT + HT][4]
// [64][4]), summed over the tiles by the same fixed-order reduction. dz itself never reaches HBM.
// RG (recompute gates): the forward saved no gates (lstm_tm_fwd SG = false). Each step's i, f, g, o
// are recomputed here from x_t and h_{t-1} - the forward's own bf16 operands, fragments, bias and MFMA
// order, so the pre-activations are bitwise the forward's - one step ahead, in the MFMA phase of the
// step before (off the serial chain: they depend on saved data only). x_t / h_{t-1} come through the
// same register rings as the WG streams and are staged row-major ([sequence][channel], the forward's B
// operand layout) into a double buffer.
// UP (un-pool on load): the layer's output went through MaxPooling1D(P) (valid, stride P) and dhout is
// the POOLED gradient [T / P][Mp][H] with the pool's byte argmax pidx of the same shape; the dh stream
// reads pooled granule floor(t / P) and its 4 argmax bytes and keeps the components whose argmax is
// t mod P (zero past the last window), as maxpool1d_bwd would have written them at full resolution -
// that kernel and its full-resolution dh round trip through HBM are gone.
template <int H, int KX, int GR, int D, bool DZ, bool DX, bool LAST, bool WG = false, bool RG = false,
          bool UP = false, bool XB = false, bool HB = false>
__device__ __forceinline__ void lstm_tm_bwd_body(
    const float* __restrict__ dhout, const __bf16* __restrict__ gbuf, const float* __restrict__ cbuf,
    const float* __restrict__ W, const float* __restrict__ U, float* __restrict__ dx, __bf16* __restrict__ dz,
    int Mp, int T, int Din, int Dw, int tile, int ntiles, const float* __restrict__ xw = nullptr,
    const float* __restrict__ hw = nullptr, float* __restrict__ wsr = nullptr,
    const float* __restrict__ bias = nullptr, const unsigned char* __restrict__ pidx = nullptr, int P = 1) {
  static_assert(!(UP && LAST), "un-pooling needs a per-step gradient");
  using C = TMC<H>;
  constexpr int CPL = C::CPL, NW = C::NW, NT = C::NT, G4 = C::G4, KB = C::KB;
  static_assert(!WG || (CPL == 1 && NT == 16 * H && G4 == 16 * NW && GR == 4), "fused weight gradients: H <= 64");
  static_assert(!RG || (CPL == 1 && NT == 16 * H && GR == 4), "recomputed gates: H <= 64, 16-byte x granules");
  constexpr bool XS = WG || RG;                   // x_t / h_{t-1} streams
  constexpr int NXB = KX * 2;                     // din blocks of dx^T (16 rows each)
  constexpr int TX = (NXB + NW - 1) / NW;         // dx tiles per wave
  static_assert(16 * G4 / 4 == NT, "one dz float4 granule per thread");
  // LDS pitches chosen with a model of the gfx950 bank rules (MI355X_MICROARCH.md §LDS: ds_write_b32 /
  // ds_read_b32 bank = dword mod 32 per 32-lane group, ds_read_b128 four 16-lane groups over 64 banks):
  // dz rows G4 + 16 bf16, dx rows 32 KX + 1 floats (the dx^T stores of a wave - 16 sequences x 4
  // quads - landed on 2 banks with a 32-float pitch: 16-way), x / h staging rows + 16 bf16
  constexpr int ZSP = G4 + 16, DXP = DX ? 32 * KX + 1 : 1;
  __shared__ __attribute__((aligned(16))) __bf16 zs[2][16][ZSP];        // dz row-major (B of U dz^T, W dz^T)
  // dz element e of sequence c sits at zs[.][c][zsw(c, e)]: 16-byte chunk index XOR bit 2 of the sequence
  // (scripts/lds_model/zs_swizzle.py: with the G4 + 16 pitch the cell phase's 16-bit stores were 4-way)
  auto zsw = [](int c, int e) { return TMB_ZSWZ ? e ^ (((c >> 2) & 1) << 3) : e; };
  __shared__ __attribute__((aligned(16))) float dhs[2][16][C::HP];      // dh_out tile
  __shared__ __attribute__((aligned(16))) float dxs[2][16][DXP];        // dx tile

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index in an SGPR
  const int col = lane & 15, quad = lane >> 4;
  const int row0 = tile * 16;

  for (int i = tid; i < 2 * 16 * C::HP; i += NT) (&dhs[0][0][0])[i] = 0.f;

  // fused weight gradients (WG): transposed bf16 images [row][sequence] of dz_t, [x_t | 1] and h_{t-1}
  constexpr int XR = WG ? 32 * KX + 16 : 1;        // x image rows: channels, the bias row, zero rows
  constexpr int DTM = WG ? 2 * KX + 1 : 1;         // dW^T din blocks (incl. the bias row), upper bound
  constexpr int HTW = WG ? H / 16 : 1;             // dU^T k blocks
  constexpr int NB = WG ? 4 : 1, RP = 24;          // image buffers, row pitch (48 B: 16-byte aligned rows)
  __shared__ __attribute__((aligned(16))) __bf16 zT[NB][WG ? G4 : 1][RP];
  __shared__ __attribute__((aligned(16))) __bf16 xT[NB][XR][RP];
  __shared__ __attribute__((aligned(16))) __bf16 hT[NB][WG ? H : 1][RP];
  const int dtw = (Dw + 16) / 16;                  // din blocks of this layer (record layout DT)
  f32x4_t accW[DTM], accU[HTW];
  if constexpr (WG) {
    for (int i = tid; i < NB * XR * RP; i += NT) {
      const int dn = (i / RP) % XR;
      (&xT[0][0][0])[i] = (__bf16)(dn == Dw ? 1.f : 0.f);
    }
#pragma unroll
    for (int d = 0; d < DTM; ++d) accW[d] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < HTW; ++k) accU[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // A fragments of U (dh_rec) and W (dx^T): tile row `col` of cell group gi is unit
  // 4 gi + (col >> 2) when col % 4 == 0 and zero otherwise -> acc[0] is the lane's own cell
  bf16x8_t ufr[CPL][KB];
  int unit[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) {
    const int gi = w + NW * cc;
    unit[cc] = 4 * gi + quad;
    const int au = 4 * gi + (col >> 2);
#pragma unroll
    for (int s = 0; s < KB; ++s) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float val = U[(size_t)au * G4 + 32 * s + 8 * quad + j];
        v[j] = (__bf16)(val * ((col & 3) == 0 ? 1.0f : 0.0f));
      }
      ufr[cc][s] = v;
    }
  }
  // WL (H = 64: 16 waves, 128 VGPRs each): the dx A fragments are read from an LDS image of W^T
  // instead of living in 32 VGPRs; in registers they pushed the body into 16-23 VGPRs of spills,
  // whose scratch reloads sat on the serial step
  constexpr bool WL = DX && H == 64;
  constexpr bool WRG = DX && !WL;
  __shared__ __attribute__((aligned(16))) __bf16 wls[WL ? 32 * KX : 1][WL ? G4 + 8 : 8];
  if constexpr (WL) {
    for (int i = tid; i < 32 * KX * G4; i += NT) {
      const int dn = i / G4, g = i % G4;
      wls[dn][g] = (__bf16)(dn < Dw ? W[(size_t)dn * G4 + g] : 0.f);
    }
  }
  bf16x8_t wfr[WRG ? TX : 1][WRG ? KB : 1];
  if constexpr (WRG) {
#pragma unroll
    for (int q = 0; q < TX; ++q) {
      const int xb = w + NW * q;
      const int din = 16 * xb + col;
#pragma unroll
      for (int s = 0; s < KB; ++s) {
        bf16x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (__bf16)(W[(size_t)min(din, Dw - 1) * G4 + 32 * s + 8 * quad + j] * ((xb < NXB && din < Dw) ? 1.0f : 0.0f));
        wfr[q][s] = v;
      }
    }
  }

  // ---- streams. internal state (per lane, ring over reverse steps): gates, c_t
  uint2 rg[CPL][RG ? 1 : D];                      // packed bf16 gates (not saved under RG)
  // c_t ring: under RG the forward saved c in bf16 (TM_RG_BF16C), kept raw here and widened where used
  using CT = std::conditional_t<RG && TM_RG_BF16C, __bf16, float>;
  CT rc[CPL][D];
  auto idx = [&](int tt, int cc) { return ((((size_t)tt * ntiles + tile) * NW + w) * CPL + cc) * 64 + lane; };
#define GQ_TMB_LOAD_STATE(J, SS)                                                    \
  {                                                                                 \
    const int tt_ = max(T - 1 - (SS), 0);                                           \
    _Pragma("unroll") for (int cc = 0; cc < CPL; ++cc) {                            \
      const size_t o_ = idx(tt_, cc);                                               \
      if constexpr (!RG) rg[cc][J] = *reinterpret_cast<const uint2*>(gbuf + o_ * 4); \
      rc[cc][J] = reinterpret_cast<const CT*>(cbuf)[o_];                            \
    }                                                                               \
  }
  // Streams: every wave loads and stages granule (tid mod n) of each contiguous tile (no
  // branch around memory ops, see the forward). dh: [16][H] float4 granules.
  constexpr int n_gd = 16 * H / 4;
  const int gd = (tid % n_gd) * 4;
  const float* dbase = dhout + (size_t)row0 * H + gd;
  const size_t dstep = LAST ? 0 : (size_t)Mp * H;
  const unsigned* ibase = UP ? reinterpret_cast<const unsigned*>(pidx + (size_t)row0 * H + gd) : nullptr;
  const int Ts = UP ? T / P : 0;
  // t / P as a multiply-high (exact for t * P < 2^32); P == 1 is the identity (its magic would wrap)
  const unsigned pmag = (UP && P > 1) ? 0xFFFFFFFFu / (unsigned)P + 1u : 0u;
  float4 rd[D];
  auto dh_tile = [&](int j, int t) -> float4 { (void)t; return rd[j]; };
  // dz storer: one float4 granule of the [16][4H] tile per thread
  const int gz_seq = tid / (G4 / 4), gz_c = (tid % (G4 / 4)) * 4;
  __bf16* zbase = dz + (size_t)(row0 + gz_seq) * G4 + gz_c;
  const size_t zstep = (size_t)Mp * G4;
  // dx storer over [16][Din] granules of GR floats (lanes past the tile rewrite granule 0)
  const int n_gx = 16 * Din / GR;
  const int gx = (tid % n_gx) * GR;
  const int gx_seq = gx / Din, gx_k = gx % Din;
  const size_t xstep = (size_t)Mp * Din;
  float* sbase = dx + (size_t)row0 * Din + gx;
  // WG streams: XG consecutive floats of the [16][Din] x_t tile (threads past the tile repeat it)
  // and element tid of the [16][H] h_{t-1} tile, in rings over reverse steps like the saved state
  constexpr int XG = XS ? (16 * 32 * KX / NT > 1 ? 16 * 32 * KX / NT : 1) : 1;
  static_assert(XG <= 4, "x stream granule");
  // XB / HB: x / h_{t-1} are bf16 (a recompute-gates pair's layer-A output, TM_RG_BF16H)
  std::conditional_t<XB, GranuleH<XG>, Granule<XG>> wx[XS ? D : 1];
  std::conditional_t<HB, __bf16, float> wh[XS ? D : 1];
  const int wxe = (tid * XG) % (16 * Din);
  const int wx_seq = wxe / Din, wx_k = wxe % Din;
  const auto wxb = reinterpret_cast<std::conditional_t<XB, const __bf16*, const float*>>(xw) + (size_t)row0 * Din + wxe;
  const auto whb = reinterpret_cast<std::conditional_t<HB, const __bf16*, const float*>>(hw) + (size_t)row0 * H + tid;
  const size_t whstep = (size_t)Mp * H;
#define GQ_TMB_LOAD_W(J, SS)                                                        \
  if constexpr (XS) {                                                               \
    const int tt_ = max(T - 1 - (SS), 0);                                           \
    wx[J].load(wxb + (size_t)tt_ * xstep);                                          \
    wh[J] = whb[(size_t)max(tt_ - 1, 0) * whstep];                                  \
  }

  // RG: the forward's A fragments (rows permuted: tile row `col` = gate (col & 3) of unit 4 w + (col >> 2)),
  // bias, and the row-major bf16 x_t / h_{t-1} double buffers
  constexpr int KSH = C::KSH;
  __shared__ __attribute__((aligned(16))) __bf16 xrs[RG ? 2 : 1][16][RG ? 32 * KX + 16 : 8];
  __shared__ __attribute__((aligned(16))) __bf16 hrs[RG ? 2 : 1][16][RG ? C::KPH + 16 : 8];
  bf16x8_t fu[RG ? KSH : 1], fw[RG ? KX : 1];
  f32x4_t fb4 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (RG) {
    for (int i = tid; i < 2 * 16 * (32 * KX + 16); i += NT) (&xrs[0][0][0])[i] = (__bf16)0.0f;
    for (int i = tid; i < 2 * 16 * (C::KPH + 16); i += NT) (&hrs[0][0][0])[i] = (__bf16)0.0f;
    const int au = 4 * w + (col >> 2), ag = col & 3;
#pragma unroll
    for (int s = 0; s < KSH; ++s) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * quad + j;
        v[j] = (__bf16)(U[min(k, H - 1) * G4 + ag * H + au] * (k < H ? 1.0f : 0.0f));
      }
      fu[s] = v;
    }
#pragma unroll
    for (int s = 0; s < KX; ++s) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * quad + j;
        v[j] = (__bf16)(W[min(k, Dw - 1) * G4 + ag * H + au] * (k < Dw ? 1.0f : 0.0f));
      }
      fw[s] = v;
    }
    const int u = 4 * w + quad;
    fb4 = f32x4_t{bias[u], bias[H + u], bias[2 * H + u], bias[3 * H + u]};
  }
  // x_tt and h_{tt-1} of ring slot J into buffer b (h_{-1} = 0)
  auto rg_stage = [&](int b, int J, int tt) {
    if constexpr (RG) {
#pragma unroll
      for (int q = 0; q < XG; ++q) xrs[b][wx_seq][wx_k + q] = wx[J].bf(q);
      hrs[b][tid / H][tid % H] = (__bf16)((float)wh[J] * (tt >= 1 ? 1.f : 0.f));
    }
  };
  // pre-activations from buffer b: exactly the forward's two MFMA chains (x part from the bias)
  auto rg_pre = [&](int b) -> f32x4_t {
    f32x4_t ax = fb4, ah = {0.f, 0.f, 0.f, 0.f};
    if constexpr (RG) {
#pragma unroll
      for (int s = 0; s < KX; ++s) {
        const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(&xrs[b][col][32 * s + 8 * quad]);
        ax = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[s], bx, ax, 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < KSH; ++s) {
        const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(&hrs[b][col][32 * s + 8 * quad]);
        ah = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fu[s], bh, ah, 0, 0, 0);
      }
    }
    return ax + ah;
  };

  // reverse step s <-> time t = T-1-s. Streams for step s are loaded D steps ahead.
#define GQ_TMB_LOAD_D(J, SS)                                                                \
  if constexpr (UP) {                                                                       \
    const int tt_ = max(T - 1 - (SS), 0);                                                   \
    const int st_ = P > 1 ? (int)__umulhi((unsigned)tt_, pmag) : tt_;                      \
    const int sc_ = min(st_, Ts - 1);                                                       \
    float4 v_ = *reinterpret_cast<const float4*>(dbase + (size_t)sc_ * dstep);              \
    const unsigned id_ = ibase[(size_t)sc_ * dstep / 4];                                    \
    const unsigned ph_ = st_ < Ts ? (unsigned)(tt_ - st_ * P) : 0xffu + 1u;                 \
    v_.x = (id_ & 0xffu) == ph_ ? v_.x : 0.f;                                               \
    v_.y = ((id_ >> 8) & 0xffu) == ph_ ? v_.y : 0.f;                                        \
    v_.z = ((id_ >> 16) & 0xffu) == ph_ ? v_.z : 0.f;                                       \
    v_.w = (id_ >> 24) == ph_ ? v_.w : 0.f;                                                 \
    rd[J] = v_;                                                                             \
  } else {                                                                                  \
    const int tt_ = max(T - 1 - (SS), 0);                                                   \
    float4 v_ = *reinterpret_cast<const float4*>(dbase + (size_t)tt_ * dstep);              \
    if (LAST) {                                                                             \
      const float m_ = (SS) == 0 ? 1.f : 0.f;                                               \
      v_.x *= m_; v_.y *= m_; v_.z *= m_; v_.w *= m_;                                       \
    }                                                                                       \
    rd[J] = v_;                                                                             \
  }
#pragma unroll
  for (int j = 0; j < D; ++j) {
    GQ_TMB_LOAD_STATE(j, j)
    GQ_TMB_LOAD_D(j, j)
    GQ_TMB_LOAD_W(j, j)
  }
  __syncthreads();
  // stage step 0 (t = T-1) tiles
  *reinterpret_cast<float4*>(&dhs[0][gd / H][gd % H]) = dh_tile(0, T - 1);
  GQ_TMB_LOAD_D(0, D)
  rg_stage(0, 0, T - 1);
  float dc[CPL], dhr[CPL], dhn[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) dc[cc] = dhr[cc] = 0.f;
  __syncthreads();
  // (RG) gates of the step to come: pre-activations from the MFMA phase of the step before, activated
  // at the end of that phase (after its dx / weight-gradient MFMAs have covered the MFMA latency)
  auto rg_act = [&](const f32x4_t& a) {
    return make_float4(sigmoidf_fast(a[0]), sigmoidf_fast(a[1]), tanhf_fast(a[2]), sigmoidf_fast(a[3]));
  };
  f32x4_t pre = rg_pre(0);
  float4 gn = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (RG) gn = rg_act(pre);
  // dh_out of the step to come, read from LDS one step early (right after the barrier that
  // published it) so the cell phase does not wait on an LDS round trip
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) dhn[cc] = dhs[0][col][unit[cc]];

  for (int s0 = 0; s0 < T; s0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int s = s0 + j;
      const int t = T - 1 - s;
      const int p = s & 1;
      const int jn = (j + 1 == D) ? 0 : j + 1;
      // ---------------- cell phase
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc) {
        const int u = unit[cc];
        const float cp = (float)rc[cc][jn] * (t > 0 ? 1.f : 0.f);      // c_{t-1}
        const float dh = dhn[cc] + dhr[cc];
        float4 g4;
        if constexpr (RG)
          g4 = gn;
        else
          g4 = gates_unpack(rg[cc][j]);
        const float tc = tanhf_fast((float)rc[cc][j]);
        const float dct = dc[cc] + dh * g4.w * (1.f - tc * tc);
        dc[cc] = dct * g4.y;
        const __bf16 z0 = (__bf16)(dct * g4.z * g4.x * (1.f - g4.x));
        const __bf16 z1 = (__bf16)(dct * cp * g4.y * (1.f - g4.y));
        const __bf16 z2 = (__bf16)(dct * g4.x * (1.f - g4.z * g4.z));
        const __bf16 z3 = (__bf16)(dh * tc * g4.w * (1.f - g4.w));
        zs[p][col][zsw(col, 0 * H + u)] = z0;
        zs[p][col][zsw(col, 1 * H + u)] = z1;
        zs[p][col][zsw(col, 2 * H + u)] = z2;
        zs[p][col][zsw(col, 3 * H + u)] = z3;
        if constexpr (WG) {
          zT[s & 3][0 * H + u][col] = z0;
          zT[s & 3][1 * H + u][col] = z1;
          zT[s & 3][2 * H + u][col] = z2;
          zT[s & 3][3 * H + u][col] = z3;
        }
      }
      if constexpr (WG) {   // stage [x_t | 1] and h_{t-1} of this step, refill the slots
        const float hm = t >= 1 ? 1.f : 0.f;
#pragma unroll
        for (int q = 0; q < XG; ++q) {
          const int dn = wx_k + q;
          xT[s & 3][dn][wx_seq] = dn < Dw ? wx[j].bf(q) : (__bf16)(dn == Dw ? 1.f : 0.f);
        }
        hT[s & 3][tid % H][tid / H] = (__bf16)((float)wh[j] * hm);
      }
      rg_stage((s + 1) & 1, jn, t - 1);            // (RG) x_{t-1}, h_{t-2}: the next step's gates
      GQ_TMB_LOAD_W(j, s + D)
      GQ_TMB_LOAD_STATE(j, s + D)
      *reinterpret_cast<float4*>(&dhs[p ^ 1][gd / H][gd % H]) = dh_tile(jn, t - 1);   // dh tile of step s+1
      GQ_TMB_LOAD_D(jn, s + 1 + D)
      lds_barrier();
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc) dhn[cc] = dhs[p ^ 1][col][unit[cc]];   // next step's dh_out
      // ---------------- MFMA phase
      // (a) serial chain: dh_{t-1} = U dz_t
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc) {
        f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const bf16x8_t bz = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][zsw(col, 32 * k + 8 * quad)]);
          if (k & 1) a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[cc][k], bz, a1, 0, 0, 0);
          else a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[cc][k], bz, a0, 0, 0, 0);
        }
        dhr[cc] = a0[0] + a1[0];
      }
      if constexpr (RG) pre = rg_pre((s + 1) & 1);   // next step's gates, behind the serial chain
      // (a') weight gradients of the step pair (s - 1, s) at odd s, or of the last step alone
      // (K lanes of the missing older step zeroed); the unrolled chunk's pad steps add nothing
      if (WG && t >= 0 && ((s & 1) || t == 0)) {
        const int half = quad >> 1, so = 8 * (quad & 1);      // K = 8 quad + i -> (step of the pair, sequence)
        const int bk = half ? (s & 3) : ((s - 1) & 3);
        const bool live = half || (s & 1);
        const bf16x8_t zero8 = {};
        // (both operands of a dead half are zeroed: its buffers may hold anything, NaN patterns too)
        bf16x8_t az = *reinterpret_cast<const bf16x8_t*>(&zT[bk][16 * w + col][so]);
        az = live ? az : zero8;
#pragma unroll
        for (int d = 0; d < DTM; ++d)
          if (d < dtw) {                            // wave-uniform, no global memory access inside
            bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(&xT[bk][16 * d + col][so]);
            bx = live ? bx : zero8;
            accW[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bx, accW[d], 0, 0, 0);
          }
#pragma unroll
        for (int k = 0; k < HTW; ++k) {
          bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(&hT[bk][16 * k + col][so]);
          bh = live ? bh : zero8;
          accU[k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bh, accU[k], 0, 0, 0);
        }
      }
      // (b) dz tile of this step -> HBM as bf16 (its exact values: the MFMAs above consumed
      // these bf16 values; steps past t = 0 pad the unrolled chunk: scratch row)
      if constexpr (DZ) {
        const uint2 zv = *reinterpret_cast<const uint2*>(&zs[p][gz_seq][zsw(gz_seq, gz_c)]);
        const int tz = t >= 0 ? t : T;
        *reinterpret_cast<uint2*>(zbase + (size_t)tz * zstep) = zv;
      }
      // (c) previous step's dx tile -> HBM (written by all waves before this barrier)
      if constexpr (DX) {
        const int ts = (s >= 1 && s <= T) ? t + 1 : T;
#pragma unroll
        for (int q = 0; q < GR; ++q) sbase[(size_t)ts * xstep + q] = dxs[p ^ 1][gx_seq][gx_k + q];
      }
      // (d) dx^T = W dz^T for this step (steps past t = 0 only pad the unrolled chunk and
      // must not overwrite the t = 0 tile the epilogue stores; no memory op in the branch)
      if (DX && t >= 0) {
#pragma unroll
        for (int q = 0; q < TX; ++q) {
          const int xb = w + NW * q;
          if (xb < NXB) {                           // wave-uniform
            f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < KB; ++k) {
              const bf16x8_t bz = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][zsw(col, 32 * k + 8 * quad)]);
              bf16x8_t wa;
              if constexpr (WL) wa = *reinterpret_cast<const bf16x8_t*>(&wls[16 * xb + col][32 * k + 8 * quad]);
              else wa = wfr[q][k];
              a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, bz, a, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) dxs[p][col][16 * xb + 4 * quad + r] = a[r];
          }
        }
      }
      if constexpr (RG) gn = rg_act(pre);           // the next step's gates
    }
  }
  __syncthreads();
  if constexpr (DX) {   // dx tile of t = 0
    const int pl = (T - 1) & 1;
#pragma unroll
    for (int q = 0; q < GR; ++q) sbase[q] = dxs[pl][gx_seq][gx_k + q];
  }
  if constexpr (WG) {   // this tile's split record: wave w = column block w / 4, record wave w % 4
    const int cb = w >> 2, wr = w & 3;
    float* rec = wsr + ((size_t)tile * (G4 / 64) + cb) * (size_t)(dtw + HTW) * 1024;
#pragma unroll
    for (int d = 0; d < DTM; ++d)
      if (d < dtw) *reinterpret_cast<f32x4_t*>(rec + ((size_t)(d * 4 + wr) * 64 + lane) * 4) = accW[d];
#pragma unroll
    for (int k = 0; k < HTW; ++k)
      *reinterpret_cast<f32x4_t*>(rec + ((size_t)((dtw + k) * 4 + wr) * 64 + lane) * 4) = accU[k];
  }
#undef GQ_TMB_LOAD_STATE
#undef GQ_TMB_LOAD_D
#undef GQ_TMB_LOAD_W
}

}  // namespace gq
