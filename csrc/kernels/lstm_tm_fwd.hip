// Time-major persistent LSTM forward for gfx950: one layer (lstm_tm_fwd) or a layer pair in one
// launch (lstm_tm2_fwd).
//
// Layout: every activation inside the TimeLayer is time-major, [T][Mp][C] with Mp a
// multiple of 16, so the per-step tile of a 16-sequence block is ONE contiguous run of
// 16*C floats. All global traffic in the recurrence is tile-granular and coalesced:
//   * loader lanes stream x_t tiles (float4 / float2 / float granules) through a register ring and
//     stage them into LDS one step ahead;
//   * storer lanes write whole h_t tiles from an fp32 LDS copy;
//   * the training-only state (packed bf16 gates and c, or c alone when the backward recomputes the
//     gates) is written in a lane-natural layout ([T][tile][wave][cell][lane]) - one contiguous run per
//     wave and step.
// (Measured on the CML shapes, per-cell scattered accesses - 16 rows per instruction -
// were what bound lstm_v3; see profiles/r1_lstm_microbench.md.)
//
// Compute mapping (as lstm_v3): the rows of the MFMA A operand are permuted so one
// 16x16 output tile holds (unit, gate) pairs and every lane receives the i,f,g,o
// pre-activations of its own cell(s): 5 activations per cell and lane, one LDS
// barrier per step. H <= 64: one cell per lane, H/4 waves.
//
// The host entry points turn (H, x channel blocks, x granule, train, saved gates, pool) into template
// arguments with tm_dispatch / dispatch_bools (lstm_tm_common.h); only the combinations tm_supported
// and tm_rg_ok admit are instantiated.
#include "common.h"

#include "lstm_tm_common.h"

namespace gq {

// =====================================================================================
// forward
// x: [T][Mp][Din]  hout: [T][Mp][H]  gbuf: [T][tiles][NW][CPL][64][4]  cbuf: [..][64]
// 1024-thread workgroups ask for 8 waves per SIMD, i.e. two workgroups per CU (at the default
// allocation, ~70-80 VGPRs, only one fits and a 418-tile grid - SoilNet, 6,688 sequences - runs in
// two rounds on 256 CUs) where that costs no spills: the H = 64 layer with a 32-channel input
// (70.6 vs 76.7 us on the SoilNet step) and the H = 32 pair (214.5 vs 221.5 us). The 64-channel
// input variant spills at 64 VGPRs (169 vs 105 us) and keeps the default.
template <int NT, int KX = 1>
struct TmOcc {
  static constexpr int W = (NT >= 1024 && KX == 1) ? 8 : 1;
};

// SG = false (train mode, recompute-gates backward, lstm_tm_bwd_body RG): only c is saved; the
// backward recomputes the gates from x_t and h_{t-1} (same bf16 operands, same MFMA order: bitwise the
// forward's pre-activations), which halves the forward's state stream (h + c + packed gates = 16 B per
// cell-step -> 8 B) and drops the backward's 8-byte gate read
template <int H, bool TRAIN, int KX, int GR, int D, bool SG = true>
__global__ __launch_bounds__(TMC<H>::NT, (TmOcc<TMC<H>::NT, KX>::W)) void lstm_tm_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ U,
    const float* __restrict__ bias, float* __restrict__ hout, __bf16* __restrict__ gbuf,
    float* __restrict__ cbuf, int Mp, int T, int Din, int Dw) {
  // Din: channels of the x layout (row pitch); Dw <= Din: rows of W (padding channels of x are zero)
  using C = TMC<H>;
  constexpr int CPL = C::CPL, NW = C::NW, NT = C::NT, G4 = C::G4;
  constexpr int KPX = 32 * KX;
  __shared__ __attribute__((aligned(16))) __bf16 hs[2][16][C::KPH + 8];
  __shared__ __attribute__((aligned(16))) __bf16 xs[2][16][KPX + 8];
  __shared__ __attribute__((aligned(16))) float hf[2][16][C::HP];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index in an SGPR
  const int col = lane & 15, quad = lane >> 4;
  const int tile = blockIdx.x, ntiles = gridDim.x, row0 = tile * 16;

  for (int i = tid; i < 2 * 16 * (C::KPH + 8); i += NT) (&hs[0][0][0])[i] = (__bf16)0.0f;
  for (int i = tid; i < 2 * 16 * (KPX + 8); i += NT) (&xs[0][0][0])[i] = (__bf16)0.0f;

  // A fragments: tile row `col` of cell group gi = gate (col & 3) of unit 4 gi + (col >> 2)
  bf16x8_t ufr[CPL][C::KSH], wfr[CPL][KX];
  f32x4_t bias4[CPL];
  int unit[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) {
    const int gi = w + NW * cc;
    const int au = 4 * gi + (col >> 2), ag = col & 3;
    unit[cc] = 4 * gi + quad;
#pragma unroll
    for (int s = 0; s < C::KSH; ++s) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * quad + j;
        v[j] = (__bf16)(U[min(k, H - 1) * G4 + ag * H + au] * (k < H ? 1.0f : 0.0f));
      }
      ufr[cc][s] = v;
    }
#pragma unroll
    for (int s = 0; s < KX; ++s) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * quad + j;
        v[j] = (__bf16)(W[min(k, Dw - 1) * G4 + ag * H + au] * (k < Dw ? 1.0f : 0.0f));
      }
      wfr[cc][s] = v;
    }
    const int u = unit[cc];
    bias4[cc] = f32x4_t{bias[u], bias[H + u], bias[2 * H + u], bias[3 * H + u]};
  }

  // x loader: every wave streams granule (tid mod n) of the contiguous [16][Din] tile and
  // stages it (identical duplicates across waves). No branch surrounds a memory op: with a
  // predicate around loads hipcc drained vmcnt at the join every step (seen in the ISA).
  const int n_gx = 16 * Din / GR;
  const int gx = (tid % n_gx) * GR;
  const int gx_seq = gx / Din, gx_k = gx % Din;
  const float* xbase = x + (size_t)row0 * Din + gx;
  const size_t xstep = (size_t)Mp * Din;
  Granule<GR> xr[D];
  // h storer: every wave stores granule (tid mod n) of the [16][H] tile; a step without an
  // h to store writes the scratch time row T.
  constexpr int n_gh = 16 * H / 4;
  const int gh = (tid % n_gh) * 4;
  float* hbase = hout + (size_t)row0 * H + gh;
  const size_t hstep = (size_t)Mp * H;

#pragma unroll
  for (int j = 0; j < D; ++j) xr[j].load(xbase + (size_t)min(j, T - 1) * xstep);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < GR; ++q) xs[0][gx_seq][gx_k + q] = (__bf16)xr[0].v[q];
  xr[0].load(xbase + (size_t)min(D, T - 1) * xstep);
  float c[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) c[cc] = 0.f;
  __syncthreads();

  // steps 0 .. T (step T only stores h_{T-1})
  for (int t0 = 0; t0 <= T; t0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int t = t0 + j;
      const int p = t & 1;
      const int jn = (j + 1 == D) ? 0 : j + 1;
      {                                             // h_{t-1}: one contiguous tile
        const int ts = (t >= 1 && t <= T) ? t - 1 : T;
        const float4 v = *reinterpret_cast<const float4*>(&hf[p ^ 1][gh / H][gh % H]);
        *reinterpret_cast<float4*>(hbase + (size_t)ts * hstep) = v;
      }
      f32x4_t acc[CPL];
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc) {
        // x and h parts in independent accumulators: their MFMA chains overlap instead of
        // the h part waiting for the x part's result
        f32x4_t accx = bias4[cc], acch = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KX; ++s) {
          const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(&xs[p][col][32 * s + 8 * quad]);
          accx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[cc][s], bx, accx, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < C::KSH; ++s) {
          const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(&hs[p][col][32 * s + 8 * quad]);
          acch = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[cc][s], bh, acch, 0, 0, 0);
        }
        acc[cc] = accx + acch;
      }
      // stage x_{t+1}, refill the slot with x_{t+1+D}
#pragma unroll
      for (int q = 0; q < GR; ++q) xs[p ^ 1][gx_seq][gx_k + q] = (__bf16)xr[jn].v[q];
      xr[jn].load(xbase + (size_t)min(t + 1 + D, T - 1) * xstep);
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc) {
        const float iv = sigmoidf_fast(acc[cc][0]);
        const float fv = sigmoidf_fast(acc[cc][1]);
        const float gv = tanhf_fast(acc[cc][2]);
        const float ov = sigmoidf_fast(acc[cc][3]);
        c[cc] = fv * c[cc] + iv * gv;
        const float hv = ov * tanhf_fast(c[cc]);
        const int u = unit[cc];
        hs[p ^ 1][col][u] = (__bf16)hv;
        hf[p][col][u] = hv;
        if constexpr (TRAIN) {                       // steps past T-1 write the scratch row T
          const size_t o = ((((size_t)min(t, T) * ntiles + tile) * NW + w) * CPL + cc) * 64 + lane;
          if constexpr (SG) *reinterpret_cast<uint2*>(gbuf + o * 4) = gates_pack(iv, fv, gv, ov);
          if constexpr (!SG && TM_RG_BF16C) reinterpret_cast<__bf16*>(cbuf)[o] = (__bf16)c[cc];
          else cbuf[o] = c[cc];
        }
      }
      lds_barrier();
    }
  }
}

// =====================================================================================
// forward of a layer PAIR (layer A: Din -> H, layer B: H -> H, both return_sequences),
// wavefront-pipelined inside one workgroup: waves [0, NW) run layer A at step s while waves
// [NW, 2 NW) run layer B at step s - 1, fed from A's bf16 h tile in LDS (no HBM round trip,
// no second launch). One LDS barrier per step for both layers, so the pair costs ~one
// recurrence of T + 1 steps instead of two of T. Outputs and saved state are exactly those
// of two lstm_tm_fwd_kernel launches (same bf16 operands, same accumulation order).
// (The reference stacks time1/time2 and time_layers[2i]/[2i+1], libs/create_model.py:61-79.)
// PL: MaxPooling1D(P) of layer B's output in the same launch - the storer lanes of layer B keep a
// running max + byte argmax of their h granule (PoolAcc) and write the pooled tile and its argmax
// when a window closes (the maxpool1d_fwd pass over hB is gone; hB itself is still stored for the
// backward)
template <int H, bool TRAIN, int KX, int GR, int D, bool SG = true, bool PL = false>
__global__ __launch_bounds__(2 * TMC<H>::NT, (TmOcc<2 * TMC<H>::NT, KX>::W)) void lstm_tm2_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ WA, const float* __restrict__ UA,
    const float* __restrict__ bA, const float* __restrict__ WB, const float* __restrict__ UB,
    const float* __restrict__ bB, float* __restrict__ hA, __bf16* __restrict__ gA, float* __restrict__ cA,
    float* __restrict__ hB, __bf16* __restrict__ gB, float* __restrict__ cB, int Mp, int T, int Din, int Dw,
    int P = 0, float* __restrict__ pout = nullptr, unsigned* __restrict__ iout = nullptr) {
  using C = TMC<H>;
  static_assert(C::CPL == 1, "pair kernel: one cell per lane (H <= 64)");
  constexpr int NW = C::NW, NTL = C::NT, G4 = C::G4;
  constexpr int KPX = 32 * KX;
  constexpr int KS = C::KSH;                       // K steps over an H-wide operand
  constexpr int KW = KX > KS ? KX : KS;
  // [layer][parity]: indexed (not pointer-selected) so every access stays a DS instruction
  __shared__ __attribute__((aligned(16))) __bf16 hs[2][2][16][C::KPH + 8];
  __shared__ __attribute__((aligned(16))) __bf16 xs[2][16][KPX + 8];
  __shared__ __attribute__((aligned(16))) float hf[2][2][16][C::HP];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool layerB = wv >= NW;                     // SGPR: branches on it are scalar
  const int L = layerB ? 1 : 0;
  const int w = layerB ? wv - NW : wv;
  const int tl = tid - (layerB ? NTL : 0);          // thread index within the layer
  const int col = lane & 15, quad = lane >> 4;
  const int tile = blockIdx.x, ntiles = gridDim.x, row0 = tile * 16;

  for (int i = tid; i < 2 * 2 * 16 * (C::KPH + 8); i += 2 * NTL) (&hs[0][0][0][0])[i] = (__bf16)0.0f;
  for (int i = tid; i < 2 * 16 * (KPX + 8); i += 2 * NTL) (&xs[0][0][0])[i] = (__bf16)0.0f;

  // A fragments (rows permuted as in lstm_tm_fwd_kernel): U and W of this wave's layer
  const float* Ul = layerB ? UB : UA;
  const float* Wl = layerB ? WB : WA;
  const float* bl = layerB ? bB : bA;
  const int Dl = layerB ? H : Dw;                   // rows of this layer's W
  bf16x8_t ufr[KS], wfr[KW];
  const int au = 4 * w + (col >> 2), ag = col & 3;
  const int unit = 4 * w + quad;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    bf16x8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * s + 8 * quad + j;
      v[j] = (__bf16)(Ul[min(k, H - 1) * G4 + ag * H + au] * (k < H ? 1.0f : 0.0f));
    }
    ufr[s] = v;
  }
#pragma unroll
  for (int s = 0; s < KW; ++s) {
    bf16x8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * s + 8 * quad + j;
      v[j] = (__bf16)(Wl[min(k, Dl - 1) * G4 + ag * H + au] * (k < Dl ? 1.0f : 0.0f));
    }
    wfr[s] = v;
  }
  const f32x4_t bias4 = f32x4_t{bl[unit], bl[H + unit], bl[2 * H + unit], bl[3 * H + unit]};

  // x loader (all threads, granule tid mod n; duplicates are identical) and h storers
  const int n_gx = 16 * Din / GR;
  const int gx = (tid % n_gx) * GR;
  const int gx_seq = gx / Din, gx_k = gx % Din;
  const float* xbase = x + (size_t)row0 * Din + gx;
  const size_t xstep = (size_t)Mp * Din;
  Granule<GR> xr[D];
  constexpr int n_gh = 16 * H / 4;
  const int gh = (tl % n_gh) * 4;
  float* hbase = (layerB ? hB : hA) + (size_t)row0 * H + gh;
  // recompute-gates pairs (training without saved gates) store layer A's h in bf16: its readers are this
  // pair's backward (B's x stream, A's h_{t-1} stream), which stage it as bf16 MFMA operands anyway
  constexpr bool HBA = TRAIN && !SG && TM_RG_BF16H;
  __bf16* hbaseA = reinterpret_cast<__bf16*>(hA) + (size_t)row0 * H + gh;
  const size_t hstep = (size_t)Mp * H;
  __bf16* gbuf = layerB ? gB : gA;
  float* cbuf = layerB ? cB : cA;
  PoolAcc pacc{};
  const bool pooler = PL && layerB && wave_uniform(tl < n_gh);
  const int To = PL ? T / P : 0;
#pragma unroll
  for (int j = 0; j < D; ++j) xr[j].load(xbase + (size_t)min(j, T - 1) * xstep);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < GR; ++q) xs[0][gx_seq][gx_k + q] = (__bf16)xr[0].v[q];
  xr[0].load(xbase + (size_t)min(D, T - 1) * xstep);
  float c = 0.f;
  __syncthreads();

  // steps 0 .. T+1: A computes t = s (s < T), B computes t = s - 1 (1 <= s <= T); each layer
  // stores the h tile of its previous step (A: s - 1, B: s - 2; invalid -> scratch row T)
  for (int t0 = 0; t0 <= T + 1; t0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int s = t0 + j;
      const int p = s & 1;
      const int jn = (j + 1 == D) ? 0 : j + 1;
      const int tc = layerB ? s - 1 : s;             // time step this layer computes
      {
        const int ts = (tc >= 1 && tc <= T) ? tc - 1 : T;
        const float4 v = *reinterpret_cast<const float4*>(&hf[L][p ^ 1][gh / H][gh % H]);
        if (HBA && !layerB)                        // (uniform) layer A's h in bf16, TM_RG_BF16H
          *reinterpret_cast<bf16x4_t*>(hbaseA + (size_t)ts * hstep) =
              bf16x4_t{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
        else
          *reinterpret_cast<float4*>(hbase + (size_t)ts * hstep) = v;
        if constexpr (PL) {
          if (pooler && ts < T) pacc.step(v, ts, P, To, pout, iout, (size_t)row0 * H + gh, hstep);
        }
      }
      f32x4_t accx = bias4, acch = {0.f, 0.f, 0.f, 0.f};   // independent MFMA chains
      if (layerB) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(&hs[0][p][col][32 * k + 8 * quad]);
          accx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[k], bx, accx, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int k = 0; k < KX; ++k) {
          const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(&xs[p][col][32 * k + 8 * quad]);
          accx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[k], bx, accx, 0, 0, 0);
        }
      }
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(&hs[L][p][col][32 * k + 8 * quad]);
        acch = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[k], bh, acch, 0, 0, 0);
      }
      const f32x4_t acc = accx + acch;
      // stage x_{s+1}, refill the slot with x_{s+1+D}
#pragma unroll
      for (int q = 0; q < GR; ++q) xs[p ^ 1][gx_seq][gx_k + q] = (__bf16)xr[jn].v[q];
      xr[jn].load(xbase + (size_t)min(s + 1 + D, T - 1) * xstep);
      {
        // branch-free (a branch here makes the compiler drain the x prefetch ring at the join):
        // B's step s = 0 is masked to keep c = 0, h = 0
        const float m = tc >= 0 ? 1.f : 0.f;
        const float iv = sigmoidf_fast(acc[0]);
        const float fv = sigmoidf_fast(acc[1]);
        const float gv = tanhf_fast(acc[2]);
        const float ov = sigmoidf_fast(acc[3]);
        c = (fv * c + iv * gv) * m;
        const float hv = ov * tanhf_fast(c) * m;
        hs[L][p ^ 1][col][unit] = (__bf16)hv;
        hf[L][p][col][unit] = hv;
        if constexpr (TRAIN) {                       // invalid steps write the scratch row T
          const size_t o = (((size_t)(tc >= 0 ? min(tc, T) : T) * ntiles + tile) * NW + w) * 64 + lane;
          if constexpr (SG) *reinterpret_cast<uint2*>(gbuf + o * 4) = gates_pack(iv, fv, gv, ov);
          if constexpr (!SG && TM_RG_BF16C) reinterpret_cast<__bf16*>(cbuf)[o] = (__bf16)c;
          else cbuf[o] = c;
        }
      }
      lds_barrier();
    }
  }
}

// =====================================================================================
// host side
// (MaxPooling1D fused into the single-layer recurrences - running max + argmax in the forward, un-pooling on
// load in the backward - was measured slower on both shapes: CML 0.766 vs 0.713 ms, SoilNet 3.920 vs
// 3.894 ms; profiles/r3_bench_soilnet_poolfusion.json. Pooling runs as pool.hip kernels.)
constexpr int TM_FWD_D = 6;      // ring depth (steps) of the x stream

// x: [T, Mp, Din] time-major; W: [Dw, 4H] with Dw <= Din (x channels >= Dw must be zero, e.g. the
// alignment padding of a 19-channel input to 20). Returns [h (T,Mp,H), gates (state), c (state)].
// store_gates = false (train): the gates state is empty and the backward recomputes the gates
// (lstm_tm_bwd with an empty g; H <= 32, 16-byte x granules: tm_rg_ok).
std::vector<at::Tensor> lstm_tm_fwd(const at::Tensor& x, const at::Tensor& W, const at::Tensor& U,
                                    const at::Tensor& b, bool train, bool store_gates) {
  check_f32_cuda(x, "x");
  check_f32_cuda(W, "W");
  check_f32_cuda(U, "U");
  check_f32_cuda(b, "b");
  TORCH_CHECK(x.dim() == 3, "lstm_tm_fwd: x must be [T, Mp, Din]");
  const int T = (int)x.size(0), Mp = (int)x.size(1), Din = (int)x.size(2), H = (int)U.size(0);
  TORCH_CHECK(Mp % 16 == 0 && Mp > 0 && T > 0, "lstm_tm_fwd: Mp must be a positive multiple of 16");
  const int Dw = (int)W.size(0);
  TORCH_CHECK(U.size(1) == 4 * H && Dw >= 1 && Dw <= Din && W.size(1) == 4 * H && b.numel() == 4 * H,
              "lstm_tm_fwd: weight shapes");
  const int gr = tm_granule(Din, x.data_ptr());
  TORCH_CHECK(tm_supported(H, Din, gr), "lstm_tm_fwd: unsupported (H, Din) = (", H, ", ", Din, ")");
  TORCH_CHECK(store_gates || !train || tm_rg_ok(H, gr), "lstm_tm_fwd: recomputed gates need H <= 32, Din % 4 == 0");
  c10::DeviceGuard guard(x.device());
  auto opt = x.options();
  // one extra (scratch) time row: stores of steps that have nothing to store land there
  at::Tensor h = at::empty({T + 1, Mp, H}, opt);
  at::Tensor g = (train && store_gates) ? at::empty({T + 1, Mp, H, 4}, opt.dtype(at::kBFloat16))
                                        : at::empty({0}, opt.dtype(at::kBFloat16));
  const bool cbf = train && !store_gates && TM_RG_BF16C;     // (recompute-gates c in bf16)
  at::Tensor c = train ? at::empty({T + 1, Mp, H}, cbf ? opt.dtype(at::kBFloat16) : opt) : at::empty({0}, opt);
  const int ntiles = Mp / 16;
  auto st = stream();
  __bf16* gp = (train && store_gates) ? bf16_ptr(g) : nullptr;
  float* cp = train ? reinterpret_cast<float*>(c.data_ptr()) : nullptr;
  tm_dispatch<16, 32, 64>(H, Din, gr, "lstm_tm: hidden size must be 16, 32 or 64", [&](auto hc, auto kxc, auto grc) {
    constexpr int HH = decltype(hc)::value, KX = decltype(kxc)::value, GR = decltype(grc)::value;
    // SG = false: training with a recompute-gates backward, c only
    dispatch_bools([&](auto trc, auto sgc) {
      constexpr bool TRAIN = decltype(trc)::value, SG = decltype(sgc)::value;
      if constexpr (SG || (TRAIN && tm_rg_ok(HH, GR)))
        hipLaunchKernelGGL((lstm_tm_fwd_kernel<HH, TRAIN, KX, GR, TM_FWD_D, SG>), dim3(ntiles), dim3(TMC<HH>::NT), 0,
                           st, x.data_ptr<float>(), W.data_ptr<float>(), U.data_ptr<float>(), b.data_ptr<float>(),
                           h.data_ptr<float>(), gp, cp, Mp, T, Din, Dw);
      else
        TORCH_CHECK(false, "lstm_tm_fwd: recomputed gates need H <= 32, Din % 4 == 0");
    }, train, !train || store_gates);
  });
  GQ_LAUNCH_CHECK();
  return {h.narrow(0, 0, T), g, c};
}

// Pair forward (lstm_tm2_fwd_kernel): x [T, Mp, Din]; A: W [Dw <= Din, 4H], B: W [H, 4H].
// Returns [hA, gA, cA, hB, gB, cB] with the layouts of lstm_tm_fwd.
// pool > 0: MaxPooling1D(pool) of hB in the same launch; two more outputs [pooled (T/pool, Mp, H), argmax
// bytes (same shape)]
std::vector<at::Tensor> lstm_tm2_fwd(const at::Tensor& x, const at::Tensor& WA, const at::Tensor& UA,
                                     const at::Tensor& bA, const at::Tensor& WB, const at::Tensor& UB,
                                     const at::Tensor& bB, bool train, bool store_gates, int64_t pool) {
  for (const at::Tensor* t : {&x, &WA, &UA, &bA, &WB, &UB, &bB}) check_f32_cuda(*t, "lstm_tm2_fwd operand");
  TORCH_CHECK(x.dim() == 3, "lstm_tm2_fwd: x must be [T, Mp, Din]");
  const int T = (int)x.size(0), Mp = (int)x.size(1), Din = (int)x.size(2), H = (int)UA.size(0);
  const int Dw = (int)WA.size(0);
  TORCH_CHECK(Mp % 16 == 0 && Mp > 0 && T > 0, "lstm_tm2_fwd: Mp must be a positive multiple of 16");
  TORCH_CHECK(UA.size(1) == 4 * H && Dw >= 1 && Dw <= Din && WA.size(1) == 4 * H && bA.numel() == 4 * H,
              "lstm_tm2_fwd: layer A weight shapes");
  TORCH_CHECK(UB.size(0) == H && UB.size(1) == 4 * H && WB.size(0) == H && WB.size(1) == 4 * H && bB.numel() == 4 * H,
              "lstm_tm2_fwd: layer B must be H -> H with the same H");
  const int gr = tm_granule(Din, x.data_ptr());
  TORCH_CHECK(H <= 32 && tm_supported(H, Din, gr), "lstm_tm2_fwd: unsupported (H, Din) = (", H, ", ", Din, ")");
  TORCH_CHECK(store_gates || !train || tm_rg_ok(H, gr), "lstm_tm2_fwd: recomputed gates need Din % 4 == 0");
  const bool sg = train && store_gates;
  c10::DeviceGuard guard(x.device());
  auto opt = x.options();
  auto mk = [&](bool state, int last) {
    return state ? (train ? at::empty({T + 1, Mp, H, last}, opt) : at::empty({0}, opt)) : at::empty({T + 1, Mp, H}, opt);
  };
  at::Tensor hA = (train && !sg && TM_RG_BF16H) ? at::empty({T + 1, Mp, H}, opt.dtype(at::kBFloat16)) : mk(false, 0);
  at::Tensor hB = mk(false, 0);
  at::Tensor gA = sg ? at::empty({T + 1, Mp, H, 4}, opt.dtype(at::kBFloat16)) : at::empty({0}, opt.dtype(at::kBFloat16));
  at::Tensor gB = sg ? at::empty({T + 1, Mp, H, 4}, opt.dtype(at::kBFloat16)) : at::empty({0}, opt.dtype(at::kBFloat16));
  const bool cbf = train && !sg && TM_RG_BF16C;              // (recompute-gates c in bf16)
  const auto copt = cbf ? opt.dtype(at::kBFloat16) : opt;
  at::Tensor cA = train ? at::empty({T + 1, Mp, H}, copt) : at::empty({0}, opt);
  at::Tensor cB = train ? at::empty({T + 1, Mp, H}, copt) : at::empty({0}, opt);
  const int ntiles = Mp / 16;
  auto st = stream();
  __bf16* gAp = sg ? bf16_ptr(gA) : nullptr;
  __bf16* gBp = sg ? bf16_ptr(gB) : nullptr;
  float* cAp = train ? reinterpret_cast<float*>(cA.data_ptr()) : nullptr;
  float* cBp = train ? reinterpret_cast<float*>(cB.data_ptr()) : nullptr;
  at::Tensor pooled, pidx;
  const TmPool pl = tm_pool_outputs((int)pool, T, Mp, H, opt, pooled, pidx);
  // layer pairs run 2 x H/4 waves in one workgroup: H <= 32
  tm_dispatch<16, 32>(H, Din, gr, "lstm_tm2: hidden size must be 16 or 32", [&](auto hc, auto kxc, auto grc) {
    constexpr int HH = decltype(hc)::value, KX = decltype(kxc)::value, GR = decltype(grc)::value;
    dispatch_bools([&](auto trc, auto sgc, auto plc) {
      constexpr bool TRAIN = decltype(trc)::value, SG = decltype(sgc)::value, PL = decltype(plc)::value;
      if constexpr (SG || (TRAIN && tm_rg_ok(HH, GR)))
        hipLaunchKernelGGL((lstm_tm2_fwd_kernel<HH, TRAIN, KX, GR, TM_FWD_D, SG, PL>), dim3(ntiles),
                           dim3(2 * TMC<HH>::NT), 0, st, x.data_ptr<float>(), WA.data_ptr<float>(),
                           UA.data_ptr<float>(), bA.data_ptr<float>(), WB.data_ptr<float>(), UB.data_ptr<float>(),
                           bB.data_ptr<float>(), reinterpret_cast<float*>(hA.data_ptr()), gAp, cAp,
                           hB.data_ptr<float>(), gBp, cBp, Mp, T, Din, Dw, pl.P, pl.out, pl.idx);
      else
        TORCH_CHECK(false, "lstm_tm2_fwd: recomputed gates need Din % 4 == 0");
    }, train, !train || store_gates, pl.P > 0);
  });
  GQ_LAUNCH_CHECK();
  return {hA.narrow(0, 0, T), gA, cA, hB.narrow(0, 0, T), gB, cB, pooled, pidx};
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("lstm_tm_fwd", &gq::lstm_tm_fwd);
  m.impl("lstm_tm2_fwd", &gq::lstm_tm2_fwd);
}
