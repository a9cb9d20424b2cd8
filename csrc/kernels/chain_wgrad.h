// Weight-gradient epilogue of the backward chain's upper workgroups (lstm_chain_bwd.hip): after its reverse loop the
// workgroup of (layer, tile) - an H = 32 / 64 chain stage or time4 - builds the dW | db and dU partial of its
// own 16 sequences over all T steps of the layer and writes it as ONE split record in GradsGeom's layout
// (lstm_grads_body.h), record index = tile. The layer's reduction (lstm_grads_reduce_multi_kernel) then runs
// unchanged with splits = ntiles. Those workgroups are done 30 - 60 us into a launch that the two H = 16
// stages hold open for ~100 us, their dz is their own and x / h lie in HBM since the forward; the H = 16 stages
// are the critical path and keep their jobs in the tail launch (lstm_grads_multi).
//
// It is lstm_grads_body with another row tile: one MFMA K tile = 2 time steps x the tile's 16 sequences,
// K index k = 2 * sequence + (step & 1), i.e. rows (2p) Mp + 16 tile + k / 2 and (2p + 1) Mp + 16 tile + k / 2
// of the time-major arrays; h_{t-1} lies Mp rows back (zero at t = 0); the second step of the last pair is
// masked when T is odd. A 256-thread wave group owns one 64-gate-unit column block, the groups of a workgroup
// share the [x | 1] and h_{t-1} images; 4 H / 64 column blocks run side by side, time4's 8 in two passes.
// Nobody waits for another workgroup.
#pragma once
#include "lstm_grads_body.h"

namespace gq {

// the job of one backward chain workgroup row (kernel argument, ChainBArgs::wj)
struct ChainWJob {
  const float* x;                    // the layer's input rows [T Mp][ldx], time-major
  const float* h;                    // the layer's output [T][Mp][H]
  const __bf16* dz;                  // [T + 1][Mp][4H]: the stage's own dz
  float* ws;                         // ntiles split records (GradsGeom(H, Din).RC floats each)
  long x_elems;                      // floats readable from x
  int ldx, T, Din, on;               // Din: rows of W (channels >= Din of x are not read); on: 0 = no epilogue
};

constexpr int CW_DTM = 5;            // din tiles (incl. the bias row) at most: Din <= 64

template <int H>
struct ChainWLds {
  static constexpr int NCB = 4 * H / GR_CB;              // column blocks of the layer
  static constexpr int NG = NCB < 4 ? NCB : 4;           // wave groups side by side
  static constexpr int DZT = NG * GR_CB * GR_LDR * 2;    // dz^T  [NG 64 gate-units][k]
  static constexpr int XT = CW_DTM * 16 * GR_LDR * 2;    // [x|1]^T [din][k]
  static constexpr int HT = H * GR_LDR * 2;              // h_{t-1}^T [unit][k]
  static constexpr int BYTES = DZT + XT + HT;
};

// Called by every live thread of the workgroup (threads past 256 NG only keep the barriers' count). The caller
// has drained the workgroup's dz stores and made them visible to its own loads (a __syncthreads()).
template <int H>
__device__ __forceinline__ void chain_wgrad_body(const float* __restrict__ x, const float* __restrict__ hseq,
                                                 const __bf16* __restrict__ dz, float* __restrict__ ws, long x_elems,
                                                 int ldx, int T, int Dw, int Mp, int tile, char* __restrict__ smem) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  using L = ChainWLds<H>;
  constexpr int G4 = 4 * H, HT = H / 16, NCB = L::NCB, NG = L::NG, NPASS = NCB / NG, NTH = 256 * NG;
  constexpr int NHI = 16 * H / 4;                        // h_{t-1} items (sequence, unit quad)
  static_assert(NCB % NG == 0 && 16 * 16 + NHI <= NTH && L::DZT % 16 == 0 && L::XT % 16 == 0, "chain wgrad tiling");
  auto dzT = reinterpret_cast<__bf16 (*)[GR_LDR]>(smem);
  auto xT = reinterpret_cast<__bf16 (*)[GR_LDR]>(smem + L::DZT);      // hT follows it: one image [80 + H][k]
  auto hT = reinterpret_cast<__bf16 (*)[GR_LDR]>(smem + L::DZT + L::XT);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool act = wv < 4 * NG;                          // wave-uniform
  const int g = wv >> 2, wl = wv & 3;                    // wave group (column block of the pass), wave in it
  const int col = lane & 15, quad = lane >> 4;
  const int DT = (Dw + 1 + 15) / 16;
  const int npairs = (T + 1) / 2;
  const int seq0 = 16 * tile;

  // dz item: sequence zr, gate-unit quad zq of the pass's NG 64 gate-units, both steps of the pair
  const int zq = tid % (NG * 16), zr = min(tid / (NG * 16), 15);
  const size_t zstep = (size_t)Mp * G4;
  const __bf16* zb = dz + (size_t)(seq0 + zr) * G4 + 4 * zq;
  // x / h_{t-1} item: threads [0, 16 nq) stage x (sequence, channel quad), the last NHI threads h_{t-1}
  // (sequence, unit quad); the ranges are disjoint. One form for both: rows `st` floats apart per step, the
  // h rows one step back, the image rows ch0 .. ch0 + 3 of the [x | 1 | h] image
  const int nq = (Dw + 3) / 4;
  const bool isx = tid < 16 * nq, ish = act && tid >= NTH - NHI;
  const int hi = max(tid - (NTH - NHI), 0);
  const int ir = isx ? tid / nq : hi / (H / 4), iq = isx ? tid % nq : hi % (H / 4);
  const long st = isx ? (long)Mp * ldx : (long)Mp * H;
  const float* ib = isx ? x : hseq;
  const long i0 = isx ? (long)(seq0 + ir) * ldx + 4 * iq : (long)(seq0 + ir) * H + 4 * iq;
  const long ilast = isx ? (x_elems - 4) / 4 * 4 : (long)T * Mp * H - 4;   // (a strided x view may end early)
  const int ioff = isx ? 0 : -1;
  const int nch = isx ? min(4, Dw - 4 * iq) : 4;         // channels of the quad that exist
  __bf16* idst = &xT[(isx ? 0 : CW_DTM * 16) + 4 * iq][2 * ir];

  if (act)
    for (int e = tid; e < CW_DTM * 16 * GR_LDR; e += NTH) (&xT[0][0])[e] = (__bf16)0.f;   // channels > Dw stay 0

  for (int ps = 0; ps < NPASS; ++ps) {
    f32x4_t accW[CW_DTM], accU[HT];
#pragma unroll
    for (int d = 0; d < CW_DTM; ++d) accW[d] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < HT; ++k) accU[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const __bf16* zp = zb + ps * NG * GR_CB;
    // ---- per-pair register images (prefetch ring of depth 1)
    uint2 rz[2];
    float4 ri[2];
    auto load_pair = [&](int p) {
      rz[0] = *reinterpret_cast<const uint2*>(zp + (size_t)(2 * p) * zstep);
      rz[1] = *reinterpret_cast<const uint2*>(zp + (size_t)min(2 * p + 1, T - 1) * zstep);
      if (isx || ish) {
        const long o0 = (long)max(2 * p + ioff, 0) * st, o1 = (long)min(2 * p + 1 + ioff, T - 1) * st;
        ri[0] = *reinterpret_cast<const float4*>(ib + min(i0 + o0, ilast));
        ri[1] = *reinterpret_cast<const float4*>(ib + min(i0 + o1, ilast));
      }
    };
    auto stage_pair = [&](int p) {
      const bool v1 = 2 * p + 1 < T;                     // the pair's second step exists
      {
        // packed (k = 2 zr, 2 zr + 1) bf16x2 per gate-unit; a masked step stages zeros (select: the row
        // read in its place holds another step's values)
        const unsigned a[4] = {rz[0].x << 16, rz[0].x & 0xffff0000u, rz[0].y << 16, rz[0].y & 0xffff0000u};
        const unsigned b[4] = {rz[1].x << 16, rz[1].x & 0xffff0000u, rz[1].y << 16, rz[1].y & 0xffff0000u};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<unsigned*>(&dzT[4 * zq + j][2 * zr]) = (a[j] >> 16) | (v1 ? b[j] : 0u);
      }
      if (isx || ish) {
        const bool v0 = 2 * p + ioff >= 0;               // h_{t-1} of t = 0 is zero
        const float a[4] = {ri[0].x, ri[0].y, ri[0].z, ri[0].w};
        const float b[4] = {ri[1].x, ri[1].y, ri[1].z, ri[1].w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nch)
            *reinterpret_cast<bf16x2_t*>(idst + j * GR_LDR) = bf16x2_t{(__bf16)(v0 ? a[j] : 0.f), (__bf16)(v1 ? b[j] : 0.f)};
      }
      if (tid < 16) *reinterpret_cast<bf16x2_t*>(&xT[Dw][2 * tid]) = bf16x2_t{(__bf16)1.f, (__bf16)(v1 ? 1.f : 0.f)};   // bias channel
    };

    if (act) load_pair(0);
    for (int p = 0; p < npairs; ++p) {
      lds_barrier();                                     // the previous pair's LDS reads are done
      if (act) {
        stage_pair(p);
        load_pair(min(p + 1, npairs - 1));               // prefetch (the last one is a harmless reload)
      }
      lds_barrier();
      if (act) {
        const bf16x8_t az = *reinterpret_cast<const bf16x8_t*>(&dzT[GR_CB * g + 16 * wl + col][8 * quad]);
#pragma unroll
        for (int d = 0; d < CW_DTM; ++d) {
          if (d < DT) {                                  // uniform
            const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(&xT[16 * d + col][8 * quad]);
            accW[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bx, accW[d], 0, 0, 0);
          }
        }
#pragma unroll
        for (int k = 0; k < HT; ++k) {
          const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(&hT[16 * k + col][8 * quad]);
          accU[k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bh, accU[k], 0, 0, 0);
        }
      }
    }
    // ---- this tile's record of column block ps NG + g, fragment order (float4 per lane)
    if (act) {
      float* rec = ws + ((size_t)tile * NCB + ps * NG + g) * (size_t)(DT + HT) * 1024;
#pragma unroll
      for (int d = 0; d < CW_DTM; ++d)
        if (d < DT) *reinterpret_cast<f32x4_t*>(rec + ((size_t)(d * 4 + wl) * 64 + lane) * 4) = accW[d];
#pragma unroll
      for (int k = 0; k < HT; ++k) *reinterpret_cast<f32x4_t*>(rec + ((size_t)((DT + k) * 4 + wl) * 64 + lane) * 4) = accU[k];
    }
  }
}

}  // namespace gq
