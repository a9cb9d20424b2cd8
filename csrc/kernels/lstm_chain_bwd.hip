// Backward of the LSTM chain (lstm_chain_fwd.hip; the hand-off protocol: lstm_chain_common.h): the
// layers' reverse recurrences, top layer first. Stage k's dx (the
// gradient of the layer below's output, un-pooled by the CONSUMER with the forward's argmax
// bytes when a MaxPooling1D sits between them) is handed off as granules like the forward's
// h; every stage also writes its dz [T+1][Mp][4H] for the weight-gradient pass. The last
// stage writes its dx as plain fp32 (the GCN backward's input).
#include "chain_head.h"
#include "chain_wgrad.h"
#include "lstm_grads_body.h"
#include "lstm_chain_common.h"
#include "lstm_tm_common.h"

namespace gq {

struct ChainBStage {
  const float* dh;                   // stage 0: fp32 gradient of the layer's (pooled) output [Ts][Mp][H]
  const unsigned long long* din;     // stages > 0: tagged dx stream of the stage above [Ts][Mp][H]
  const unsigned char* pidx;         // P > 0: argmax bytes of the pool after this layer [Ts][Mp][H]
  const __bf16* g;
  const float* c;
  const float* W;
  const float* U;
  __bf16* dz;                        // [T+1][Mp][4H] bf16 (the exact MFMA operand values)
  unsigned long long* sout;          // tagged dx stream [T+1][Mp][Din] (nullptr: last stage)
  float* dx;                         // last stage: fp32 dx [T][Mp][Din]
  long long* trace_mid;              // profiling: time the step loop starts
  long long* prof;                   // profiling (GNNQC_CHAIN_PROF=1): tile 0's per-step phase clocks
  // Unused, always zero: the arguments of the retired producer-side un-pooling (profiles/README.md).
  // They and the kernel's punp test stay for now: without them the kernel-argument layout shifts, and
  // that build measured 0.2374 against 0.2343 ms/step on one box (profiles/chain_variant_retirement.txt)
  const unsigned char* uidx;
  int uP, uT, punp;
  int H, T, Din, Dw, KX, P, Ts;
};

// time4's backward (with the head backward and the loss gradient as its prologue) as the first
// stage of the backward launch (lstm_chain_head_bwd): it publishes dx - the gradient of the
// chain's pooled top output - as granules, so the top chain stage starts after time4's first
// reverse step instead of after the whole time4_head_bwd launch (~26 us).
struct ChainT4B {
  const float* h;                    // time4's h [T][Mp][128] (h_{T-1} feeds the head)
  const float* g;                    // saved gates, fp32 (time4_head.hip t4_sidx layout)
  const float* c;                    // saved (c_t, c_{t-1})
  const bf16x8_t* pk;                // the forward's fragment image of (W, U) (lstm_chain_head_fwd)
  const float* hb;                   // the forward's dh_{T-1} tiles for dL/dloss = 1 (ChainT4::hb) or nullptr
  __bf16* dz;                        // [T+1][Mp][512] bf16 (the weight-gradient pass's input)
  unsigned long long* sout;          // dx granule stream [T][Mp][Din]
  int T, Din, Dw, on;
  ChainHead hd;
};

struct ChainBArgs {
  ChainBStage st[CHAIN_MAX];
  int ns, ntiles, nt8, Mp;
  int* ctl;
  long long* trace;
  ChainT4B t4;                       // t4.on: blocks [ns nt8, (ns + 1) nt8) run time4's backward
  // weight-gradient epilogues (chain_wgrad.h) of stage s / [CHAIN_MAX]: time4. Appended: ChainBStage and the
  // offsets of every field above stay where they were (profiles/chain_variant_retirement.txt)
  ChainWJob wj[CHAIN_MAX + 1];
};
static_assert(sizeof(ChainBArgs) <= 4096, "chain backward kernel arguments");

// LDS pitches of the backward stages (bf16 dz rows G4 + ZPAD, fp32 dx rows 32 KX + XPAD), chosen with
// scripts/lds_model as in lstm_tm_bwd_body.h: with a 32-float dx pitch the dx wave's dx^T stores
// (16 sequences x 4 quads per wave) fell on 2 banks of ds_write_b32's 32 (16-way); 33 leaves 2-way
#ifndef CHAINB_ZPAD
#define CHAINB_ZPAD 16
#endif
#ifndef CHAINB_XPAD
#define CHAINB_XPAD 1
#endif
// H = 16 stages (chain_bwd_stage16): the dz and dh double buffers and the dx wave's dx tiles
template <int KX>
struct ChainBLds16 {
  static constexpr int ZS = 2 * 16 * (4 * 16 + CHAINB_ZPAD) * 2;
  static constexpr int DH = 2 * 16 * TMC<16>::HP * 4;
  static constexpr int DX = 2 * 16 * (32 * KX + CHAINB_XPAD) * 4;
  static constexpr int BYTES = ZS + DH + DX;
};
// H >= 32 stages split the two per-step products over K (chain_bwd_stage_sk): every wave runs a
// full 16-row MFMA tile of dh_rec^T = U dz^T / dx^T = W dz^T over a K slice and the partial tiles
// meet in LDS (dpart / xpart, a second barrier per step). The one-tile-per-wave layout (each wave
// owning its own four units: 12 of every 16 A rows zero) issued 4x the MFMAs and made those stages
// MFMA-pipe bound (H = 64: ~0.4 us of a 1.3 us step in the products alone, measured).
template <int H, int KX>
struct ChainBLdsSK {
  static constexpr int NW = TMC<H>::NW, UT = H / 16, KG = NW / UT, NXB = 2 * KX, KXG = NW / NXB;
  static constexpr int ZS = 2 * 16 * (4 * H + CHAINB_ZPAD) * 2;
  static constexpr int DH = 2 * 16 * TMC<H>::HP * 4;
  static constexpr int DP = KG * 16 * TMC<H>::HP * 4;
  static constexpr int XPP = 32 * KX + 4;              // xpart row pitch
  static constexpr int XP = 2 * KXG * 16 * XPP * 4;
  static constexpr int BYTES = ZS + DH + DP + XP;
};
constexpr int chainb_max(int a, int b) { return a > b ? a : b; }
static constexpr int CHAINB_LDS_STAGE =
    chainb_max(chainb_max(ChainBLds16<1>::BYTES, ChainBLds16<2>::BYTES),
               chainb_max(chainb_max(ChainBLdsSK<32, 1>::BYTES, ChainBLdsSK<32, 2>::BYTES),
                          chainb_max(ChainBLdsSK<64, 1>::BYTES, ChainBLdsSK<64, 2>::BYTES)));

struct ChainT4BLds {
  static constexpr int DHT = 16 * 132 * 4;                 // dh_{T-1} from the head
  static constexpr int ZS = 16 * (512 + 8) * 2;            // bf16 dz tile
  static constexpr int DN = 2 * 16 * 132 * 4;              // dh_rec partials of the two K halves
  static constexpr int DXP = 4 * 16 * 68 * 4;              // dx partials of the four K quarters
  static constexpr int STEP = ZS + DN + DXP;
  static constexpr int HEAD = ChainHeadBwdLds<128>::BYTES; // the head prologue's scratch (same bytes)
  static constexpr int BYTES = DHT + (STEP > HEAD ? STEP : HEAD);
};
static constexpr int CHAINB_LDS = ChainT4BLds::BYTES > CHAINB_LDS_STAGE ? ChainT4BLds::BYTES : CHAINB_LDS_STAGE;
static_assert(ChainWLds<32>::BYTES <= CHAINB_LDS && ChainWLds<64>::BYTES <= CHAINB_LDS &&
                  ChainWLds<128>::BYTES <= CHAINB_LDS, "the weight-gradient epilogue runs in the stages' LDS");

#ifndef CHAINB_LEAD
#define CHAINB_LEAD 1
#endif
#ifndef CHAINB_PUBBATCH
#define CHAINB_PUBBATCH 4    // backward publisher: LDS reads of this many dx elements per lane, then their stores
#endif
#ifndef CHAINB_NPUB
#define CHAINB_NPUB 4        // publisher waves per H <= 32 stage (each publishes every NPUB-th 64-element slice;
                             // same-box chain bwd 156.8 / 136.9 / 133.0 / 130.0 us for 1 / 2 / 3 / 4)
#endif
#ifndef CHAINB_PUBPRIO
#define CHAINB_PUBPRIO 2     // s_setprio of the backward publisher and dz waves (same-box A/B: chain bwd 127.3 -> 124.2 us, bench 0.2626 -> 0.2596 ms)
#endif
#ifndef CHAINB_DXPRIO
#define CHAINB_DXPRIO 2      // s_setprio of the backward dx wave (same-box A/B: chain bwd 124.0 -> 122.2 us, bench 0.2589 -> 0.2562 ms)
#endif
// ring depths (reverse steps of prefetch) per hidden size
#ifndef CHAINB_D16
#define CHAINB_D16 4
#endif
#ifndef CHAINB_D32
#define CHAINB_D32 4
#endif
#ifndef CHAINB_D64
#define CHAINB_D64 2
#endif
// Threads of a backward stage workgroup. Behind the 16 H / 64 compute waves an H <= 32 stage runs
// CHAINB_NPUB publisher waves and, last, the dz wave; an H = 16 stage has the dx wave between them.
// The compute waves of an H = 64 stage fill the workgroup: they store dz and dx themselves.
// (These helpers keep their general form: the kernel calls chainb_live_threads out of line, so a
// simpler body would change the device code.)
__host__ __device__ constexpr bool chainb_dxw(int h) {
  return h < 32 && TMC<16>::NT + 64 * CHAINB_NPUB + 64 <= 1024;
}
// publisher waves of a stage (0: H = 64)
__host__ __device__ constexpr int chainb_npub(int h, int nt) {
  return nt + 64 > 1024 ? 0
       : chainb_max(1, CHAINB_NPUB < (1024 - nt - (chainb_dxw(h) ? 64 : 0) - 64) / 64
                           ? CHAINB_NPUB : (1024 - nt - (chainb_dxw(h) ? 64 : 0) - 64) / 64);
}
__host__ __device__ constexpr bool chainb_dzw(int h, int nt) {
  return chainb_npub(h, nt) > 0 && nt + 64 * chainb_npub(h, nt) + 64 + (chainb_dxw(h) ? 64 : 0) <= 1024;
}
__host__ __device__ constexpr int chainb_live_threads(int h, int nt) {
  return nt + 64 * chainb_npub(h, nt) + (chainb_dxw(h) ? 64 : 0) + (chainb_dzw(h, nt) ? 64 : 0);
}
static_assert(chainb_dxw(16) && chainb_dzw(16, TMC<16>::NT) && chainb_npub(16, TMC<16>::NT) == CHAINB_NPUB &&
                  !chainb_dxw(32) && chainb_dzw(32, TMC<32>::NT) && chainb_npub(32, TMC<32>::NT) == CHAINB_NPUB &&
                  chainb_live_threads(64, TMC<64>::NT) == 1024,
              "wave roles of the backward stages (chain_bwd_stage16, chain_bwd_stage_sk)");

// One H = 16 layer of one tile, reverse in time: lstm_tm_bwd_body (DZ + DX) with one dh element per
// lane from the stage above's stream (or, stage 0, from global memory), un-pooled on load, and dx
// published element-wise.
//
// The bottom layers' T reverse steps are the backward's critical path, so between two barriers only
// what needs dh_rec stays behind the MFMAs, and the hand-off staging runs while LDS reads fly:
//
//   barrier s                      dz(s) is in zs[s & 1], dh(s + 1) in dhs[(s + 1) & 1]
//   ds_read_b128 of dz(s) K-block 0, MFMA as soon as it is there
//   ds_read_b128 of K-block 1 and the read of dh(s + 1)
//     while they fly: dh(s + 2) from its ring slot (tag check, un-pool select) -> dhs[s & 1],
//                     ring load of dh(s + 2 + D)
//   second MFMA: dh_rec = U dz(s)
//     in its shadow: gates of step s + 1 unpacked, tanh(c), every factor that does not need dh_rec
//   dh = dh(s + 1) + dh_rec, dct, dc, four products, bf16, dz(s + 1) -> zs[(s + 1) & 1]
//   state load of step s + 1 + D into the slot just consumed
//
// dhs[s & 1] was last read after barrier s - 1 and is read again after barrier s + 1, so two
// buffers suffice. Steps past the sequence (s >= T, and the un-pooling tail past the last pooling
// window) carry no source granule: they are never waited for and stage a zero. The hoisted
// factors reassociate the cell's products (dct * (g * i * (1 - i)) for ((dct * g) * i) * (1 - i)):
// bf16 rounding flips in dz against the per-layer kernels, nothing else.
// Measured placements (profiles/chain_bwd_h16_pipeline_ab.txt): both K-block reads ahead of the
// first MFMA, tanh(c) ahead of the MFMAs, the state load pinned behind the dz stores or moved into
// the MFMA shadow, chain_wait inlined, a ring of 2 / 3 / 5 / 6 steps: all slower than this order.
// Wave-uniform cursors replace the per-step address products: the saved state and the dh source
// are walked one step at a time, and every load is a fixed base, a 32-bit step offset and a lane
// offset (the arrays of an H = 16 stage stay below 4 GiB: lstm_chain_bwd checks it).
//
// dx^T = W dz^T is the dx wave's, not the compute waves' (between the step's MFMA and the next cell
// phase it sat on the recurrence's path).
template <int KX, int D, bool SRC, bool UP, bool XO>
__device__ __forceinline__ void chain_bwd_stage16(const ChainBStage S, int tile, int ntiles, int Mp, unsigned tagb,
                                                  int* ctl, char* smem) {
  constexpr int H = 16;
  using C = TMC<H>;
  constexpr int NW = C::NW, NT = C::NT, G4 = C::G4, KB = C::KB;
  constexpr int NXB = KX * 2;
  constexpr int NPUB = CHAINB_NPUB;
  static_assert(C::CPL == 1 && 16 * H == NT && KB == 2, "one dh element per lane, two K blocks of dz");
  static_assert(D >= 2, "H = 16 stage: ring of at least two steps");
  using L = ChainBLds16<KX>;
  static_assert(L::BYTES <= CHAINB_LDS_STAGE && L::ZS % 16 == 0 && L::DH % 16 == 0, "chain bwd LDS layout");
  auto zs = reinterpret_cast<__bf16 (*)[16][G4 + CHAINB_ZPAD]>(smem);
  auto dhs = reinterpret_cast<float (*)[16][C::HP]>(smem + L::ZS);
  auto dxs = reinterpret_cast<float (*)[16][32 * KX + CHAINB_XPAD]>(smem + L::ZS + L::DH);

  const int T = S.T, Din = S.Din, Dw = S.Dw, P = S.P, Ts = S.Ts;
  // source kind and un-pooling are template parameters: with run-time branches around the
  // ring loads the compiler drained the whole prefetch ring (vmcnt(0)) every D steps
  const int tid = threadIdx.x, lane = tid & 63;
  const int row0 = tile * 16;
  if (tid >= NT + 64 * NPUB + 64) {
    // dz wave: after step s's barrier, the dz tile of step s from zs[s & 1] (held until step s + 2's
    // cell phase) -> HBM with 16-byte stores, beside the publisher's dx granules
    if (CHAINB_PUBPRIO > 0) __builtin_amdgcn_s_setprio(CHAINB_PUBPRIO);
    const int nsteps = (T + D - 1) / D * D;
    __syncthreads();
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      lds_barrier();
      if (s < T) {
        const int pb = s & 1;
        __bf16* zt = S.dz + ((size_t)(T - 1 - s) * Mp + row0) * G4;
#pragma unroll
        for (int q = lane; q < 16 * G4 / 8; q += 64) {
          const int e = 8 * q;
          *reinterpret_cast<uint4*>(zt + e) = *reinterpret_cast<const uint4*>(&zs[pb][e / G4][e % G4]);
        }
      }
    }
    __syncthreads();
    return;
  }
  if (tid >= NT + 64 * NPUB) {
    // dx wave: after step s's barrier, dx^T = W dz^T of that step from zs[s & 1] into dxs[s & 1]
    // (the publisher stores it after the next barrier). It joins barrier s + 1 only once
    // done, and zs[s & 1] is rewritten only in step s + 2's cell phase (after barrier s + 1), so the
    // compute waves go from their dh_rec MFMA straight to the next cell phase.
    if (CHAINB_DXPRIO > 0) __builtin_amdgcn_s_setprio(CHAINB_DXPRIO);
    const int col = lane & 15, quad = lane >> 4;
    bf16x8_t wx[NXB][KB];
#pragma unroll
    for (int xb = 0; xb < NXB; ++xb) {
      const int din = 16 * xb + col;
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        bf16x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (__bf16)(S.W[(size_t)min(din, Dw - 1) * G4 + 32 * k + 8 * quad + j] * (din < Dw ? 1.f : 0.f));
        wx[xb][k] = v;
      }
    }
    const int nsteps = (T + D - 1) / D * D;
    __syncthreads();
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      lds_barrier();
      if (s < T) {
        const int p = s & 1;
        bf16x8_t bz[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) bz[k] = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][32 * k + 8 * quad]);
#pragma unroll
        for (int xb = 0; xb < NXB; ++xb) {
          f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k = 0; k < KB; ++k) a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wx[xb][k], bz[k], a, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r) dxs[p][col][16 * xb + 4 * quad + r] = a[r];
        }
        chain_mark_wave((S.prof != nullptr && tile == 0) ? S.prof : nullptr, s, 6);   // (dx tile in LDS)
      }
    }
    __syncthreads();
    return;
  }
  if (tid >= NT) {
    // Publisher waves (spare waves of the 1024-thread workgroup): they alone store the dx granules.
    // The write-through (sc1) stores are acknowledged only after the memory round trip and the
    // vector-memory counter retires in order, so in a compute wave every wait for a ring load also
    // waited for the stores issued before it (~2 us per step, 6x the step time). The publishers join
    // the same barriers and read the dx tile from LDS.
    if (CHAINB_PUBPRIO > 0) __builtin_amdgcn_s_setprio(CHAINB_PUBPRIO);
    const int nsteps = (T + D - 1) / D * D;
    const int nx = 16 * Din;
    const size_t xstep = (size_t)Mp * Din;
    // publisher wave pj of NPUB publishes the 64-element slices pj, pj + NPUB, ... of each dx tile
    // (pj as a scalar: derived from tid alone, the element counts below were per-lane values to the
    // compiler and every "wave-uniform" test in the step an exec-masked branch)
    const int pj = __builtin_amdgcn_readfirstlane((tid - NT) >> 6);
    constexpr int ESTR = 64 * NPUB;
    const int dq = ESTR / Din, dr = ESTR % Din;
    // LDS reads of CHAINB_PUBBATCH elements per lane first, then their stores: a read -> wait -> store
    // loop per element paid one LDS round trip per element on the publisher's step (16 Din / 64 =
    // Din / 4 elements per lane, the same count on every lane since Din % 4 == 0). (All Din / 4 at
    // once, up to 16, pushed the kernel from 32 to 176 bytes of scratch: chain bwd 133 -> 258 us.)
    constexpr int PUBN = CHAINB_PUBBATCH > 0 ? CHAINB_PUBBATCH : 1;   // elements per lane per batch
    // The publisher's step paces the stage (profiles/chain_bwd_step_micro.txt: 951 shader clocks per step,
    // 779 with idle publishers, 843 with this form), so nothing that is fixed for the launch stays in it.
    // A lane's elements 64 pj + lane + ESTR i, i < npub, sit at fixed offsets of a dxs buffer: the
    // division by Din is done once, here. PUBE: a lane's elements of the widest tile (Din <= 64: chain_bwd_setup).
    constexpr int PUBE = (16 * 64 + ESTR - 1) / ESTR;
    const int npub = min(max((nx - 64 * pj + ESTR - 1) / ESTR, 0), PUBE);   // wave-uniform: nx % 64 == 0
    int lofs[PUBE];
    {
      int row = (lane + 64 * pj) / Din, k = (lane + 64 * pj) % Din;
#pragma unroll
      for (int i = 0; i < PUBE; ++i) {
        lofs[i] = row * (32 * KX + CHAINB_XPAD) + k;
        row += dq;
        k += dr;
        if (k >= Din) { k -= Din; ++row; }
      }
    }
    const size_t o0 = (size_t)row0 * Din + 64 * pj + lane;
    auto publish = [&](int buf, int ts) {
      const unsigned tag = tagb | (unsigned)ts;
      const float* xt = &dxs[buf][0][0];
      const size_t o = o0 + (size_t)ts * xstep;
#pragma unroll
      for (int i0 = 0; i0 < PUBE; i0 += PUBN) {
        float vv[PUBN];
#pragma unroll
        for (int i = i0; i < i0 + PUBN && i < PUBE; ++i) {
          if (i < npub) vv[i - i0] = xt[lofs[i]];
        }
#pragma unroll
        for (int i = i0; i < i0 + PUBN && i < PUBE; ++i) {
          if (i < npub) {
            if constexpr (XO) st_granule(S.sout + o + ESTR * i, vv[i - i0], tag);
            else S.dx[o + ESTR * i] = vv[i - i0];
          }
        }
      }
    };
    __syncthreads();
    __syncthreads();
    long long* prw = (S.prof != nullptr && tile == 0 && pj == 0) ? S.prof : nullptr;
    for (int s = 0; s < nsteps; ++s) {   // step s - 1's dx tile (the dx wave's) is complete after barrier s
      lds_barrier();
      const int t = T - 1 - s;
      if (s >= 1 && s <= T) publish((s - 1) & 1, t + 1);
      if (s < T) chain_mark_wave(prw, s, 7);   // (the publisher's work of the step is issued)
    }
    __syncthreads();
    publish((T - 1) & 1, 0);
    return;
  }
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, quad = lane >> 4;

  for (int i = tid; i < 2 * 16 * C::HP; i += NT) (&dhs[0][0][0])[i] = 0.f;

  // U^T rows of this wave's four units (rows with (col & 3) != 0 zero: element 0 of the product is
  // this lane's unit)
  const int unit = 4 * w + quad;
  bf16x8_t ufr[KB];
  {
    const int au = 4 * w + (col >> 2);
#pragma unroll
    for (int s = 0; s < KB; ++s) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float val = S.U[(size_t)au * G4 + 32 * s + 8 * quad + j];
        v[j] = (__bf16)(val * ((col & 3) == 0 ? 1.f : 0.f));
      }
      ufr[s] = v;
    }
  }

  // forward state ring (gates, c_t) and the dh element ring, D reverse steps ahead
  uint2 rg[D];                       // packed bf16 gates
  float rc[D];
  unsigned long long rq[D];
  unsigned ri[D];
  // tt / P as a multiply-high with the magic floor(2^32 / P) + 1 (exact for tt * P < 2^32; here
  // tt < 4096, P <= 255): the per-step integer divisions by the run-time pool size cost the
  // un-pooling stages ~160 shader clocks per step on the dh staging (phase table, round 5). The
  // magic of P == 1 would be 2^32, which wraps to 0, so that pool size (a chain that ends in
  // MaxPooling1D(1)) takes the identity instead
  const unsigned pmag = (UP && P > 1) ? 0xFFFFFFFFu / (unsigned)P + 1u : 0u;
  auto divp = [&](int tt) { return P > 1 ? (int)__umulhi((unsigned)tt, pmag) : tt; };
  // source time of the dh of time tt (-1: past the last pooling window -> zero gradient)
  auto src_t = [&](int tt) {
    if constexpr (UP) return tt < Ts * P ? divp(tt) : -1;
    else return tt;
  };
  const size_t eoff = (size_t)row0 * H + tid;        // this lane's dh element in a [Mp][H] row block
  const size_t hstep = (size_t)Mp * H;

  if constexpr (SRC) {    // start once the stage above is D + LEAD steps ahead (see the forward)
    int tw = T - 1 - (D + CHAINB_LEAD);
    tw = max(tw, 0);
    const int st = src_t(tw);
    if (st >= 0) (void)chain_wait(S.din + eoff + (size_t)st * hstep, tagb | (unsigned)st, ctl);
  }
  constexpr unsigned NOSRC = 0xFFFFFFFFu;
  const unsigned lo8 = (unsigned)((tile * NW + w) * 64 + lane) * 8u;    // this lane's cell in a state step (bytes of g)
  const unsigned gstr = (unsigned)(ntiles * NW * 64 * 8);               // bytes per step of g (c: half)
  const char* gbase = reinterpret_cast<const char*>(S.g);
  const char* cbase = reinterpret_cast<const char*>(S.c);
  int stt = T - 1;                                                      // time of the next state load
  auto state_load = [&](int J) {
    const unsigned o = (unsigned)__builtin_amdgcn_readfirstlane(stt) * gstr + lo8;   // (a scalar product)
    rg[J] = *reinterpret_cast<const uint2*>(gbase + o);
    rc[J] = *reinterpret_cast<const float*>(cbase + (o >> 1));
    stt = max(stt - 1, 0);                                              // (steps past the sequence reload t = 0)
  };
  // dh source cursor: time dtt (< 0 past the sequence), source row dst and phase dph = dtt - dst P of
  // an un-pooling stage (dph >= P: the tail past the last pooling window, read from the last row)
  constexpr unsigned ESZ = SRC ? 8 : 4;
  const unsigned eo = (unsigned)eoff;
  const unsigned hrow = (unsigned)hstep;
  const char* dbase = SRC ? reinterpret_cast<const char*>(S.din) : reinterpret_cast<const char*>(S.dh);
  const char* pbase = reinterpret_cast<const char*>(S.pidx);
  int dtt = T - 1;
  int dst = UP ? min(divp(dtt), Ts - 1) : dtt;
  int dph = UP ? dtt - dst * P : 0;
  const unsigned dlim = (unsigned)(UP ? Ts * P : T);                    // times with a source granule: [0, dlim)
  unsigned rinf[D];                 // per ring slot: phase << 12 | source row, NOSRC: no source granule
  auto ring_load = [&](int J) {
    const unsigned o = (unsigned)max(dst, 0) * hrow + eo;
    if constexpr (SRC) rq[J] = ld_granule(reinterpret_cast<const unsigned long long*>(dbase + o * ESZ));
    else rq[J] = (unsigned long long)__float_as_uint(*reinterpret_cast<const float*>(dbase + o * ESZ));
    if constexpr (UP) ri[J] = (unsigned)*reinterpret_cast<const unsigned char*>(pbase + o);
    else ri[J] = 0u;
    const unsigned inf = ((unsigned)dph << 12) | (unsigned)dst;
    rinf[J] = (unsigned)dtt < dlim ? inf : NOSRC;
    --dtt;
    if constexpr (UP) {
      const bool wrap = dph == 0;                                       // the source row changes
      dst = wrap ? dst - 1 : dst;
      dph = wrap ? P - 1 : dph - 1;
    } else {
      --dst;
    }
  };
  // dh of ring slot J (tag-checked for a stream source, un-pool select)
  auto stage = [&](int J) -> float {
    const unsigned inf = rinf[J];
    const bool has = inf != NOSRC;
    if constexpr (SRC) {
      const unsigned want = tagb | (inf & 0xfffu);
      const bool bad = has && (unsigned)(rq[J] >> 32) != want;
      if (__builtin_amdgcn_ballot_w64(bad) != 0) {
        rq[J] = chain_wait(S.din + eoff + (size_t)(inf & 0xfffu) * hstep, want, ctl);
      }
    }
    const float v = __uint_as_float((unsigned)rq[J]);
    bool keep = has;
    if constexpr (UP) keep = keep && ri[J] == (inf >> 12);
    return keep ? v : 0.f;
  };
  // the cell of one step in two halves: what the saved state alone gives, and what needs dh_rec
  // (tanh(c) stays a statement of its own: folded into cell_pre as a local the compiler scheduled the
  // step differently, same-box 0.2383-0.2403 against 0.2350-0.2360 ms/step)
  float tc, fo, ff, z0, z1, z2, z3;
  auto cell_pre_c = [&](int J) { tc = tanhf_fast(rc[J]); };
  auto cell_pre = [&](int J, int JN, int tt) {
    const float cp = rc[JN] * (tt > 0 ? 1.f : 0.f);                     // c_{t-1}
    const float4 g4 = gates_unpack(rg[J]);
    fo = g4.w * (1.f - tc * tc);
    ff = g4.y;
    z0 = g4.z * g4.x * (1.f - g4.x);
    z1 = cp * g4.y * (1.f - g4.y);
    z2 = g4.x * (1.f - g4.z * g4.z);
    z3 = tc * g4.w * (1.f - g4.w);
  };
  float dc = 0.f;
  auto cell_tail = [&](int pb, float dh) {
    const float dct = dc + dh * fo;
    dc = dct * ff;
    zs[pb][col][0 * H + unit] = (__bf16)(dct * z0);
    zs[pb][col][1 * H + unit] = (__bf16)(dct * z1);
    zs[pb][col][2 * H + unit] = (__bf16)(dct * z2);
    zs[pb][col][3 * H + unit] = (__bf16)(dh * z3);
  };

#pragma unroll
  for (int j = 0; j < D; ++j) {
    state_load(j);
    ring_load(j);
  }
  __syncthreads();
  dhs[0][tid / H][tid % H] = stage(0);          // dh of steps 0 and 1
  ring_load(0);
  dhs[1][tid / H][tid % H] = stage(1);
  ring_load(1);
  __syncthreads();
  float dhn = dhs[0][col][unit];
  if (tid == 0 && S.trace_mid) S.trace_mid[blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime();
  cell_pre_c(0);
  cell_pre(0, 1, T - 1);                        // step 0: no dh_rec yet
  cell_tail(0, dhn);
  state_load(0);

  long long* pr = (S.prof != nullptr && tile == 0) ? S.prof : nullptr;
  for (int s0 = 0; s0 < T; s0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int s = s0 + j;
      const int p = s & 1;
      const int j1 = (j + 1) % D, j2 = (j + 2) % D;
      lds_barrier();
      chain_mark(pr, s, 0);
      const bf16x8_t bz0 = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][8 * quad]);
      __builtin_amdgcn_sched_barrier(0);         // (the fences keep this order: see the stage's header)
      f32x4_t a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[0], bz0, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8_t bz1 = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][32 + 8 * quad]);
      dhn = dhs[p ^ 1][col][unit];
      dhs[p][tid / H][tid % H] = stage(j2);     // dh of step s + 2, then its slot's next load
      ring_load(j2);
      chain_mark(pr, s, 1);
      __builtin_amdgcn_sched_barrier(0);
      const f32x4_t a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[1], bz1, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      cell_pre_c(j1);
      cell_pre(j1, j2, T - 2 - s);
      __builtin_amdgcn_sched_barrier(0);
      float dhr = a0[0] + a1[0];
#ifdef GQ_CHAIN_PROF
      if (pr != nullptr) asm volatile("" : "+v"(dhr));
#endif
      chain_mark(pr, s, 2);
      cell_tail(p ^ 1, dhn + dhr);
      chain_mark(pr, s, 3);
      state_load(j1);
      chain_mark(pr, s, 4);
    }
  }
  __syncthreads();
}

// One H = 32 / 64 layer of one tile, reverse in time, with the two per-step products split over K
// (ChainBLdsSK): the cell phase, a barrier, the partial products into LDS, a second barrier, the sum
// of the dh_rec partials. dh comes one element per lane from the stage above's stream (or, stage 0,
// from global memory), un-pooled on load. An H = 32 stage hands its dz and dx tiles to the dz wave
// and the publisher waves; the compute waves of an H = 64 stage store them themselves.
template <int H, int KX, int D, bool SRC, bool UP, bool XO>
__device__ __forceinline__ void chain_bwd_stage_sk(const ChainBStage S, int tile, int ntiles, int Mp, unsigned tagb,
                                                   int* ctl, char* smem) {
  using C = TMC<H>;
  constexpr int CPL = C::CPL, NW = C::NW, NT = C::NT, G4 = C::G4, KB = C::KB;
  constexpr int NXB = KX * 2;
  static_assert(H >= 32 && CPL == 1 && 16 * H == NT, "one dh element per lane");
  using LK = ChainBLdsSK<H, KX>;
  constexpr int UT = LK::UT, KG = LK::KG, KXG = LK::KXG, KPG = KB / KG, KPX = KB / KXG;
  constexpr int NPUB = CHAINB_NPUB;
  static_assert(NW % UT == 0 && KB % KG == 0 && NW % NXB == 0 && KB % KXG == 0, "split-K tiling");
  static_assert(LK::BYTES <= CHAINB_LDS_STAGE && LK::ZS % 16 == 0 && LK::DH % 16 == 0, "chain bwd LDS layout");
  auto zs = reinterpret_cast<__bf16 (*)[16][G4 + CHAINB_ZPAD]>(smem);
  auto dhs = reinterpret_cast<float (*)[16][C::HP]>(smem + LK::ZS);
  auto dpart = reinterpret_cast<float (*)[16][C::HP]>(smem + LK::ZS + LK::DH);                      // [KG]
  auto xpart = reinterpret_cast<float (*)[KXG][16][LK::XPP]>(smem + LK::ZS + LK::DH + LK::DP);      // [2][KXG]

  const int T = S.T, Din = S.Din, Dw = S.Dw, P = S.P, Ts = S.Ts;
  // source kind and un-pooling are template parameters: with run-time branches around the
  // ring loads the compiler drained the whole prefetch ring (vmcnt(0)) every D steps
  const int tid = threadIdx.x, lane = tid & 63;
  const int row0 = tile * 16;
  constexpr bool PUBW = H == 32;                   // publisher waves and the dz wave (chainb_live_threads)
  if constexpr (PUBW) {
    if (tid >= NT + 64 * NPUB) {
      // dz wave: after step s's barrier (the first of the step's two), the dz tile of step s from zs[s & 1] (held until step s + 2's
      // cell phase) -> HBM with 16-byte stores, beside the publisher's dx granules
      if (CHAINB_PUBPRIO > 0) __builtin_amdgcn_s_setprio(CHAINB_PUBPRIO);
      const int nsteps = (T + D - 1) / D * D;
      __syncthreads();
      __syncthreads();
      for (int s = 0; s < nsteps; ++s) {
        lds_barrier();
        if (s < T) {
          const int pb = s & 1;
          __bf16* zt = S.dz + ((size_t)(T - 1 - s) * Mp + row0) * G4;
#pragma unroll
          for (int q = lane; q < 16 * G4 / 8; q += 64) {
            const int e = 8 * q;
            *reinterpret_cast<uint4*>(zt + e) = *reinterpret_cast<const uint4*>(&zs[pb][e / G4][e % G4]);
          }
        }
        lds_barrier();
      }
      __syncthreads();
      return;
    }
    if (tid >= NT) {
      // publisher waves, as in chain_bwd_stage16; the dx tile is the sum of the K slices' partial tiles
      if (CHAINB_PUBPRIO > 0) __builtin_amdgcn_s_setprio(CHAINB_PUBPRIO);
      const int nsteps = (T + D - 1) / D * D;
      const int nx = 16 * Din;
      const size_t xstep = (size_t)Mp * Din;
      // publisher wave pj of NPUB publishes the 64-element slices pj, pj + NPUB, ... of each dx tile
      const int pj = (tid - NT) >> 6;
      constexpr int ESTR = 64 * NPUB;
      const int dq = ESTR / Din, dr = ESTR % Din;
      // LDS reads of CHAINB_PUBBATCH elements per lane first, then their stores: a read -> wait -> store
      // loop per element paid one LDS round trip per element on the publisher's step (16 Din / 64 =
      // Din / 4 elements per lane, the same count on every lane since Din % 4 == 0). (All Din / 4 at
      // once, up to 16, pushed the kernel from 32 to 176 bytes of scratch: chain bwd 133 -> 258 us.)
      constexpr int PUBN = CHAINB_PUBBATCH > 0 ? CHAINB_PUBBATCH : 1;   // elements per lane per batch
      auto publish = [&](int buf, int ts) {
        const unsigned tag = tagb | (unsigned)ts;
        for (int e0 = 64 * pj; e0 < nx; e0 += ESTR * PUBN) {
          const int niter = min((nx - e0 + ESTR - 1) / ESTR, PUBN);
          float vv[PUBN];
          int row = (lane + e0) / Din, k = (lane + e0) % Din;
#pragma unroll
          for (int i = 0; i < PUBN; ++i) {
            if (i < niter) {                          // wave-uniform
              float v = 0.f;
#pragma unroll
              for (int g = 0; g < KXG; ++g) v += xpart[buf][g][row][k];
              vv[i] = v;
            }
            row += dq;
            k += dr;
            if (k >= Din) { k -= Din; ++row; }
          }
#pragma unroll
          for (int i = 0; i < PUBN; ++i) {
            if (i < niter) {
              const int e = e0 + lane + ESTR * i;
              const size_t o = (size_t)row0 * Din + e + (size_t)ts * xstep;
              if constexpr (XO) st_granule(S.sout + o, vv[i], tag);
              else S.dx[o] = vv[i];
            }
          }
        }
      };
      __syncthreads();
      __syncthreads();
      for (int s = 0; s < nsteps; ++s) {   // two barriers per step; step s's dx tile is complete after the second
        lds_barrier();
        lds_barrier();
        if (s < T) publish(s & 1, T - 1 - s);
      }
      __syncthreads();
      return;
    }
  }
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, quad = lane >> 4;

  for (int i = tid; i < 2 * 16 * C::HP; i += NT) (&dhs[0][0][0])[i] = 0.f;

  const int unit = 4 * w + quad;
  // wave w owns unit tile ut over K slice kg of dh_rec^T, din tile xt over K slice kx of dx^T
  const int ut = w % UT, kg = w / UT, xt = w % NXB, kx = w / NXB;
  bf16x8_t ufr[KPG];
  bf16x8_t ufk[KPX];                               // (the W fragments of this wave's dx slice)
#pragma unroll
  for (int q = 0; q < KPG; ++q) {
    bf16x8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)S.U[(size_t)(16 * ut + col) * G4 + 32 * (kg * KPG + q) + 8 * quad + j];
    ufr[q] = v;
  }
  {
    const int din = 16 * xt + col;
#pragma unroll
    for (int q = 0; q < KPX; ++q) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (__bf16)(S.W[(size_t)min(din, Dw - 1) * G4 + 32 * (kx * KPX + q) + 8 * quad + j] * (din < Dw ? 1.f : 0.f));
      ufk[q] = v;
    }
  }

  // forward state ring (gates, c_t) and the dh element ring, D reverse steps ahead
  uint2 rg[D];                       // packed bf16 gates
  float rc[D];
  unsigned long long rq[D];
  unsigned ri[D];
  auto sidx = [&](int tt) { return ((((size_t)tt * ntiles + tile) * NW + w)) * 64 + lane; };
  // tt / P as a multiply-high (see chain_bwd_stage16); P == 1 takes the identity
  const unsigned pmag = (UP && P > 1) ? 0xFFFFFFFFu / (unsigned)P + 1u : 0u;
  auto divp = [&](int tt) { return P > 1 ? (int)__umulhi((unsigned)tt, pmag) : tt; };
  // source time of the dh of time tt (-1: past the last pooling window -> zero gradient)
  auto src_t = [&](int tt) {
    if constexpr (UP) return tt < Ts * P ? divp(tt) : -1;
    else return tt;
  };
  const size_t eoff = (size_t)row0 * H + tid;        // this lane's dh element in a [Mp][H] row block
  const size_t hstep = (size_t)Mp * H;
  auto load_dh = [&](int J, int SS) {
    const int tt = max(T - 1 - SS, 0);
    const int st = max(src_t(tt), 0);
    if constexpr (SRC) rq[J] = ld_granule(S.din + eoff + (size_t)st * hstep);
    else rq[J] = (unsigned long long)__float_as_uint(S.dh[eoff + (size_t)st * hstep]);
    if constexpr (UP) ri[J] = (unsigned)S.pidx[eoff + (size_t)st * hstep];
    else ri[J] = 0u;
  };
  auto load = [&](int J, int SS) {
    const size_t o = sidx(max(T - 1 - SS, 0));
    rg[J] = *reinterpret_cast<const uint2*>(S.g + o * 4);
    rc[J] = S.c[o];
    load_dh(J, SS);
  };
  // dh of time tt from ring slot J (tag-checked for a stream source)
  auto stage_dh = [&](int J, int tt) -> float {
    const int st = tt >= 0 ? src_t(tt) : -1;
    if constexpr (SRC) {
      const bool bad = st >= 0 && (unsigned)(rq[J] >> 32) != (tagb | (unsigned)st);
      if (__builtin_amdgcn_ballot_w64(bad) != 0)
        rq[J] = chain_wait(S.din + eoff + (size_t)max(st, 0) * hstep, tagb | (unsigned)max(st, 0), ctl);
    }
    const float v = __uint_as_float((unsigned)rq[J]);
    bool keep = st >= 0;
    if constexpr (UP) keep = keep && ri[J] == (unsigned)(tt - st * P);
    return keep ? v : 0.f;
  };
  // H = 64, whose compute waves store dz and dx themselves. dz: one float4 granule of the [16][4H]
  // tile per thread
  const int gz_seq = tid / (G4 / 4), gz_c = (tid % (G4 / 4)) * 4;
  __bf16* zbase = S.dz + (size_t)(row0 + gz_seq) * G4 + gz_c;
  const size_t zstep = (size_t)Mp * G4;
  // dx: element e of the [16][Din] tile per lane, NQ passes (Din <= 64), clamped duplicates
  // instead of a branch; XO: publish granules, else (bottom stage) plain fp32
  constexpr int NQ = (16 * 64 + NT - 1) / NT;
  const int nx = 16 * Din;
  const size_t xstep = (size_t)Mp * Din;
  int xrow[NQ], xk[NQ], xo[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = min(tid + q * NT, nx - 1);
    xrow[q] = e / Din;
    xk[q] = e % Din;
    xo[q] = row0 * Din + e;
  }
  auto store_dx = [&](int buf, int ts, unsigned tag) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < KXG; ++g) v += xpart[buf][g][xrow[q]][xk[q]];
      const size_t o = (size_t)xo[q] + (size_t)ts * xstep;
      if constexpr (XO) st_granule(S.sout + o, v, tag);
      else S.dx[o] = v;
    }
  };

  if constexpr (SRC) {    // start once the stage above is D + LEAD steps ahead (see the forward)
    int tw = T - 1 - (D + CHAINB_LEAD);
    tw = max(tw, 0);
    const int st = src_t(tw);
    if (st >= 0) (void)chain_wait(S.din + eoff + (size_t)st * hstep, tagb | (unsigned)st, ctl);
  }
#pragma unroll
  for (int j = 0; j < D; ++j) load(j, j);
  __syncthreads();
  dhs[0][tid / H][tid % H] = stage_dh(0, T - 1);
  load_dh(0, D);                     // (the dh slot alone: the state of step 0 is still to be used)
  float dc = 0.f, dhr = 0.f, dhn;
  __syncthreads();
  dhn = dhs[0][col][unit];
  if (tid == 0 && S.trace_mid) S.trace_mid[blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime();

  long long* pr = (S.prof != nullptr && tile == 0) ? S.prof : nullptr;
  for (int s0 = 0; s0 < T; s0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int s = s0 + j;
      const int t = T - 1 - s;
      const int p = s & 1;
      const int jn = (j + 1 == D) ? 0 : j + 1;
      chain_mark(pr, s, 0);
      {
        const float cp = rc[jn] * (t > 0 ? 1.f : 0.f);
        const float dh = dhn + dhr;
        const float4 g4 = gates_unpack(rg[j]);
        const float tc = tanhf_fast(rc[j]);
        const float dct = dc + dh * g4.w * (1.f - tc * tc);
        dc = dct * g4.y;
        zs[p][col][0 * H + unit] = (__bf16)(dct * g4.z * g4.x * (1.f - g4.x));
        zs[p][col][1 * H + unit] = (__bf16)(dct * cp * g4.y * (1.f - g4.y));
        zs[p][col][2 * H + unit] = (__bf16)(dct * g4.x * (1.f - g4.z * g4.z));
        zs[p][col][3 * H + unit] = (__bf16)(dh * tc * g4.w * (1.f - g4.w));
      }
      {   // state of step s + D and the dh of step s + 1 (time t - 1)
        const int tt = max(T - 1 - (s + D), 0);
        const size_t o = sidx(tt);
        rg[j] = *reinterpret_cast<const uint2*>(S.g + o * 4);
        rc[j] = S.c[o];
      }
      chain_mark(pr, s, 1);
      dhs[p ^ 1][tid / H][tid % H] = stage_dh(jn, t - 1);
      chain_mark(pr, s, 2);
      {
        const int tt = max(T - 1 - (s + 1 + D), 0);
        const int st = max(src_t(tt), 0);
        if constexpr (SRC) rq[jn] = ld_granule(S.din + eoff + (size_t)st * hstep);
        else rq[jn] = (unsigned long long)__float_as_uint(S.dh[eoff + (size_t)st * hstep]);
        if constexpr (UP) ri[jn] = (unsigned)S.pidx[eoff + (size_t)st * hstep];
        else ri[jn] = 0u;
      }
      lds_barrier();
      chain_mark(pr, s, 3);
      dhn = dhs[p ^ 1][col][unit];
      {   // partial products of this wave's K slices -> LDS
        f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < KPG; ++q) {
          const bf16x8_t bz = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][32 * (kg * KPG + q) + 8 * quad]);
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[q], bz, a, 0, 0, 0);
        }
        f32x4_t b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < KPX; ++q) {
          const bf16x8_t bz = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][32 * (kx * KPX + q) + 8 * quad]);
          b = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufk[q], bz, b, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dpart[kg][col][16 * ut + 4 * quad + r] = a[r];
          xpart[p][kx][col][16 * xt + 4 * quad + r] = b[r];
        }
      }
      chain_mark(pr, s, 4);
      if constexpr (!PUBW) {   // dz tile -> HBM (weight-gradient pass; else the dz wave stores it)
        const uint2 zv = *reinterpret_cast<const uint2*>(&zs[p][gz_seq][gz_c]);
        const int tz = t >= 0 ? t : T;
        *reinterpret_cast<uint2*>(zbase + (size_t)tz * zstep) = zv;
      }
      if constexpr (!PUBW) {   // previous step's dx tile (time t + 1) -> stream / HBM; steps outside write row T
        const int ts = (s >= 1 && s <= T) ? t + 1 : T;
        store_dx(p ^ 1, ts, tagb | (unsigned)ts);
      }
      {   // the partial tiles meet: dh_{t-1} of this lane's cell
        lds_barrier();
        float sdh = 0.f;
#pragma unroll
        for (int g = 0; g < KG; ++g) sdh += dpart[g][col][unit];
        dhr = sdh;
      }
      chain_mark(pr, s, 5);
    }
  }
  __syncthreads();
  if constexpr (!PUBW) store_dx((T - 1) & 1, 0, tagb);     // dx tile of t = 0
}

// The head's weight-gradient records of `tile`, built by the time4 backward workgroup after its
// reverse steps (the forward launch handed over dh_{T-1} only): the head backward as it runs in the
// other mode, its dh landing in the now free dhT tile. A function of its own that reads the kernel's
// arguments itself (ka: the launch's kernarg segment; smem: the workgroup's LDS): inlined behind the
// step loop, its live ranges (the whole ChainHead, thread-index arithmetic shared with the
// prologue) cost that loop registers - 24 to 27 VGPR spills instead of 4, with reloads in every
// reverse step, in each inlined arrangement compiled; like this the kernel's resources are the
// same as without it.
typedef __attribute__((address_space(4))) ChainBArgs ChainBKernArgs;
typedef __attribute__((address_space(3))) char ChainLdsChar;
__device__ __noinline__ void chain_t4_bwd_records(const ChainBKernArgs* ka, ChainLdsChar* smem, int tile, int ntiles,
                                                  int Mp) {
  using L = ChainT4BLds;
  char* s = (char*)smem;
  const ChainT4B& Q = ((const ChainBArgs*)ka)->t4;
  chain_head_bwd<128>(Q.hd, Q.h + (size_t)(Q.T - 1) * Mp * 128, tile, ntiles, reinterpret_cast<float*>(s), s + L::DHT);
}

// The weight-gradient record of (layer, tile), built by the layer's backward workgroup after its reverse
// steps (chain_wgrad.h): job = the stage index, CHAIN_MAX for time4; hidden size H. Like
// chain_t4_bwd_records a function of its own that reads the launch's kernarg segment itself, so that the
// step loops in front of it keep their registers. Every live thread of the workgroup calls it. The
// barrier in front drains the workgroup's dz stores and makes them visible to its own loads (workgroup
// scope: one CU, one vector L1, which has not held these lines before), and frees the stage's LDS.
static __device__ __noinline__ void chain_wgrad_epilogue(const ChainBKernArgs* ka_v, ChainLdsChar* smem, int job_v,
                                                         int H_v, int tile_v) {
  const unsigned long long kp = (unsigned long long)ka_v;
  const ChainBKernArgs* ka = (const ChainBKernArgs*)(
      ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(kp >> 32)) << 32) |
      (unsigned)__builtin_amdgcn_readfirstlane((int)kp));
  // (arguments of a call arrive in vector registers: made scalar again, the job record is read with scalar
  // loads from the kernarg segment and every branch on it is uniform)
  const int job = __builtin_amdgcn_readfirstlane(job_v), H = __builtin_amdgcn_readfirstlane(H_v);
  const int tile = __builtin_amdgcn_readfirstlane(tile_v);
  const __attribute__((address_space(4))) ChainWJob* J = &ka->wj[job];
  if (!J->on) return;                              // (frozen weights, or the switch is off)
  __syncthreads();
  const float* x = J->x;
  const float* h = J->h;
  const __bf16* dz = J->dz;
  float* ws = J->ws;
  const long x_elems = J->x_elems;
  const int ldx = J->ldx, T = J->T, Dw = J->Din, Mp = ka->Mp;
  if (H == 32) chain_wgrad_body<32>(x, h, dz, ws, x_elems, ldx, T, Dw, Mp, tile, (char*)smem);
  else if (H == 64) chain_wgrad_body<64>(x, h, dz, ws, x_elems, ldx, T, Dw, Mp, tile, (char*)smem);
  else if (H == 128) chain_wgrad_body<128>(x, h, dz, ws, x_elems, ldx, T, Dw, Mp, tile, (char*)smem);
}

// time4's backward on one 16-sequence tile with 1024 threads: dh_{T-1} from the forward launch
// (Q.hb, with the head backward - chain_head.h, waves 8..15 repeating waves 0..7 - run AFTER the
// steps for its weight-gradient records) or from the head backward run first (Q.hb == nullptr),
// then the reverse recurrence with two cells per lane:
// dh_rec^T = U dz^T with wave w on unit tile w % 8 over K half w / 8, dx^T = W dz^T with din tile
// w % 4 over K quarter w / 4 (partials summed through LDS), dz -> HBM, dx -> granules (tag =
// pooled time of the chain's top layer). Then this tile's share of the head-gradient reduction.
__device__ __forceinline__ void chain_t4_bwd_stage(const ChainT4B Q, const ChainBKernArgs* kargs, int tile, int ntiles,
                                                   int Mp, unsigned tagb, char* smem, long long* mk = nullptr) {
  constexpr int H = 128, G4 = 4 * H, NW = 16, CPL = 2, HP = H + 4, ZP = G4 + 8, XP = 68;
  using L = ChainT4BLds;
  static_assert(L::DHT % 16 == 0 && L::ZS % 16 == 0 && L::DN % 16 == 0, "t4 backward LDS layout");
  float* dhT = reinterpret_cast<float*>(smem);
  char* rs = smem + L::DHT;
  auto zs = reinterpret_cast<__bf16 (*)[ZP]>(rs);
  auto dhn = reinterpret_cast<float (*)[16][HP]>(rs + L::ZS);
  auto dxp = reinterpret_cast<float (*)[16][XP]>(rs + L::ZS + L::DN);
  const int T = Q.T, Din = Q.Din, Dw = Q.Dw;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, quad = lane >> 4;
  const int row0 = tile * 16;

  int unit[CPL];
  size_t so[CPL];                                  // this cell's index in time4's state layout (t = 0)
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) {
    const int gi = w + NW * cc;
    unit[cc] = 4 * gi + quad;
    so[cc] = (((size_t)tile * 8 + (gi & 7)) * 4 + (gi >> 3)) * 64 + lane;
  }
  const size_t sstep = (size_t)ntiles * 8 * 4 * 64;
  // forward state ring (2 reverse steps), refilled right after the cell phase that used a slot
  float4 rg[2][CPL];
  float2 rcs[2][CPL];
  auto load_slot = [&](int j, int t) {
    const size_t tc = (size_t)max(t, 0);
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
      const size_t o = tc * sstep + so[cc];
      rg[j][cc] = *reinterpret_cast<const float4*>(Q.g + o * 4);
      rcs[j][cc] = *reinterpret_cast<const float2*>(Q.c + o * 2);
    }
  };
  load_slot(0, T - 1);
  load_slot(1, T - 2);
  if (Q.hb != nullptr) {                           // dh_{T-1} from the forward launch (dL/dloss = 1): scale
    const float gl = Q.hd.dloss[0];
    for (int e = tid; e < 16 * H; e += 1024) dhT[(e / H) * HP + e % H] = gl * Q.hb[((size_t)tile * 16 + e / H) * H + e % H];
  } else {
    chain_head_bwd<H>(Q.hd, Q.h + (size_t)(T - 1) * Mp * H, tile, ntiles, dhT, rs);
  }
  // weight fragments (after the head prologue: live through it they would crowd its registers),
  // from the forward's lane-contiguous fragment image (time4_head.hip's backward layout: wave
  // w' < 8 holds unit tile w' over the full K, and din tile w' % 4 over gate-column half w' / 4)
  // (Every prologue load before one wait - dL/dloss, both dh loads and these fragments in flight
  // together - compiled with spill traffic inside the step loop below: not done, see
  // profiles/chain_head_handover_ab.txt.)
  const int ut = w & 7, kh = w >> 3, dt = w & 3, kq = w >> 2;
  bf16x8_t ufr[8], wfr[4];
  {
    const bf16x8_t* pu = Q.pk + T4PK_N + (size_t)ut * 16 * 64 + lane;
    const bf16x8_t* pw = Q.pk + T4PK_N + T4PK_BU + (size_t)(dt + 4 * (kq >> 1)) * 8 * 64 + lane;
#pragma unroll
    for (int s = 0; s < 8; ++s) ufr[s] = pu[(8 * kh + s) * 64];
#pragma unroll
    for (int s = 0; s < 4; ++s) wfr[s] = pw[(4 * (kq & 1) + s) * 64];
  }
  __syncthreads();                                 // the head scratch becomes the step tiles
  if (mk != nullptr && tid == 0) mk[0] = (long long)__builtin_amdgcn_s_memrealtime();   // (trace: head done)
  // dx element of this thread (threads past the [16][Din] tile re-read the last one, no store)
  const int nx = 16 * Din;
  const bool ownx = tid < nx;
  const int ex = min(tid, nx - 1), er = ex / Din, ek = ex % Din;
  const size_t xstep = (size_t)Mp * Din, xoff = (size_t)(row0 + er) * Din + ek;
  const int zq = tid >> 6, zc = (tid & 63) * 8;    // dz store: 8 bf16 of the [16][512] tile
  float dc[CPL], dhr[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) dc[cc] = dhr[cc] = 0.f;
  for (int s0 = 0; s0 < T; s0 += 2) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {                   // (static ring slot: a dynamic index spilled the ring)
    const int s = s0 + j;
    if (s >= T) break;
    const int t = T - 1 - s;
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
      const int u = unit[cc];
      const float dh = dhr[cc] + (s == 0 ? dhT[col * HP + u] : 0.f);
      const float4 g = rg[j][cc];
      const float cprev = rcs[j][cc].y;            // (0 at t = 0: the forward's initial state)
      const float tc = tanhf_fast(rcs[j][cc].x);
      const float dct = dc[cc] + dh * g.w * (1.f - tc * tc);
      dc[cc] = dct * g.y;
      zs[col][0 * H + u] = (__bf16)(dct * g.z * g.x * (1.f - g.x));
      zs[col][1 * H + u] = (__bf16)(dct * cprev * g.y * (1.f - g.y));
      zs[col][2 * H + u] = (__bf16)(dct * g.x * (1.f - g.z * g.z));
      zs[col][3 * H + u] = (__bf16)(dh * tc * g.w * (1.f - g.w));
    }
    load_slot(j, t - 2);
    lds_barrier();
    *reinterpret_cast<uint4*>(Q.dz + ((size_t)t * Mp + row0 + zq) * G4 + zc) = *reinterpret_cast<const uint4*>(&zs[zq][zc]);
    {
      f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const bf16x8_t bz = *reinterpret_cast<const bf16x8_t*>(&zs[col][32 * (8 * kh + q) + 8 * quad]);
        if (q & 1) a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[q], bz, a1, 0, 0, 0);
        else a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[q], bz, a0, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bf16x8_t bz = *reinterpret_cast<const bf16x8_t*>(&zs[col][32 * (4 * kq + q) + 8 * quad]);
        if (q & 1) b1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[q], bz, b1, 0, 0, 0);
        else b0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[q], bz, b0, 0, 0, 0);
      }
      const f32x4_t a = a0 + a1, b = b0 + b1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dhn[kh][col][16 * ut + 4 * quad + r] = a[r];
        dxp[kq][col][16 * dt + 4 * quad + r] = b[r];
      }
    }
    lds_barrier();
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) dhr[cc] = dhn[0][col][unit[cc]] + dhn[1][col][unit[cc]];
    const float v = (dxp[0][er][ek] + dxp[1][er][ek]) + (dxp[2][er][ek] + dxp[3][er][ek]);
    if (ownx) st_granule(Q.sout + xoff + (size_t)t * xstep, v, tagb | (unsigned)t);
  }
  }
  if (mk != nullptr && tid == 0) mk[64] = (long long)__builtin_amdgcn_s_memrealtime();  // (trace: steps done)
  if (Q.hb != nullptr) {
    // the head's weight-gradient records, which nothing needed before: this workgroup is done ~15 us
    // into a launch of ~100 us
    __syncthreads();                               // the step tiles become the head scratch
    chain_t4_bwd_records(kargs, (ChainLdsChar*)smem, tile, ntiles, Mp);
  }
  // time4's own weight-gradient record of this tile (the other tiles' head records arrive meanwhile)
  chain_wgrad_epilogue(kargs, (ChainLdsChar*)smem, CHAIN_MAX, H, tile);
  chain_head_bwd_reduce<H>(Q.hd, tile, ntiles);
}

__global__ __launch_bounds__(1024) void lstm_chain_bwd_kernel(ChainBArgs A) {
  const int nblk = gridDim.x;
  __shared__ __attribute__((aligned(16))) char smem[CHAINB_LDS];
  const int s = blockIdx.x / A.nt8, tile = blockIdx.x % A.nt8;
  if (s == A.ns && A.t4.on && tile < A.ntiles) {  // time4 + head backward of this tile
    if (threadIdx.x == 0) A.trace[2 * blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime();
    const unsigned tagb = chain_tag_base((unsigned)__hip_atomic_load(A.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    // (A is this kernel's only explicit argument: it starts the kernarg segment)
    chain_t4_bwd_stage(A.t4, (const ChainBKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), tile, A.ntiles, A.Mp, tagb,
                       smem, blockIdx.x < 64 ? A.trace + 512 + blockIdx.x : nullptr);
    __syncthreads();
    if (threadIdx.x == 0) A.trace[2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime();
    chain_finish(A.ctl, nblk);
    return;
  }
  if (s >= A.ns || tile >= A.ntiles) {
    chain_finish(A.ctl, nblk);
    return;
  }
  if (threadIdx.x == 0) A.trace[2 * blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime();
  const unsigned E = (unsigned)__hip_atomic_load(A.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned tagb = chain_tag_base(E);
  // the stage record is loaded field by field from the kernel arguments (scalar loads): a
  // reference into the by-value argument array made the compiler copy the whole array to
  // scratch and read every field from there inside the step loop
  const ChainBStage S = A.st[s];
  const int H = S.H, KX = S.KX;
  const bool src = s > 0 || A.t4.on;              // (stage 0 then reads time4's dx granules)
  // (the stage function of a hidden size, called straight from the kernel: a wrapper template that
  // picked it changed the generated code)
#define GQ_CHAINB_STAGE_16(KXX, DD, SRCV, UPV, XOV) chain_bwd_stage16<KXX, DD, SRCV, UPV, XOV>
#define GQ_CHAINB_STAGE_32(KXX, DD, SRCV, UPV, XOV) chain_bwd_stage_sk<32, KXX, DD, SRCV, UPV, XOV>
#define GQ_CHAINB_STAGE_64(KXX, DD, SRCV, UPV, XOV) chain_bwd_stage_sk<64, KXX, DD, SRCV, UPV, XOV>
#define GQ_CHAINB_BODY3(HH, KXX, DD, SRCV, UPV, XOV)                                    \
  {                                                                                     \
    if (threadIdx.x >= chainb_live_threads(HH, TMC<HH>::NT)) return;                    \
    GQ_CHAINB_STAGE_##HH(KXX, DD, SRCV, UPV, XOV)(S, tile, A.ntiles, A.Mp, tagb, A.ctl, smem); \
  }
#define GQ_CHAINB_BODY2(HH, KXX, DD, SRCV, UPV)                                         \
  if (!SRCV || S.sout) GQ_CHAINB_BODY3(HH, KXX, DD, SRCV, UPV, true)                    \
  else GQ_CHAINB_BODY3(HH, KXX, DD, SRCV, UPV, false)
#define GQ_CHAINB_BODY(HH, KXX, DD)                                                     \
  {                                                                                     \
    if (src) { if (S.P > 0 && !S.punp) { GQ_CHAINB_BODY2(HH, KXX, DD, true, true) }    \
               else { GQ_CHAINB_BODY2(HH, KXX, DD, true, false) } }                     \
    else { if (S.P > 0) { GQ_CHAINB_BODY3(HH, KXX, DD, false, true, true) }             \
           else { GQ_CHAINB_BODY3(HH, KXX, DD, false, false, true) } }                  \
  }
  if (H == 16) { if (KX == 1) GQ_CHAINB_BODY(16, 1, CHAINB_D16) else GQ_CHAINB_BODY(16, 2, CHAINB_D16) }
  else if (H == 32) { if (KX == 1) GQ_CHAINB_BODY(32, 1, CHAINB_D32) else GQ_CHAINB_BODY(32, 2, CHAINB_D32) }
  else { if (KX == 1) GQ_CHAINB_BODY(64, 1, CHAINB_D64) else GQ_CHAINB_BODY(64, 2, CHAINB_D64) }
#undef GQ_CHAINB_BODY
#undef GQ_CHAINB_BODY2
#undef GQ_CHAINB_BODY3
#undef GQ_CHAINB_STAGE_16
#undef GQ_CHAINB_STAGE_32
#undef GQ_CHAINB_STAGE_64
  // an upper stage's weight-gradient record of this tile; the H = 16 stages run to the launch's end and
  // leave theirs to the tail launch (lstm_grads_multi)
  if (H != 16)
    chain_wgrad_epilogue((const ChainBKernArgs*)__builtin_amdgcn_kernarg_segment_ptr(), (ChainLdsChar*)smem, s, H, tile);
  __syncthreads();
  if (threadIdx.x == 0) A.trace[2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime();
  chain_finish(A.ctl, nblk);
}

// Backward of a chain, stages listed TOP layer first. dh: gradient of the top layer's output
// (pooled if pool[0] > 0); per stage the forward's g / c, W, U, the argmax bytes of the pool
// after the layer (empty if none) and pool size; x_width[s]: channels of the layer's input
// layout. Returns [dz_0 .. dz_{n-1}, dx of the bottom layer].
static std::vector<at::Tensor> chain_bwd_setup(ChainBArgs& A, std::vector<at::Tensor>& keep, const at::Tensor& dh,
                                               at::TensorList g, at::TensorList c, at::TensorList W, at::TensorList U,
                                               at::TensorList pidx, at::IntArrayRef pool, at::IntArrayRef x_width,
                                               at::IntArrayRef T_in, int extra_blocks) {
  check_f32_cuda(dh, "dh");
  const int ns = (int)W.size();
  TORCH_CHECK(ns >= 1 && ns <= CHAIN_MAX && (int)U.size() == ns && (int)g.size() == ns && (int)c.size() == ns &&
                  (int)pidx.size() == ns && (int)pool.size() == ns && (int)x_width.size() == ns &&
                  (int)T_in.size() == ns, "lstm_chain_bwd: stage lists");
  TORCH_CHECK(dh.dim() == 3 && dh.is_contiguous(), "lstm_chain_bwd: dh must be a contiguous [Ts, Mp, H]");
  const int Mp = (int)dh.size(1);
  TORCH_CHECK(Mp % 16 == 0, "lstm_chain_bwd: Mp");
  const int ntiles = Mp / 16, nt8 = (ntiles + 7) / 8 * 8;
  TORCH_CHECK(ns * nt8 + extra_blocks <= chain_capacity(dh.get_device()), "lstm_chain_bwd: ", ns * nt8 + extra_blocks,
              " workgroups cannot all be resident on this device");
  c10::DeviceGuard guard(dh.device());
  auto opt = dh.options();
  A.ns = ns;
  A.ntiles = ntiles;
  A.nt8 = nt8;
  A.Mp = Mp;
  A.ctl = chain_ctl(dh.get_device());
  A.trace = chain_trace_buf(dh.get_device());
  chain_prof_clear(dh.get_device());
  std::vector<at::Tensor> dzs;
  at::Tensor dx, prev;
  for (int s = 0; s < ns; ++s) {
    const int H = (int)U[s].size(0), Dw = (int)W[s].size(0), T = (int)T_in[s], Din = (int)x_width[s];
    const int P = (int)pool[s];
    TORCH_CHECK(H == 16 || H == 32 || H == 64, "lstm_chain_bwd: hidden size ", H);
    TORCH_CHECK(Dw <= Din && Din <= 64 && Din % 4 == 0 && T >= 1 && T < 4096, "lstm_chain_bwd: stage ", s, " shape");
    for (const at::Tensor* t : {&c[s], &W[s], &U[s]}) check_f32_cuda(*t, "lstm_chain_bwd operand");
    check_gates_cuda(g[s]);
    TORCH_CHECK(g[s].numel() == (long)(T + 1) * Mp * H * 4 && c[s].numel() == (long)(T + 1) * Mp * H,
                "lstm_chain_bwd: saved state shapes");
    // (the H = 16 stages address their saved state and their dh source with 32-bit byte offsets)
    TORCH_CHECK(H != 16 || (long)(T + 1) * Mp * H * 8 < (1L << 32), "lstm_chain_bwd: stage ", s, " state too large");
    const int Ts = P > 0 ? T / P : T;
    if (s == 0) {
      TORCH_CHECK(dh.size(0) == Ts && dh.size(2) == H, "lstm_chain_bwd: dh shape");
    } else {
      TORCH_CHECK((int)x_width[s - 1] == H, "lstm_chain_bwd: stage ", s, " output width");
      TORCH_CHECK((int)T_in[s - 1] == Ts, "lstm_chain_bwd: lengths");
    }
    if (P > 0) {
      TORCH_CHECK(pidx[s].numel() == (long)Ts * Mp * H && pidx[s].scalar_type() == at::kByte,
                  "lstm_chain_bwd: argmax bytes");
    }
    ChainBStage& S = A.st[s];
    S.dh = s == 0 ? dh.data_ptr<float>() : nullptr;
    S.din = s == 0 ? nullptr : reinterpret_cast<const unsigned long long*>(prev.data_ptr<int64_t>());
    S.pidx = P > 0 ? pidx[s].data_ptr<uint8_t>() : nullptr;
    S.g = bf16_ptr(g[s]);
    S.c = c[s].data_ptr<float>();
    S.W = W[s].data_ptr<float>();
    S.U = U[s].data_ptr<float>();
    at::Tensor dz = at::empty({T + 1, Mp, 4 * H}, opt.dtype(at::kBFloat16));
    S.dz = bf16_ptr(dz);
    dzs.push_back(dz);
    const bool last = s + 1 == ns && ns > 1;     // (a single stage publishes: profiling)
    if (!last) {
      at::Tensor so = at::empty({T + 1, Mp, Din}, opt.dtype(at::kLong));
      S.sout = reinterpret_cast<unsigned long long*>(so.data_ptr<int64_t>());
      S.dx = nullptr;
      keep.push_back(so);
      prev = so;
    } else {
      dx = at::empty({T + 1, Mp, Din}, opt);
      S.sout = nullptr;
      S.dx = dx.data_ptr<float>();
    }
    S.H = H;
    S.T = T;
    S.Din = Din;
    S.Dw = Dw;
    S.KX = (Din + 31) / 32;
    S.P = P;
    S.Ts = Ts;
    S.trace_mid = A.trace + 512;
    S.prof = chain_prof_rows(dh.get_device(), s);
  }
  dzs.push_back(dx.defined() ? dx.narrow(0, 0, (int)T_in[ns - 1]) : at::empty({0}, opt));
  return dzs;
}

// The weight-gradient epilogue of one backward workgroup row (chain_wgrad.h): x / h the layer's input and output
// of the forward, dz the stage's own, ws a workspace of exactly ntiles records (lstm_grads_record_ws).
static ChainWJob chain_wgrad_job(const at::Tensor& x, const at::Tensor& h, const __bf16* dz, const at::Tensor& ws,
                                 const at::Tensor& W, int H, int T, int Mp) {
  check_f32_cuda(h, "lstm_chain_bwd weight-gradient h");
  check_f32_cuda(ws, "lstm_chain_bwd weight-gradient workspace");
  const int Dw = (int)W.size(0), ntiles = Mp / 16;
  TORCH_CHECK(H == 32 || H == 64 || H == 128, "lstm_chain_bwd: a weight-gradient epilogue needs H = 32, 64 or 128");
  TORCH_CHECK(Dw >= 1 && Dw <= 64 && W.size(1) == 4 * H, "lstm_chain_bwd: weight-gradient W shape");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 3 && x.size(0) == T && x.size(1) == Mp &&
                  x.size(2) >= Dw, "lstm_chain_bwd: weight-gradient x shape");
  const long ldx = x.stride(1);
  TORCH_CHECK(x.stride(2) == 1 && ldx % 4 == 0 && ldx >= x.size(2) && x.stride(0) == (long)Mp * ldx &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "lstm_chain_bwd: weight-gradient x layout");
  const long x_elems = (long)(x.storage().nbytes() / sizeof(float)) - x.storage_offset();
  TORCH_CHECK(((long)T * Mp - 1) * ldx + (Dw + 3) / 4 * 4 <= x_elems, "lstm_chain_bwd: weight-gradient x storage");
  TORCH_CHECK(h.numel() == (long)T * Mp * H, "lstm_chain_bwd: weight-gradient h shape");
  TORCH_CHECK(ws.numel() == (long)ntiles * GradsGeom(H, Dw).RC,
              "lstm_chain_bwd: the weight-gradient workspace holds one record per tile");
  ChainWJob J{};
  J.x = x.data_ptr<float>();
  J.h = h.data_ptr<float>();
  J.dz = dz;
  J.ws = ws.data_ptr<float>();
  J.x_elems = x_elems;
  J.ldx = (int)ldx;
  J.T = T;
  J.Din = Dw;
  J.on = 1;
  return J;
}

// wgrad (optional): [x_s, h_s, ws_s] per stage - the layer's forward input and output and a workspace of ntiles
// records; an empty ws_s leaves the stage's weight gradients to the caller (frozen weights, H = 16)
static void chain_wgrad_jobs(ChainBArgs& A, const std::vector<at::Tensor>& wgrad, at::TensorList W, at::IntArrayRef T_in) {
  TORCH_CHECK((int)wgrad.size() >= 3 * A.ns, "lstm_chain_bwd: wgrad lists [x, h, ws] per stage");
  for (int s = 0; s < A.ns; ++s) {
    if (wgrad[3 * s + 2].numel() == 0) continue;
    A.wj[s] = chain_wgrad_job(wgrad[3 * s], wgrad[3 * s + 1], A.st[s].dz, wgrad[3 * s + 2], W[s], A.st[s].H, (int)T_in[s],
                              A.Mp);
  }
}

std::vector<at::Tensor> lstm_chain_bwd(const at::Tensor& dh, at::TensorList g, at::TensorList c, at::TensorList W,
                                       at::TensorList U, at::TensorList pidx, at::IntArrayRef pool,
                                       at::IntArrayRef x_width, at::IntArrayRef T_in,
                                       c10::optional<std::vector<at::Tensor>> wgrad) {
  ChainBArgs A{};
  std::vector<at::Tensor> keep;
  auto res = chain_bwd_setup(A, keep, dh, g, c, W, U, pidx, pool, x_width, T_in, 0);
  if (wgrad.has_value()) {
    TORCH_CHECK((int)wgrad->size() == 3 * A.ns, "lstm_chain_bwd: wgrad lists [x, h, ws] per stage");
    chain_wgrad_jobs(A, *wgrad, W, T_in);
  }
  hipLaunchKernelGGL(lstm_chain_bwd_kernel, dim3(A.ns * A.nt8), dim3(1024), 0, stream(), A);
  GQ_LAUNCH_CHECK();
  return res;
}

// lstm_chain_bwd with time4 + the head as its first stage (chain_t4_bwd_stage): dloss [1]; x4 the
// pooled top chain output (time4's input, [T4, Mp, Din]); h4 / g4 / c4 time4's saved forward state
// (lstm_chain_head_fwd / time4_head_fwd); Wt4 / Ut4 its weights and pk their fragment image (the
// forward's last result); head = [W1, b1, W2, b2, W3, b3]
// with their gradients hgrads (accumulated); then the chain stages, TOP layer first, as for
// lstm_chain_bwd (the top one must pool by 3). Returns [dz4 [T4 + 1, Mp, 512], dz_0 .. dz_{n-1}, dx].
std::vector<at::Tensor> lstm_chain_head_bwd(const at::Tensor& dloss, const at::Tensor& x4, const at::Tensor& h4,
                                            const at::Tensor& g4, const at::Tensor& c4, const at::Tensor& Wt4,
                                            const at::Tensor& Ut4, const at::Tensor& pk, const at::Tensor& hb,
                                            at::TensorList head, const at::Tensor& y,
                                            const at::Tensor& mask, int64_t M, double alpha1, double alpha2, double w0,
                                            double w1, at::TensorList hgrads, at::TensorList g, at::TensorList c,
                                            at::TensorList W, at::TensorList U, at::TensorList pidx,
                                            at::IntArrayRef pool, at::IntArrayRef x_width, at::IntArrayRef T_in,
                                            c10::optional<std::vector<at::Tensor>> wgrad) {
  check_f32_cuda(x4, "x4");
  for (const at::Tensor* t : {&dloss, &h4, &g4, &c4, &Wt4, &Ut4}) check_f32_cuda(*t, "lstm_chain_head_bwd operand");
  TORCH_CHECK(x4.dim() == 3 && x4.is_contiguous(), "lstm_chain_head_bwd: x4 must be a contiguous [T4, Mp, Din]");
  const int T4 = (int)x4.size(0), Mp = (int)x4.size(1), Din = (int)x4.size(2), Dw = (int)Wt4.size(0);
  TORCH_CHECK(T4 >= 1 && T4 <= 16 && Din <= 64 && Dw >= 1 && Dw <= Din && Wt4.size(1) == 512 && Ut4.size(0) == 128 &&
                  Ut4.size(1) == 512, "lstm_chain_head_bwd: time4 shapes");
  TORCH_CHECK(dloss.numel() == 1, "lstm_chain_head_bwd: dloss must be a scalar");
  TORCH_CHECK(h4.numel() == (long)T4 * Mp * 128 && g4.numel() == (long)T4 * Mp * 128 * 4 && c4.numel() == (long)T4 * Mp * 128 * 2,
              "lstm_chain_head_bwd: time4 saved state shapes");
  TORCH_CHECK(pool.size() >= 1 && pool[0] == 3, "lstm_chain_head_bwd: the top chain stage must pool by 3");
  ChainBArgs A{};
  std::vector<at::Tensor> keep;
  c10::DeviceGuard guard(x4.device());
  auto opt = x4.options();
  at::Tensor so = at::empty({T4, Mp, Din}, opt.dtype(at::kLong));      // time4's dx granules
  auto res = chain_bwd_setup(A, keep, x4, g, c, W, U, pidx, pool, x_width, T_in, (Mp / 16 + 7) / 8 * 8);
  A.st[0].dh = nullptr;
  A.st[0].din = reinterpret_cast<const unsigned long long*>(so.data_ptr<int64_t>());
  ChainT4B& Q = A.t4;
  Q.on = 1;
  Q.h = h4.data_ptr<float>();
  Q.g = g4.data_ptr<float>();
  Q.c = c4.data_ptr<float>();
  TORCH_CHECK(pk.is_cuda() && pk.is_contiguous() && pk.nbytes() == (size_t)T4PK_ALL * 16,
              "lstm_chain_head_bwd: pk must be the forward's full fragment image");
  Q.pk = reinterpret_cast<const bf16x8_t*>(pk.data_ptr());
  if (hb.numel() > 0) {
    check_f32_cuda(hb, "lstm_chain_head_bwd hb");
    TORCH_CHECK(hb.numel() == (long)(Mp / 16) * 16 * 128, "lstm_chain_head_bwd: hb must be the forward's dh tiles");
    Q.hb = hb.data_ptr<float>();
  } else {
    Q.hb = nullptr;
  }
  at::Tensor dz4 = at::empty({T4 + 1, Mp, 512}, opt.dtype(at::kBFloat16));
  Q.dz = bf16_ptr(dz4);
  Q.sout = reinterpret_cast<unsigned long long*>(so.data_ptr<int64_t>());
  Q.T = T4;
  Q.Din = Din;
  Q.Dw = Dw;
  at::Tensor gpart;
  t4_head_bwd_args(Q.hd, head, y, mask, M, Mp, alpha1, alpha2, w0, w1, dloss, hgrads, gpart);
  if (wgrad.has_value()) {       // the stages' [x, h, ws], then time4's ws (its x and h are x4 / h4)
    TORCH_CHECK((int)wgrad->size() == 3 * A.ns + 1, "lstm_chain_head_bwd: wgrad lists [x, h, ws] per stage + time4's ws");
    chain_wgrad_jobs(A, *wgrad, W, T_in);
    const at::Tensor& ws4 = (*wgrad)[3 * A.ns];
    if (ws4.numel() > 0) A.wj[CHAIN_MAX] = chain_wgrad_job(x4, h4, Q.dz, ws4, Wt4, 128, T4, Mp);
  }
  hipLaunchKernelGGL(lstm_chain_bwd_kernel, dim3((A.ns + 1) * A.nt8), dim3(1024), 0, stream(), A);
  GQ_LAUNCH_CHECK();
  res.insert(res.begin(), dz4);
  return res;
}

int chain_bwd_occupancy() { return chain_occupancy(reinterpret_cast<const void*>(&lstm_chain_bwd_kernel)); }

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("lstm_chain_bwd", &gq::lstm_chain_bwd);
  m.impl("lstm_chain_head_bwd", &gq::lstm_chain_head_bwd);
}
