// Cross-CU layer pipeline for the forward of a time-major LSTM stack (gfx950; the hand-off: lstm_chain_common.h).
//
// The per-layer forward kernels (lstm_tm_fwd.hip) run one after another: with the CML batch a
// recurrence occupies 8 of the 256 CUs, and the stack's six recurrences (plus three pool
// launches) are a serial sum. Sequences never mix across layers, so tile j of layer k+1
// only needs tile j of layer k - and only up to the step it is at. This kernel runs all
// layers of the stack at once: workgroup (stage s, tile j) computes layer s of tile j on
// its own CU and consumes layer s-1's output AS IT IS PRODUCED, a few steps behind.
//
// A MaxPooling1D(3) between two stages is done by the CONSUMER while staging its input
// (three granules per element, max + first-max argmax byte): the producer's own per-step
// pooling lengthened its serial chain by ~110 ns per step (58 -> 78 us for the first pooled
// CML layer), while the consumer, running at a third of the producer's step rate, has slack.
// Each stage also writes everything the per-layer kernels write (h, gate / cell state for
// the backward, pooled output + argmax bytes), so the backward is unchanged.
#include "chain_head.h"
#include "gcn_fused.h"
#include "lstm_chain_common.h"
#include "lstm_tm_common.h"

namespace gq {

// granule ring depth of a non-pooling consumer: an sc1 load of a line another CU wrote
// through to memory takes microseconds under load, D steps of ~0.33 us each must cover it.
// D, LEAD1 and CHAINB_LEAD (lstm_chain_bwd.hip) from a same-box sweep of compile-time variants
// (scripts/build_chain_variants.py, scripts/gpu_ab_chain.sh; CML step, ms): D = 6 / LEAD 2 / 2:
// 0.3099 0.3092; D = 5: 0.3105; D = 4: 0.3072 0.3070; D = 3: 0.3055; D = 8: 0.3121; D = 4 with
// CHAINB_LEAD 1: 0.3025; D = 4 with both leads 1: 0.3021 0.3022 0.3006 (kept); D = 3 with both
// leads 1: 0.3044 0.2999. A shorter ring lets each consumer start sooner behind its producer.
#ifndef CHAIN_D
#define CHAIN_D 4
#endif
#ifndef CHAIN_D3
#define CHAIN_D3 2           // ring of a pooling (PIN = 3) consumer: it runs at a third of the rate
#endif                       // (2 vs 3: 0.2982 0.2994 vs 0.3022 0.3027 ms/step; the backward rings at 3
                             // instead of 4 and LEAD3 = 0 were slower: 0.3054 0.3057, 0.3043)
#ifndef CHAIN_D16S
#define CHAIN_D16S 4         // ring of the H = 16 non-pooling stream consumer, the one stage that runs at its producer's rate
#endif
#ifndef CHAIN_LEAD1
#define CHAIN_LEAD1 1
#endif
#ifndef CHAIN_D0
#define CHAIN_D0 6           // x prefetch depth of stage 0 (its input is complete before the launch)
#endif
#ifndef CHAIN_RP_NAPMAX
#define CHAIN_RP_NAPMAX 16   // bulk re-poll of a stale tile: largest nap (s_sleep 2 units) between rounds
#endif
#ifndef CHAIN_PRIO
#define CHAIN_PRIO 2         // s_setprio of the compute waves of a stage with I/O waves
#endif
#ifndef CHAIN_LEAD3
#define CHAIN_LEAD3 1
#endif

struct ChainStage {
  const float* x;                    // stage 0: fp32 input [T][Mp][Din]
  const unsigned long long* xin;     // stages > 0: tagged input stream [T][Mp][Din]
  const float* W;
  const float* U;
  const float* b;
  float* h;                          // [T+1][Mp][H] (row T: scratch)
  __bf16* g;                         // train: [T+1][tiles][NW][CPL][64][4] packed bf16 gates
  float* c;
  unsigned long long* sout;          // tagged output stream [To][Mp][H] (nullptr: last stage)
  float* pout;                       // last stage only: own pooled output [T/P][Mp][H] (P > 0)
  unsigned* iout;
  float* pin_out;                    // PIN > 1: the pooled input [T][Mp][Din] + argmax bytes,
  unsigned char* pin_idx;            //   written here (the producer publishes unpooled h)
  long long* prof;                   // profiling (GNNQC_CHAIN_PROF=1): tile 0's per-step phase clocks
  int H, T, Din, Dw, KX, P, PIN;
};

struct ChainT4 {
  const unsigned long long* xin;     // the last chain stage's granule stream [>= 3 T][Mp][Din]
  const float* W;                    // [Dw][512]
  const float* U;                    // [128][512]
  const float* b;                    // [512]
  float* h;                          // [T][Mp][128]
  float* g;                          // train: [T][tiles][8][4][64][4] fp32 gates (time4_head.hip t4_sidx)
  float* c;                          // train: [T][tiles][8][4][64][2] (c_t, c_{t-1})
  float* pin_out;                    // pooled input [T][Mp][Din]: the chain stage's pooled output
  unsigned char* pin_idx;            //   and its argmax bytes
  int T, Din, Dw, on;
  ChainHead hd;
  float* hb;                         // train: dh_{T-1} of the head for dL/dloss = 1, computed here
                                     // ([ntiles][16][128]; nullptr: the backward launch runs the head backward first)
};

struct ChainArgs {
  ChainStage st[CHAIN_MAX];
  int ns, ntiles, nt8, Mp;
  int* ctl;                          // [0] epoch, [1] finished workgroups, [2] spin timeout seen
  long long* trace;                  // [blocks][2] start / end s_memrealtime (100 MHz) of the last launch
  // extra workgroups past the stages (the chain leaves most CUs idle): build the time4 kernel's
  // A-fragment image (lstm_tm_common.h t4_pack_one) from pkU / pkW into pk
  const float* pkU;
  const float* pkW;
  bf16x8_t* pk;
  int pkDw;
  int npk;                           // packing workgroups
  ChainT4 t4;                        // t4.on: time4 + head as one more stage (blocks [ns nt8, (ns + 1) nt8))
  // side job on the idle CUs: the GCN backward's coefficients (gcn_fused.h gcn_coef_fwd_body), one
  // workgroup per sample row; it only reads the store and writes its own buffer, nothing waits on it
  GcnCoefFwdJob cf;
  // gp.on: the GCN forward itself as producer workgroups (gcn_prod_body), one per sample row; the
  // first stage streams their tagged granules (st[0].xin) and the head waits for all of them
  // (ctl[10] counts them) before it reads the labels they write
  GcnProdJob gp;
};
static_assert(sizeof(ChainArgs) <= 4096, "chain forward kernel arguments");

// One layer of one tile: lstm_tm_fwd_kernel's step with the x ring fed either from global memory
// (stage 0) or from the previous stage's granule stream (SRC), the output also published as granules.
// LDS of one stage (carved from the kernel's one buffer: the stage bodies must not each
// reserve their own static arrays)
template <int H, int KX>
struct ChainLds {
  static constexpr int HS = 2 * 16 * (TMC<H>::KPH + 8) * 2;
  static constexpr int XS = 2 * 16 * (32 * KX + 8) * 2;
  static constexpr int HF = 2 * 16 * TMC<H>::HP * 4;
  // the cells' packed gates and c of two steps (staged for the publisher wave)
  static constexpr int GS = 2 * 16 * H * 8;
  static constexpr int CS = 2 * 16 * H * 4;
  static constexpr int BYTES = HS + XS + HF + GS + CS;
};
constexpr int chain_max2(int a, int b) { return a > b ? a : b; }
static constexpr int CHAIN_LDS_STAGE = chain_max2(chain_max2(ChainLds<64, 2>::BYTES, ChainLds<32, 2>::BYTES),
                                                  ChainLds<16, 2>::BYTES);

// Gate scaling: sigmoid(z) = 1 / (1 + 2^(-z log2 e)), tanh(z) = 2 / (1 + 2^(-2 z log2 e)) - 1, one
// v_exp_f32 each after one multiply. (Folding the scale into the bf16 weight fragments saved the
// multiplies but rounded W log2(e) instead of W: the kernels' rounding no longer matched the other
// LSTM kernels' and the numerics oracle, so the weights stay unscaled.)
__device__ __forceinline__ float chain_gate_scale(int ag) { return ag == 2 ? -2.8853900817779268f : -1.4426950408889634f; }

// Roles of a stage workgroup. H = 16 / 32: waves [0, NW) compute the cells and store their own
// outputs straight from registers (h, the granule that publishes it, the packed gates and c for the
// backward); they issue no global load, so no s_waitcnt vmcnt ever waits on their write-through
// stores. D more waves (the I/O waves) take turns streaming x: I/O wave k loads the whole [16][Din]
// tile of every step s = k (mod D) D steps ahead and, in step s - 1, waits for it (its own loads
// only: a plain vmcnt(0)), checks the tags (re-polls a stale granule), max-pools PIN consecutive
// steps (writing the pooled input and the argmax bytes for the backward) and writes x_s into the
// LDS tile of the next step. (A register ring of D slots in one wave was the first form: the
// compiler's wait insertion drained the whole ring at the top of every unrolled round.) For a last
// stage that pools its own output, I/O wave 0 pools h from the fp32 LDS tile. One LDS barrier per
// step. (H = 16 stages with an unpooled input: the compute waves write the publisher's LDS copies of
// step t at the top of step t + 1, and the publisher runs two steps behind; chain_stage LATEW.) Without I/O waves every thread also streams x through a D-slot register ring, as one role.
// (I/O waves only when they fit the 1024-thread workgroup and a lane's share of one step's tile - ngl
// granules of pin steps each - stays within 24 registers pairs. Every stage of the dispatch table has
// them at the default ring depths; a deeper ring reaches the one-role form, e.g. CHAIN_D = 8 at
// H = 32 / 64: 512 + 64 * 8 + 64 threads.)
__host__ __device__ constexpr int chain_io_waves(int nt, int d, int ngl = 1, int pin = 1) {
  return nt + 64 * d + 64 <= 1024 && ngl * pin <= 12 ? d : 0;   // (+ the publisher wave)
}
// a pooling consumer (pin = 3 granules per element) splits each step's tile over two I/O waves
// (and so does a 64-channel input of an H = 64 stage, 8 granule pairs per lane in one wave: its I/O
// waves' registers spilled; with two waves per step the ring is 3 steps deep to fit the workgroup)
__host__ __device__ constexpr int chain_io_group(int pin, int kx = 1, int h = 16) {
  return pin > 1 || (h == 64 && kx == 2) ? 2 : 1;
}
__host__ __device__ constexpr int chain_stage_d(int h, int kx, int d) {
  return h == 64 && kx == 2 && d > 3 ? 3 : d;
}
// threads of a stage workgroup that run the stage (compute + I/O waves + the publisher)
__host__ __device__ constexpr int chain_live_threads(int nt, int d, int kx, bool src, int pin, int h = 16) {
  return nt + 64 * chain_io_waves(nt, d * chain_io_group(pin, kx, h),
                                  (16 * 32 * kx / (src ? 2 : 4) + 64 * chain_io_group(pin, kx, h) - 1) /
                                      (64 * chain_io_group(pin, kx, h)),
                                  pin) +
         (chain_io_waves(nt, d * chain_io_group(pin, kx, h),
                         (16 * 32 * kx / (src ? 2 : 4) + 64 * chain_io_group(pin, kx, h) - 1) /
                             (64 * chain_io_group(pin, kx, h)),
                         pin) > 0 ? 64 : 0);
}

// Compute layout of a forward chain stage: one cell per lane (as TMC), except H = 64, which runs two
// cells per lane on 8 compute waves so that the I/O waves and the publisher fit the 1024-thread
// workgroup too (with 16 compute waves every thread streamed its own x granules and stored its own
// outputs, and its loads waited behind its write-through stores). The saved gates / c keep the
// one-cell-per-lane layout of the backward (cell (wave gi, lane), gi = compute wave + NW * cc).
template <int H>
struct ChainCfg {
  static constexpr int CPL = H == 64 ? 2 : 1;
  static constexpr int NW = H / 4 / CPL, NT = 64 * NW, G4 = 4 * H;
  static constexpr int KSH = TMC<H>::KSH, KPH = TMC<H>::KPH, HP = TMC<H>::HP;
  static constexpr int NWV = H / 4, NCELL = 64 * NWV;     // the saved-state layout's waves / cells per tile
};

// XC: channels of the x tile the I/O waves load (32 KX, or 16 for a KX = 1 stage with Din <= 16)
template <int H, bool TRAIN, int KX, int D, bool SRC, int PIN, int XC = 32 * KX>
__device__ __forceinline__ void chain_stage(const ChainStage& S, int tile, int ntiles, int Mp, unsigned tagb,
                                            int* ctl, char* smem) {
  using C = ChainCfg<H>;
  constexpr int NW = C::NW, NT = C::NT, G4 = C::G4, CPL = C::CPL, NWV = C::NWV, NCELL = C::NCELL;
  constexpr int KPX = 32 * KX;
  // elements per streamed granule: stage 0 reads float4 of x; a stream consumer reads two adjacent
  // 8-byte {value, tag} granules with one 16-byte load (each half is one whole granule)
  constexpr int GR = SRC ? 2 : 4;
  constexpr int G = chain_io_group(PIN, KX, H);  // I/O waves sharing one step's tile
  constexpr int NIOW = chain_io_waves(NT, D * G, (16 * KPX / GR + 64 * G - 1) / (64 * G), PIN);   // (0: none)
  constexpr bool IOW = NIOW > 0;
  constexpr int NIO = IOW ? 64 * G : NT;         // threads streaming one step's tile
  constexpr int NSLOT = IOW ? 1 : D;             // x slots per streaming thread
  // granules per streaming lane: I/O waves cover the stage's tile class (XC channels); without
  // them every thread streams one granule (the host requires 16 Din / GR <= NT then)
  static_assert(XC <= KPX, "x tile class");
  constexpr int NGL = IOW ? (16 * XC / GR + NIO - 1) / NIO : 1;
  // H = 16 stages with I/O waves and an unpooled input (the bottom layer, which paces the whole chain,
  // and the one consumer that runs at its producer's rate): the compute waves write the publisher's
  // LDS copies of step t at the top of step t + 1, off the path from the cell to the barrier
  constexpr bool LATEW = H == 16 && IOW && PIN == 1;
  using L = ChainLds<H, KX>;
  static_assert(L::BYTES <= CHAIN_LDS_STAGE && L::HS % 16 == 0 && L::XS % 16 == 0, "chain LDS layout");
  auto hs = reinterpret_cast<__bf16 (*)[16][C::KPH + 8]>(smem);
  auto xs = reinterpret_cast<__bf16 (*)[16][KPX + 8]>(smem + L::HS);
  auto hf = reinterpret_cast<float (*)[16][C::HP]>(smem + L::HS + L::XS);
  auto gst = reinterpret_cast<uint2 (*)[NCELL]>(smem + L::HS + L::XS + L::HF);            // [2][cells] (IOW)
  auto cst = reinterpret_cast<float (*)[NCELL]>(smem + L::HS + L::XS + L::HF + L::GS);   // [2][cells] (IOW)

  const int T = S.T, Din = S.Din, Dw = S.Dw, P = S.P;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, quad = lane >> 4;
  const int row0 = tile * 16;
  const size_t hstep = (size_t)Mp * H;
  const int To = P > 0 ? T / P : T;      // (P > 0 only without a consumer stage)

  constexpr int NTL = NT + 64 * NIOW + (IOW ? 64 : 0);   // live threads (the rest exited)
  for (int i = tid; i < 2 * 16 * (C::KPH + 8); i += NTL) (&hs[0][0][0])[i] = (__bf16)0.0f;
  for (int i = tid; i < 2 * 16 * (KPX + 8); i += NTL) (&xs[0][0][0])[i] = (__bf16)0.0f;

  // ---- x streaming: lane iot of a streaming wave / thread block owns granules iot + NIO j of the
  // contiguous [16][Din] tile (mod n_gx: duplicate lanes load and write the same values; no branch
  // around a load - the compiler drains vmcnt at the join of one)
  const bool compute = w < NW;
  const int iow = IOW ? (w - NW) / G : 0;        // I/O wave group (IOW): steps s = iow (mod D)
  const int iot = IOW ? ((w - NW) % G) * 64 + lane : tid;
  const int n_gx = 16 * Din / GR;
  const size_t xstep = (size_t)Mp * Din;
  // per granule: its element offset in the tile (32 bits; the tile of step tx starts at element
  // (tx Mp + row0) Din) and its LDS byte offset in the bf16 x tile
  int goff[NGL], loff[NGL];
#pragma unroll
  for (int j = 0; j < NGL; ++j) {
    const int gx = min(iot + NIO * j, n_gx - 1) * GR;
    goff[j] = gx;
    loff[j] = ((gx / Din) * (KPX + 8) + gx % Din) * 2;
  }
  const size_t xbase = (size_t)row0 * Din;
  char* xsb = reinterpret_cast<char*>(&xs[0][0][0]);
  constexpr int XBUF = 16 * (KPX + 8) * 2;       // bytes of one x tile buffer
  // (x granules as whole vectors: a float[4] ring was split into scalars and the compiler copied
  // lanes of a just-issued load into the loop-carried registers - an immediate vmcnt wait for the
  // full memory latency in every staging step)
  f32x4_t xr[NSLOT][NGL];
  u64x2_t xq[NSLOT][NGL][PIN];
  // (unused since the 16-byte-load variant of load_x went: without it a few scalar instructions move, profiles/lstm_chain_split.txt)
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned long long*>(SRC ? S.xin : nullptr), (short)0, 0x7fffffff, 0x00020000);
  auto load_x = [&](int r, int tx) {
#pragma unroll
    for (int q = 0; q < (SRC ? PIN : 1); ++q) {
      const size_t tb = xbase + (size_t)(SRC ? PIN * tx + q : tx) * xstep;
#pragma unroll
      for (int j = 0; j < NGL; ++j) {
        if constexpr (SRC) {
          // (one 16-byte buffer load per granule pair instead: stale reads, ~4.5k re-polls per launch, measured)
          xq[r][j][q] = u64x2_t{ld_granule(S.xin + tb + goff[j]), ld_granule(S.xin + tb + goff[j] + 1)};
        } else {
          xr[r][j] = *reinterpret_cast<const f32x4_t*>(S.x + tb + goff[j]);
        }
      }
    }
  };
  long long* pr = (S.prof != nullptr && tile == 0) ? S.prof : nullptr;
  int mark_t = CHAIN_PROF_STEPS;                 // (profiling: the step an I/O wave's staging is clocked under)
  auto stage_x = [&](int buf, int r, int tx) {
    if constexpr (SRC) {
      // every granule's tag first (one ballot), the re-poll only on a miss
      bool bad = false;
#pragma unroll
      for (int j = 0; j < NGL; ++j)
#pragma unroll
        for (int q = 0; q < PIN; ++q) {
          const unsigned want = tagb | (unsigned)(PIN * tx + q);
          bad |= (unsigned)(xq[r][j][q].x >> 32) != want || (unsigned)(xq[r][j][q].y >> 32) != want;
        }
      if (__builtin_amdgcn_ballot_w64(bad) != 0) {
        // re-poll: every granule of the tile re-loaded AT ONCE per round (one memory round trip a
        // round, not one per granule), short back-off, bounded (a timeout flags the step)
#ifdef GQ_CHAIN_PROF
        if (lane == 0) __hip_atomic_fetch_add(ctl + 9, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0 && S.prof != nullptr)
          __hip_atomic_fetch_add(S.prof + CHAIN_PROF_STEPS * 8, 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
        const int lim0 = __hip_atomic_load(ctl + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int lim = lim0 > 0 ? lim0 : CHAIN_SPIN;
        int nap = 1;
        for (int it = 0;; ++it) {
#pragma unroll
          for (int q = 0; q < PIN; ++q) {
            const size_t tb = xbase + (size_t)(PIN * tx + q) * xstep;
#pragma unroll
            for (int j = 0; j < NGL; ++j)
              xq[r][j][q] = u64x2_t{ld_granule(S.xin + tb + goff[j]), ld_granule(S.xin + tb + goff[j] + 1)};
          }
          bad = false;
#pragma unroll
          for (int j = 0; j < NGL; ++j)
#pragma unroll
            for (int q = 0; q < PIN; ++q) {
              const unsigned want = tagb | (unsigned)(PIN * tx + q);
              bad |= (unsigned)(xq[r][j][q].x >> 32) != want || (unsigned)(xq[r][j][q].y >> 32) != want;
            }
          if (__builtin_amdgcn_ballot_w64(bad) == 0) break;
          if (it >= lim) {
            __hip_atomic_store(ctl + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          for (int k = 0; k < nap; ++k) __builtin_amdgcn_s_sleep(2);
          nap = min(nap * 2, CHAIN_RP_NAPMAX);
        }
      }
      if (iot == 0) chain_mark_wave(pr, mark_t, 6);   // (the tile's loads are in, tags checked)
      const size_t po = xbase + (size_t)tx * xstep;
#pragma unroll
      for (int j = 0; j < NGL; ++j) {
        float m0 = __uint_as_float((unsigned)xq[r][j][0].x), m1 = __uint_as_float((unsigned)xq[r][j][0].y);
        if constexpr (PIN > 1) {
          unsigned a0 = 0, a1 = 0;
#pragma unroll
          for (int q = 1; q < PIN; ++q) {
            const float v0 = __uint_as_float((unsigned)xq[r][j][q].x), v1 = __uint_as_float((unsigned)xq[r][j][q].y);
            if (v0 > m0) { m0 = v0; a0 = q; }
            if (v1 > m1) { m1 = v1; a1 = q; }
          }
          *reinterpret_cast<float2*>(S.pin_out + po + goff[j]) = make_float2(m0, m1);
          *reinterpret_cast<unsigned short*>(S.pin_idx + po + goff[j]) = (unsigned short)(a0 | (a1 << 8));
        }
        *reinterpret_cast<bf16x2_t*>(xsb + buf * XBUF + loff[j]) = bf16x2_t{(__bf16)m0, (__bf16)m1};
      }
    } else {
#pragma unroll
      for (int j = 0; j < NGL; ++j) {
        // GR = 4 consecutive channels of one sequence (Din % 4 == 0): one 8-byte LDS write
        const bf16x4_t v = __builtin_convertvector(xr[r][j], bf16x4_t);
        *reinterpret_cast<bf16x4_t*>(xsb + buf * XBUF + loff[j]) = v;
      }
    }
  };

  // ---- compute role: fragments of the pre-scaled gate weights, one cell (unit, sequence) per lane
  const int wc = compute ? w : 0;
  const int ag = col & 3;
  int unit[CPL];
  bf16x8_t ufr[CPL][C::KSH], wfr[CPL][KX];
  f32x4_t bias4[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) {
    const int gi = wc + NW * cc;                 // (the cell group: a one-cell-per-lane wave)
    const int au = 4 * gi + (col >> 2);
    unit[cc] = 4 * gi + quad;
    bias4[cc] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (compute) {
#pragma unroll
      for (int s = 0; s < C::KSH; ++s) {
        bf16x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = 32 * s + 8 * quad + j;
          v[j] = (__bf16)(S.U[min(k, H - 1) * G4 + ag * H + au] * (k < H ? 1.0f : 0.0f));
        }
        ufr[cc][s] = v;
      }
#pragma unroll
      for (int s = 0; s < KX; ++s) {
        bf16x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = 32 * s + 8 * quad + j;
          v[j] = (__bf16)(S.W[min(k, Dw - 1) * G4 + ag * H + au] * (k < Dw ? 1.0f : 0.0f));
        }
        wfr[cc][s] = v;
      }
      const int u = unit[cc];
      bias4[cc] = f32x4_t{S.b[u], S.b[H + u], S.b[2 * H + u], S.b[3 * H + u]};
    }
  }
  // this lane's output elements (sequence row0 + col, unit) in the [T][Mp][H] streams
  float* hp[CPL];
  unsigned long long* sp[CPL];
  __bf16* gp[CPL];
  float* cp[CPL];
  const size_t gstride = (size_t)ntiles * NWV * 64;
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) {
    const size_t hoff = (size_t)(row0 + col) * H + unit[cc];
    hp[cc] = S.h + hoff;
    sp[cc] = S.sout != nullptr ? S.sout + hoff : nullptr;
    gp[cc] = S.g + (((size_t)tile * NWV + wc + NW * cc) * 64 + lane) * 4;
    cp[cc] = S.c + ((size_t)tile * NWV + wc + NW * cc) * 64 + lane;
  }
  const bool publish = S.sout != nullptr;
  const bool own_pool = P > 0;

  // ---- a last stage that pools its own output: the pooling lanes (I/O wave 0, or the first 16 H / 4
  // threads) own float4 granules of the [16][H] tile
  constexpr int n_gh = 16 * H / 4;
  constexpr int NPT = IOW ? 64 : NT;             // pooling threads (the publisher wave, or every thread)
  constexpr int NPL = (n_gh + NPT - 1) / NPT;
  PoolAcc pool[NPL];
  const bool publisher = IOW && w == NW + NIOW;
  const bool pooler = IOW ? publisher : wave_uniform(tid < n_gh);
  auto pool_step = [&](int tp) {           // h_tp from hf[tp & 1]
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
      const int gh = (((IOW ? lane : tid) + NPT * q) % n_gh) * 4;
      const float4 v = *reinterpret_cast<const float4*>(&hf[tp & 1][gh / H][gh % H]);
      pool[q].step(v, tp, P, To, S.pout, S.iout, (size_t)row0 * H + gh, hstep);
    }
  };

  // ---- prologue: x_0 in LDS buffer 0, the first D steps' loads in flight
  const bool streamer = IOW ? (!compute && !publisher) : true;
  if (streamer) {
    if constexpr (SRC) {
      // start once the producer is D + LEAD (input) steps ahead: the loads then find their
      // granules. (Starting at once left every load stale: each of the first D steps then paid a
      // full re-poll round trip, ~12 us of lag per stage.)
      constexpr int LEAD = PIN > 1 ? CHAIN_LEAD3 : CHAIN_LEAD1;
      const int tw = min(D + LEAD, T - 1);
      (void)chain_wait(S.xin + xbase + goff[0] + 1 + (size_t)(PIN * tw + PIN - 1) * xstep,
                       tagb | (unsigned)(PIN * tw + PIN - 1), ctl);
    }
    if constexpr (IOW) {
      load_x(0, min(iow, T - 1));            // I/O wave k: x_k
    } else {
#pragma unroll
      for (int r = 0; r < D; ++r) load_x(r, min(r, T - 1));
    }
  }
  __syncthreads();
  if (IOW ? (streamer && iow == 0) : streamer) {
    stage_x(0, 0, 0);
    if (!IOW) load_x(0, min(D, T - 1));
  }
  float c[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) c[cc] = 0.f;
  __syncthreads();

  // (LATEW) step t - 1's outputs, carried in registers over the barrier
  float hvl[CPL], cl[CPL];
  uint2 gl[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) {
    hvl[cc] = cl[cc] = 0.f;
    gl[cc] = make_uint2(0u, 0u);
  }
  // ... and written into the publisher's LDS buffers of step tl
  auto late_write = [&](int tl) {
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
      hf[tl & 1][col][unit[cc]] = hvl[cc];
      if constexpr (TRAIN) {
        gst[tl & 1][(wc + NW * cc) * 64 + lane] = gl[cc];
        cst[tl & 1][(wc + NW * cc) * 64 + lane] = cl[cc];
      }
    }
  };

  // the compute step of time t (reads xs[p], hs[p]; writes hs[p ^ 1], the outputs)
  auto compute_step = [&](int t, auto IO, int rn) {
    constexpr bool DOI = decltype(IO)::value;
    const int p = t & 1;
    chain_mark(pr, t, 0);
    f32x4_t acc[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
      f32x4_t accx = bias4[cc], acch = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KX; ++s) {
        const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(&xs[p][col][32 * s + 8 * quad]);
        accx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[cc][s], bx, accx, 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < C::KSH; ++s) {
        const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(&hs[p][col][32 * s + 8 * quad]);
        // step t - 1's LDS copies for the publisher inside this read's latency, off the path to the
        // barrier (t = 0 writes zeros into buffer 1, which step 1's copies replace before it is read)
        if constexpr (LATEW) {
          if (s == 0 && cc == 0) late_write(t - 1);
        }
        acch = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[cc][s], bh, acch, 0, 0, 0);
      }
      acc[cc] = accx + acch;
    }
    chain_mark(pr, t, 1);
    if constexpr (DOI) {                 // (no I/O waves: every thread also streams x through its ring)
      stage_x(p ^ 1, rn, min(t + 1, T - 1));
      load_x(rn, min(t + 1 + D, T - 1));
    }
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
      const f32x4_t a = acc[cc];
      const int u = unit[cc], cell = (wc + NW * cc) * 64 + lane;
      const float iv = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(chain_gate_scale(0) * a[0]));
      const float fv = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(chain_gate_scale(1) * a[1]));
      const float gv = 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(chain_gate_scale(2) * a[2])) - 1.0f;
      const float ov = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(chain_gate_scale(3) * a[3]));
      c[cc] = fv * c[cc] + iv * gv;
      const float rc = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.8853900817779268f * c[cc]));
      const float hv = (2.0f * ov) * rc - ov;            // o tanh(c)
      hs[p ^ 1][col][u] = (__bf16)hv;
      // the granule that publishes h_t goes out at once, from registers (write-through: the consumer
      // polls it); the bulk outputs (h, packed gates, c) are staged in LDS for the publisher wave, whose
      // wide contiguous stores keep the CU's vector-memory path free for the consumer-side loads
      if (publish) st_granule(sp[cc] + (size_t)t * hstep, hv, tagb | (unsigned)t);
      if constexpr (LATEW) {
        hvl[cc] = hv;
        cl[cc] = c[cc];
        if constexpr (TRAIN) gl[cc] = gates_pack(iv, fv, gv, ov);
      } else if constexpr (IOW) {
        hf[p][col][u] = hv;
        if constexpr (TRAIN) {
          gst[p][cell] = gates_pack(iv, fv, gv, ov);
          cst[p][cell] = c[cc];
        }
      } else {
        if (own_pool) hf[p][col][u] = hv;
        hp[cc][(size_t)t * hstep] = hv;
        if constexpr (TRAIN) {
          *reinterpret_cast<uint2*>(gp[cc] + (size_t)t * gstride * 4) = gates_pack(iv, fv, gv, ov);
          cp[cc][(size_t)t * gstride] = c[cc];
        }
      }
    }
    chain_mark(pr, t, 2);
  };
  // publisher wave: step tp's h tile, gates and c from LDS buffer tp & 1 with 16-byte stores; a whole
  // [16][H] row block of the time-major streams is contiguous. (Publishing the granules from here as
  // well, a step later with 16-byte write-through buffer stores, timed out: consumers never saw them.)
  auto publish_step = [&](int tp) {
    const int pb = tp & 1;
    const size_t tile_off = ((size_t)tp * Mp + row0) * H;
#pragma unroll
    for (int q = lane; q < 16 * H / 4; q += 64) {
      const int e = 4 * q;
      *reinterpret_cast<float4*>(S.h + tile_off + e) = *reinterpret_cast<const float4*>(&hf[pb][e / H][e % H]);
    }
    if constexpr (TRAIN) {
      const size_t cell0 = ((size_t)tp * ntiles + tile) * NCELL;      // this tile's cells of step tp
#pragma unroll
      for (int q = lane; q < NCELL / 2; q += 64)
        *reinterpret_cast<uint4*>(S.g + (cell0 + 2 * q) * 4) = *reinterpret_cast<const uint4*>(&gst[pb][2 * q]);
#pragma unroll
      for (int q = lane; q < NCELL / 4; q += 64)
        *reinterpret_cast<float4*>(S.c + cell0 + 4 * q) = *reinterpret_cast<const float4*>(&cst[pb][4 * q]);
    }
    if (own_pool) pool_step(tp);
  };
  using yes = std::true_type;
  using no = std::false_type;
  if constexpr (IOW) {
    if (compute) {
      if (CHAIN_PRIO > 0) __builtin_amdgcn_s_setprio(CHAIN_PRIO);   // the serial cell math issues first on a shared SIMD
      for (int t = 0; t < T; ++t) {
        compute_step(t, no{}, 0);
        lds_barrier();
        chain_mark(pr, t, 3);
      }
      __builtin_amdgcn_s_setprio(0);
      if constexpr (LATEW) {               // the last step's copies, behind one more barrier of all roles
        late_write(T - 1);
        lds_barrier();
      }
    } else if (publisher) {
      // LATEW: the publisher runs two steps behind (buffer t & 1 holds step t - 2 until the compute
      // waves overwrite it at the top of step t + 1) and drains the last two steps behind the loop
      constexpr int LAG = LATEW ? 2 : 1;
      for (int t = 0; t < T; ++t) {
        if (t >= LAG) publish_step(t - LAG);
        chain_mark_wave(pr, t, 7);         // (the publisher reaches the step barrier)
        lds_barrier();
      }
      if constexpr (LATEW) {
        lds_barrier();
        if (T >= 2) publish_step(T - 2);
      }
      publish_step(T - 1);
    } else {
      // I/O wave k stages the steps s = k (mod D): x_{t+1} in step t, then loads x_{t+1+D}
      // the group's next loads are issued at the top of the step AFTER its staging step (right after
      // that barrier, beside the compute waves' cell math) instead of before the barrier they would
      // hold up; they still land D - 1 steps ahead of their use
      int kt = (iow + D - 1) % D;        // steps until this wave's turn: t = kt, kt + D, ...
      int next_ld = iow == 0 ? D : -1;   // (group 0 staged x_0 in the prologue)
      for (int t = 0; t < T; ++t) {
        if (next_ld >= 0) {
          load_x(0, min(next_ld, T - 1));
          next_ld = -1;
        }
        if (kt == 0 && t + 1 < T) {
          // (profiling: mark 4's clock is stored behind the staging. Stored at once, the mark's own store
          // was what the staging's wait for its loads then waited for: ~450 ticks that no other build has.)
          const long long c4 = chain_clock();
          mark_t = t;
          stage_x((t + 1) & 1, 0, t + 1);
          if (iot == 0) chain_mark_wave(pr, t, 5);
          if (iot == 0) chain_mark_wave_at(pr, t, 4, c4);
          next_ld = t + 1 + D;
        }
        kt = kt == 0 ? D - 1 : kt - 1;
        lds_barrier();
      }
      if constexpr (LATEW) lds_barrier();
    }
  } else {
    for (int t0 = 0; t0 < T; t0 += D) {
#pragma unroll
      for (int r = 0; r < D; ++r) {
        const int t = t0 + r;
        if (t >= T) break;               // (uniform: the last round of the ring may be partial)
        compute_step(t, yes{}, (r + 1 == D) ? 0 : r + 1);
        if (own_pool && pooler && t >= 1) pool_step(t - 1);
        lds_barrier();
        chain_mark(pr, t, 3);
      }
    }
  }
  if constexpr (!IOW) {
    if (own_pool && pooler) pool_step(T - 1);
  }
}

// ---- time4 (H = 128, the CML TimeLayer's last layer, last state only) + head + weighted BCE as one
// more consumer stage of the forward chain (lstm_chain_head_fwd). As its own launch
// (time4_head.hip) it could only start once the whole chain had drained, and its six steps plus
// the head (~22 us) ran serially behind it. Here one workgroup per tile consumes the last chain
// stage's UNPOOLED granules, max-pools them (MaxPooling1D(3); the pooled input and the argmax
// bytes are written for the backward) and runs each step as soon as its three input steps are
// published; the head and the loss follow the last step. 1024 threads with two cells per lane
// (the chain kernel's launch bounds give a lane 128 VGPRs; the standalone kernel's four cells per
// lane need 256). time4_head.hip's saved-state layouts (h; fp32 gates and (c_t, c_{t-1}) in its
// t4_sidx order) are kept, so its backward is unchanged.
struct ChainT4Lds {
  static constexpr int HS = 2 * 16 * (128 + 8) * 2;       // bf16 h_{t-1} (double buffer)
  static constexpr int XS = 2 * 16 * (64 + 8) * 2;        // bf16 x_t (double buffer)
  static constexpr int HL = 16 * (128 + 4) * 4;           // fp32 h_{T-1} for the head
  static constexpr int DHT = 16 * (128 + 4) * 4;          // dh_{T-1} of the head (chain_head_dh)
  // (chain_head_dh's dh tile and scratch follow the head forward's, whose tiles and weight images it reuses)
  static constexpr int HF = ChainHeadFwdLds<128>::BYTES;
  static constexpr int HB = DHT + ChainHeadDhLds<128>::BYTES;
  static constexpr int BYTES = HS + XS + HL + HF + HB;
};

template <bool TRAIN>
__device__ __forceinline__ void chain_t4_stage(const ChainT4 Q, int tile, int ntiles, int Mp, unsigned tagb, int* ctl,
                                               char* smem) {
  constexpr int H = 128, G4 = 4 * H, NW = 16, CPL = 2, KX = 2, KSH = H / 32, HPB = H + 8, XP = 64 + 8;
  static_assert(ChainT4Lds::HS % 16 == 0 && ChainT4Lds::XS % 16 == 0 && ChainT4Lds::HL % 16 == 0, "t4 LDS layout");
  auto hs = reinterpret_cast<__bf16 (*)[16][HPB]>(smem);
  auto xs = reinterpret_cast<__bf16 (*)[16][XP]>(smem + ChainT4Lds::HS);
  float* hl = reinterpret_cast<float*>(smem + ChainT4Lds::HS + ChainT4Lds::XS);
  const int T = Q.T, Din = Q.Din, Dw = Q.Dw;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, quad = lane >> 4;
  const int row0 = tile * 16;

  for (int i = tid; i < 2 * 16 * HPB; i += 1024) (&hs[0][0][0])[i] = (__bf16)0.0f;
  for (int i = tid; i < 2 * 16 * XP; i += 1024) (&xs[0][0][0])[i] = (__bf16)0.0f;
  // input element of this thread: (sequence er, channel ek) of the [16][Din] tile; threads past
  // the tile re-load the last element (every lane of a waiting wave must hold a real granule)
  const int n_el = 16 * Din;
  const bool own = tid < n_el;
  const int el = min(tid, n_el - 1), er = el / Din, ek = el % Din;
  const size_t xstep = (size_t)Mp * Din, xoff = (size_t)(row0 + er) * Din + ek;
  unsigned long long xq[3];
  auto load_x = [&](int tx) {
#pragma unroll
    for (int r = 0; r < 3; ++r) xq[r] = ld_granule(Q.xin + xoff + (size_t)(3 * tx + r) * xstep);
  };
  // the first input's granules are requested before the weight gathers (their latency overlaps)
  load_x(0);

  // weights -> permuted A fragments (as chain_stage) straight from global memory: the gathers'
  // latency is hidden behind the wait for the first input
  bf16x8_t ufr[CPL][KSH], wfr[CPL][KX];
  f32x4_t bias4[CPL];
  int unit[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) {
    const int gi = w + NW * cc;
    const int au = 4 * gi + (col >> 2), ag = col & 3;
    unit[cc] = 4 * gi + quad;
#pragma unroll
    for (int s = 0; s < KSH; ++s) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)Q.U[(32 * s + 8 * quad + j) * G4 + ag * H + au];
      ufr[cc][s] = v;
    }
#pragma unroll
    for (int s = 0; s < KX; ++s) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * quad + j;
        v[j] = (__bf16)(Q.W[min(k, Dw - 1) * G4 + ag * H + au] * (k < Dw ? 1.0f : 0.0f));
      }
      wfr[cc][s] = v;
    }
    const int u = unit[cc];
    bias4[cc] = f32x4_t{Q.b[u], Q.b[H + u], Q.b[2 * H + u], Q.b[3 * H + u]};
  }

  // x_tx = MaxPool(3) of the producer's h at 3 tx .. 3 tx + 2 (first maximum wins, its byte kept)
  auto stage_x = [&](int buf, int tx) {
    bool bad = false;
#pragma unroll
    for (int r = 0; r < 3; ++r) bad |= (unsigned)(xq[r] >> 32) != (tagb | (unsigned)(3 * tx + r));
    if (__builtin_amdgcn_ballot_w64(bad) != 0) {
      // re-poll all three granules at once, inline (a call to chain_wait here made the compiler keep
      // live registers in scratch around it: two scratch reloads in every step of this loop)
      const int lim0 = __hip_atomic_load(ctl + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int lim = lim0 > 0 ? lim0 : CHAIN_SPIN;
      for (int it = 0;; ++it) {
        __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int r = 0; r < 3; ++r) xq[r] = ld_granule(Q.xin + xoff + (size_t)(3 * tx + r) * xstep);
        bad = false;
#pragma unroll
        for (int r = 0; r < 3; ++r) bad |= (unsigned)(xq[r] >> 32) != (tagb | (unsigned)(3 * tx + r));
        if (__builtin_amdgcn_ballot_w64(bad) == 0) break;
        if (it >= lim) {
          __hip_atomic_store(ctl + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
    }
    float m = __uint_as_float((unsigned)xq[0]);
    unsigned arg = 0;
#pragma unroll
    for (int r = 1; r < 3; ++r) {
      const float v = __uint_as_float((unsigned)xq[r]);
      if (v > m) { m = v; arg = r; }
    }
    if (own) {
      Q.pin_out[xoff + (size_t)tx * xstep] = m;
      Q.pin_idx[xoff + (size_t)tx * xstep] = (unsigned char)arg;
      xs[buf][er][ek] = (__bf16)m;
    }
  };

  __syncthreads();                                // LDS zeroed
  stage_x(0, 0);
  if (T > 1) load_x(1);
  float c[CPL];
#pragma unroll
  for (int cc = 0; cc < CPL; ++cc) c[cc] = 0.f;
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const int p = t & 1;
    f32x4_t acc[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
      f32x4_t accx = bias4[cc], acch = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KX; ++s) {
        const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(&xs[p][col][32 * s + 8 * quad]);
        accx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[cc][s], bx, accx, 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < KSH; ++s) {
        const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(&hs[p][col][32 * s + 8 * quad]);
        acch = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[cc][s], bh, acch, 0, 0, 0);
      }
      acc[cc] = accx + acch;
    }
    if (wave_uniform(t + 1 < T)) {
      stage_x(p ^ 1, t + 1);
      if (wave_uniform(t + 2 < T)) load_x(t + 2);
    }
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
      const float iv = sigmoidf_fast(acc[cc][0]);
      const float fv = sigmoidf_fast(acc[cc][1]);
      const float gv = tanhf_fast(acc[cc][2]);
      const float ov = sigmoidf_fast(acc[cc][3]);
      const float cold = c[cc];
      c[cc] = fv * cold + iv * gv;
      const float hv = ov * tanhf_fast(c[cc]);
      const int u = unit[cc];
      hs[p ^ 1][col][u] = (__bf16)hv;
      Q.h[((size_t)t * Mp + row0 + col) * H + u] = hv;
      if (t == T - 1) hl[col * (H + 4) + u] = hv;
      if constexpr (TRAIN) {
        const int gi = w + NW * cc;                 // time4_head.hip's (wave, cell) of this cell
        const size_t o = ((((size_t)t * ntiles + tile) * 8 + (gi & 7)) * 4 + (gi >> 3)) * 64 + lane;
        *reinterpret_cast<float4*>(Q.g + o * 4) = make_float4(iv, fv, gv, ov);
        *reinterpret_cast<float2*>(Q.c + o * 2) = make_float2(c[cc], cold);
      }
    }
    lds_barrier();
  }
  __syncthreads();
}

static constexpr int CHAIN_LDS = ChainT4Lds::BYTES > CHAIN_LDS_STAGE ? ChainT4Lds::BYTES : CHAIN_LDS_STAGE;

template <bool TRAIN>
__global__ __launch_bounds__(1024) void lstm_chain_fwd_kernel(ChainArgs A) {
  const int nblk = gridDim.x;
  __shared__ __attribute__((aligned(16))) char smem[CHAIN_LDS];
  if ((int)blockIdx.x >= A.ns * A.nt8) {
    int r = (int)blockIdx.x - A.ns * A.nt8;
    if (A.t4.on) {
      if (r < A.nt8) {                            // time4 + head stage of tile r
        if (r < A.ntiles) {
          if (threadIdx.x == 0) A.trace[2 * blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime();
          const unsigned tagb = chain_tag_base((unsigned)__hip_atomic_load(A.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          // the head's weight images go to LDS first: this workgroup then waits ~60 us for its first
          // input anyway (the chain's stages are all far behind), and the head runs right after the
          // last time4 step
          constexpr int HOFF = ChainT4Lds::HS + ChainT4Lds::XS + ChainT4Lds::HL;
          float* hW1 = ch_head_fwd_weights<128>(smem + HOFF);
          ch_stage_weights<128>(A.t4.hd, hW1, hW1 + 128 * CH_WP);
          if (A.gp.on) {                          // the labels come from this launch's GCN producers
            if (threadIdx.x == 0) chain_wait_count(A.ctl + 10, A.gp.Mp, A.ctl);
            __syncthreads();
          }
          const bool pre = TRAIN && A.t4.hb != nullptr;
          constexpr int OFF = HOFF + ChainT4Lds::HF;     // (after the head forward's scratch and weights)
          char* dhscr = smem + OFF + ChainT4Lds::DHT;
          // the mask's partial sums (the loss gradient's 1 / max(n, 1)) as well: the labels are complete
          // here and the loads cost nothing during that wait; the time4 stage's barriers publish them
          if (pre) ch_mask_partials(A.t4.hd.mask, A.t4.hd.M, ch_head_dh_red<128>(dhscr));
          chain_t4_stage<TRAIN>(A.t4, r, A.ntiles, A.Mp, tagb, A.ctl, smem);
          long long* mk = blockIdx.x < 64 ? A.trace + 512 + blockIdx.x : nullptr;   // (trace: phase ends)
          if (mk != nullptr && threadIdx.x == 0) mk[0] = (long long)__builtin_amdgcn_s_memrealtime();
          if (threadIdx.x >= 64 * CH_NW) return;    // the head runs on 8 waves (the rest exit)
          ChainHeadKeep keep;
          chain_head_fwd<128>(A.t4.hd, r, A.ntiles, reinterpret_cast<const float*>(smem + ChainT4Lds::HS + ChainT4Lds::XS),
                              smem + HOFF, true, !pre, pre ? ch_head_dh_sz1<128>(dhscr) : nullptr, &keep);
          if (mk != nullptr && threadIdx.x == 0) mk[64] = (long long)__builtin_amdgcn_s_memrealtime();
          if constexpr (TRAIN) {
            if (A.t4.hb != nullptr) {
              // the hand-over to the backward launch: the head forward above continues into the
              // backward-to-dh (it kept z1, a1, z2 and the logit; dL/dloss = 1, scaled there), so the
              // backward's time4 stage starts its reverse steps at once. The head's weight-gradient
              // records are NOT built here, on the step's critical path between the two recurrences:
              // the backward launch's time4 workgroups build them after their reverse steps, where
              // they would otherwise idle until the chain has drained (chain_t4_bwd_stage).
              float* dhs = reinterpret_cast<float*>(smem + OFF);
              chain_head_dh<128>(A.t4.hd, r, keep, smem + HOFF, dhscr, dhs);
              __syncthreads();
              for (int e = ch_tid(); e < 16 * 128; e += 64 * CH_NW)
                A.t4.hb[((size_t)r * 16 + e / 128) * 128 + e % 128] = dhs[(e / 128) * 132 + e % 128];
              // the loss hand-off last: its stores' acknowledgement wait then overlaps nothing it delays
              chain_head_fwd_handoff<128>(A.t4.hd, r, A.ntiles, smem + HOFF);
            }
          }
          __syncthreads();
          if (threadIdx.x == 0) A.trace[2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime();
        }
        chain_finish(A.ctl, nblk);
        return;
      }
      r -= A.nt8;
    }
    if (r < A.npk) {
      const int f = r * 1024 + (int)threadIdx.x;  // packing workgroups
      if (A.pk != nullptr && f < T4PK_ALL) t4_pack_one(f, A.pkU, A.pkW, A.pkDw, A.pk);
    } else if (A.cf.on && r - A.npk < A.cf.Mp) {  // GCN backward coefficients of sample row r - npk
      gcn_coef_fwd_body<2, 16>(A.cf, r - A.npk, smem);
    } else if (A.gp.on && r - A.npk - (A.cf.on ? A.cf.Mp : 0) < A.gp.Mp) {   // GCN forward producer
      // (trace: start / end at [2 blockIdx]; rows < 32: phase A loads in / BatchNorm prepped / the
      // first pass's rows stored at [640 + 4 row + 0..2])
      if (threadIdx.x == 0 && blockIdx.x < 256) A.trace[2 * blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime();
      const unsigned E = (unsigned)__hip_atomic_load(A.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int row = r - A.npk - (A.cf.on ? A.cf.Mp : 0);
      gcn_prod_body<2, 16>(A.gp, row, chain_tag_base(E), A.ctl + 10, smem, row < 32 ? A.trace + 640 + 4 * row : nullptr);
      if (threadIdx.x == 0 && blockIdx.x < 256) A.trace[2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime();
    }
    chain_finish(A.ctl, nblk);
    return;
  }
  const int s = blockIdx.x / A.nt8, tile = blockIdx.x % A.nt8;
  if (s >= A.ns || tile >= A.ntiles) {
    chain_finish(A.ctl, nblk);
    return;
  }
  if (threadIdx.x == 0) A.trace[2 * blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime();
  const unsigned E = (unsigned)__hip_atomic_load(A.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned tagb = chain_tag_base(E);
  // (a local copy: field-wise scalar loads of the kernel arguments; a reference into the by-value
  // argument array made the compiler copy the whole array to scratch)
  const ChainStage S = A.st[s];
  const int H = S.H, KX = S.KX;
  const bool src = s > 0 || A.gp.on;              // (stage 0 then streams the GCN producers' granules)
#define GQ_CHAIN_BODYX(HH, KXX, DD, SRCV, PINV, XCV)                                    \
  {                                                                                     \
    constexpr int DS = chain_stage_d(HH, KXX, DD);                                      \
    if (threadIdx.x >= chain_live_threads(ChainCfg<HH>::NT, DS, KXX, SRCV, PINV, HH)) return; \
    chain_stage<HH, TRAIN, KXX, DS, SRCV, PINV, XCV>(S, tile, A.ntiles, A.Mp, tagb, A.ctl, smem); \
  }
#define GQ_CHAIN_BODY(HH, KXX, DD, SRCV, PINV) GQ_CHAIN_BODYX(HH, KXX, DD, SRCV, PINV, 32 * KXX)
#define GQ_CHAIN_SRC(HH, PINV, DD)                                                      \
  if (KX == 1) GQ_CHAIN_BODY(HH, 1, DD, true, PINV) else GQ_CHAIN_BODY(HH, 2, DD, true, PINV)
// the H = 16 non-pooling stream consumer (it runs at its producer's rate): a ring depth of its own,
// and with Din <= 16 its I/O waves load a 16-channel tile's granules only
#define GQ_CHAIN_SRC16                                                                  \
  if (KX == 1 && S.Din <= 16) GQ_CHAIN_BODYX(16, 1, CHAIN_D16S, true, 1, 16) \
  else GQ_CHAIN_SRC(16, 1, CHAIN_D16S)
#define GQ_CHAIN_KX(HH, SRC1)                                                           \
  if (src) { if (S.PIN == 3) { GQ_CHAIN_SRC(HH, 3, CHAIN_D3) } else { SRC1 } }          \
  else { if (KX == 1) GQ_CHAIN_BODY(HH, 1, CHAIN_D0, false, 1) else GQ_CHAIN_BODY(HH, 2, CHAIN_D0, false, 1) }
  if (H == 16) GQ_CHAIN_KX(16, GQ_CHAIN_SRC16)
  else if (H == 32) GQ_CHAIN_KX(32, GQ_CHAIN_SRC(32, 1, CHAIN_D))
  else GQ_CHAIN_KX(64, GQ_CHAIN_SRC(64, 1, CHAIN_D))
#undef GQ_CHAIN_SRC16
#undef GQ_CHAIN_BODYX
#undef GQ_CHAIN_KX
#undef GQ_CHAIN_SRC
#undef GQ_CHAIN_BODY
  __syncthreads();
  if (threadIdx.x == 0) A.trace[2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime();
  chain_finish(A.ctl, nblk);
}

// time4 + head as a chain stage (lstm_chain_head_fwd): its weights, the head and the loss inputs
struct T4Host {
  const at::Tensor* b;
  at::TensorList head;
  const at::Tensor* y;
  const at::Tensor* mask;
  int64_t M;
  double alpha1, alpha2, w0, w1;
  at::Tensor sums, hist;
};

// x [T, Mp, Din] (Din % 4 == 0, 16-B aligned); per stage W [Dw, 4H], U [H, 4H], b [4H];
// pool[s] > 0: MaxPooling1D(pool[s]) after stage s. Returns per stage [h, g, c, pooled, idx].
static std::vector<at::Tensor> chain_fwd_impl(const at::Tensor& x, at::TensorList W, at::TensorList U,
                                              at::TensorList b, at::IntArrayRef pool, bool train, const at::Tensor* pkW,
                                              const at::Tensor* pkU, const T4Host* t4 = nullptr) {
  check_f32_cuda(x, "x");
  const int ns = (int)W.size();
  TORCH_CHECK(ns >= 1 && ns <= CHAIN_MAX && (int)U.size() == ns && (int)b.size() == ns && (int)pool.size() == ns,
              "lstm_chain: stage lists");
  TORCH_CHECK(x.dim() == 3 && x.is_contiguous(), "lstm_chain: x must be a contiguous [T, Mp, Din]");
  const int Mp = (int)x.size(1);
  TORCH_CHECK(Mp % 16 == 0, "lstm_chain: Mp must be a multiple of 16");
  const int ntiles = Mp / 16, nt8 = (ntiles + 7) / 8 * 8;
  TORCH_CHECK(ns * nt8 <= chain_capacity(x.get_device()), "lstm_chain: ", ns * nt8,
              " workgroups cannot all be resident on this device");
  TORCH_CHECK(x.size(2) % 4 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "lstm_chain: x channels must be float4 granules");
  c10::DeviceGuard guard(x.device());
  auto opt = x.options();
  ChainArgs A{};
  A.ns = ns;
  A.ntiles = ntiles;
  A.nt8 = nt8;
  A.Mp = Mp;
  A.ctl = chain_ctl(x.get_device());
  A.trace = chain_trace_buf(x.get_device());
  chain_prof_clear(x.get_device());
  std::vector<at::Tensor> out;
  at::Tensor prev_stream;
  int T = (int)x.size(0), Din = (int)x.size(2);
  for (int s = 0; s < ns; ++s) {
    for (const at::Tensor* t : {&W[s], &U[s], &b[s]}) check_f32_cuda(*t, "lstm_chain weight");
    const int H = (int)U[s].size(0), Dw = (int)W[s].size(0);
    TORCH_CHECK(H == 16 || H == 32 || H == 64, "lstm_chain: hidden size ", H);
    TORCH_CHECK(W[s].size(1) == 4 * H && U[s].size(1) == 4 * H && b[s].numel() == 4 * H, "lstm_chain: weights");
    TORCH_CHECK(Dw <= Din && Din <= 64 && (s == 0 || Din <= H), "lstm_chain: stage ", s, " input width ", Din);
    TORCH_CHECK(T >= 1 && T < 4096, "lstm_chain: sequence length");
    const int P = (int)pool[s];
    const bool last = s + 1 == ns && t4 == nullptr;   // (time4 consumes the last chain stage)
    TORCH_CHECK(last || P == 0 || P == 3, "lstm_chain: pools between stages must be 3 (got ", P, ")");
    TORCH_CHECK(t4 == nullptr || s + 1 < ns || P == 3, "lstm_chain_head_fwd: the last chain stage must pool by 3");
    ChainStage& S = A.st[s];
    S.x = s == 0 ? x.data_ptr<float>() : nullptr;
    S.xin = s == 0 ? nullptr : reinterpret_cast<const unsigned long long*>(prev_stream.data_ptr<int64_t>());
    S.W = W[s].data_ptr<float>();
    S.U = U[s].data_ptr<float>();
    S.b = b[s].data_ptr<float>();
    at::Tensor h = at::empty({T + 1, Mp, H}, opt);
    at::Tensor g = train ? at::empty({T + 1, Mp, H, 4}, opt.dtype(at::kBFloat16)) : at::empty({0}, opt);
    at::Tensor c = train ? at::empty({T + 1, Mp, H}, opt) : at::empty({0}, opt);
    at::Tensor pooled, pidx;
    const TmPool pl = tm_pool_outputs(P, T, Mp, H, opt, pooled, pidx);
    const int To = P > 0 ? T / P : T;
    TORCH_CHECK(To >= 1, "lstm_chain: pooled length");
    // the stream carries the UNPOOLED h: a pooling consumer pools it (and writes pooled / pidx)
    at::Tensor so = !last ? at::empty({T, Mp, H}, opt.dtype(at::kLong)) : at::Tensor();
    S.h = h.data_ptr<float>();
    S.g = train ? bf16_ptr(g) : nullptr;
    S.c = train ? c.data_ptr<float>() : nullptr;
    S.sout = so.defined() ? reinterpret_cast<unsigned long long*>(so.data_ptr<int64_t>()) : nullptr;
    S.pout = last ? pl.out : nullptr;
    S.iout = last ? pl.idx : nullptr;
    S.P = last ? P : 0;
    if (!last && P > 0 && s + 1 < ns) {          // the next stage pools this stage's output
      A.st[s + 1].pin_out = pooled.data_ptr<float>();
      A.st[s + 1].pin_idx = pidx.data_ptr<uint8_t>();
    } else if (!last && P > 0) {                 // ... or time4 does
      A.t4.pin_out = pooled.data_ptr<float>();
      A.t4.pin_idx = pidx.data_ptr<uint8_t>();
    }
    S.H = H;
    S.T = T;
    S.Din = Din;
    S.Dw = Dw;
    S.KX = (Din + 31) / 32;
    S.PIN = s > 0 ? std::max(1, (int)pool[s - 1]) : 1;
    // a stage without I/O waves (H = 64) streams one granule per thread (chain_stage NGL)
    TORCH_CHECK(H < 64 || 16 * Din / (s == 0 ? 4 : 2) <= 64 * TMC<64>::NW, "lstm_chain: stage ", s, " input tile");
    TORCH_CHECK(s == 0 || (long)T * Mp * Din * 8 < (1L << 31), "lstm_chain: stage ", s, " input stream too large");
    TORCH_CHECK(s == 0 || Din % 2 == 0, "lstm_chain: stage ", s, " input width must be even");
    TORCH_CHECK(s > 0 || Din % 4 == 0, "lstm_chain: the input width must be a multiple of 4");
    S.prof = chain_prof_rows(x.get_device(), s);
    out.insert(out.end(), {h.narrow(0, 0, T), g, c, pooled, pidx});
    if (so.defined()) out.push_back(so);        // kept alive until the launch is enqueued
    prev_stream = so;
    T = To;
    Din = H;
  }
  int nblk = ns * nt8;
  std::vector<at::Tensor> t4out;
  at::Tensor hb_t;
  if (t4 != nullptr) {
    TORCH_CHECK(pkW != nullptr && pkU != nullptr, "lstm_chain_head_fwd: time4 weights");
    check_f32_cuda(*t4->b, "bt4");
    const int Dw4 = (int)pkW->size(0);
    TORCH_CHECK(T >= 1 && T <= 16, "lstm_chain_head_fwd: time4 sequence length 1..16 (got ", T, ")");
    TORCH_CHECK(Din <= 64 && Dw4 >= 1 && Dw4 <= Din && t4->b->numel() == 512, "lstm_chain_head_fwd: time4 input width");
    ChainT4& Q = A.t4;
    Q.on = 1;
    Q.xin = reinterpret_cast<const unsigned long long*>(prev_stream.data_ptr<int64_t>());
    Q.W = pkW->data_ptr<float>();
    Q.U = pkU->data_ptr<float>();
    Q.b = t4->b->data_ptr<float>();
    at::Tensor h4 = at::empty({T, Mp, 128}, opt);
    at::Tensor g4 = train ? at::empty({(long)T * Mp * 128 * 4}, opt) : at::empty({0}, opt);
    at::Tensor c4 = train ? at::empty({(long)T * Mp * 128 * 2}, opt) : at::empty({0}, opt);
    Q.h = h4.data_ptr<float>();
    Q.g = train ? g4.data_ptr<float>() : nullptr;
    Q.c = train ? c4.data_ptr<float>() : nullptr;
    Q.T = T;
    Q.Din = Din;
    Q.Dw = Dw4;
    at::Tensor logits, loss, part;
    t4_head_fwd_args(Q.hd, t4->head, *t4->y, *t4->mask, t4->M, Mp, t4->alpha1, t4->alpha2, t4->w0, t4->w1, t4->sums,
                     t4->hist, logits, loss, part);
    t4out = {h4, g4, c4, logits, loss, part};
    // the head's dh_{T-1} computed by this launch (GNNQC_HEAD_BWD_IN_FWD=0: the backward launch runs
    // the whole head backward before its reverse steps)
    const char* hbe = std::getenv("GNNQC_HEAD_BWD_IN_FWD");
    if (train && !(hbe != nullptr && hbe[0] == '0')) {
      hb_t = at::empty({(long)ntiles * 16 * 128}, opt);
      Q.hb = hb_t.data_ptr<float>();
    } else {
      hb_t = at::empty({0}, opt);
    }
    nblk += nt8;
  }
  at::Tensor pk;
  if (pkW != nullptr) {
    check_f32_cuda(*pkW, "Wt4");
    check_f32_cuda(*pkU, "Ut4");
    TORCH_CHECK(pkU->size(0) == 128 && pkU->size(1) == 512 && pkW->size(1) == 512 && pkW->size(0) <= 64,
                "lstm_chain_fwd_pack: time4 weights must be [<=64, 512] and [128, 512]");
    pk = at::empty({(long)T4PK_ALL * 4}, opt);                // 16 B per fragment (forward + backward)
    A.pkU = pkU->data_ptr<float>();
    A.pkW = pkW->data_ptr<float>();
    A.pkDw = (int)pkW->size(0);
    A.pk = reinterpret_cast<bf16x8_t*>(pk.data_ptr<float>());
    A.npk = (T4PK_ALL + 1023) / 1024;
    nblk += A.npk;
    TORCH_CHECK(nblk <= chain_capacity(x.get_device()), "lstm_chain: ", nblk,
                " workgroups cannot all be resident on this device");
  }
  // a deferred GCN forward (gcn_fused_fwd defer) whose output is this launch's input runs as
  // producer workgroups of this launch (the first stage streams their granules, the head waits for
  // their labels); any other pending one runs on its own first
  std::vector<at::Tensor> gp_keep;
  {
    const int dev = x.get_device();
    const GcnProdJob& P = gcn_pending(dev).prod;
    if (P.on) {
      const int H0 = A.st[0].H, Din0 = A.st[0].Din;
      const bool mine = train && t4 != nullptr && P.out == x.data_ptr<float>() && P.Mp == Mp &&
                        P.Cp == Din0 && P.D.T == (int)x.size(0) && Din0 % 2 == 0 &&
                        (H0 < 64 || 16 * Din0 / 2 <= 64 * TMC<64>::NW) &&
                        (long)P.D.T * Mp * Din0 * 8 < (1L << 31) && nblk + P.Mp <= chain_capacity(dev);
      if (mine) {
        static_assert(GcnProdLds::BYTES <= CHAIN_LDS, "GCN producer LDS");
        gcn_prod_take(dev, A.gp, gp_keep);
        A.st[0].xin = A.gp.gout;
        nblk += A.gp.Mp;
      } else {
        gcn_prod_flush_dev(dev);
      }
    }
  }
  // a pending GCN coefficient job (gcn_fused_fwd, side mode) rides on this launch when its
  // workgroups fit the co-resident grid as well; else it stays pending (gcn_coef_flush runs it)
  std::vector<at::Tensor> cf_keep;
  if (gcn_pending(x.get_device()).job.on && train &&
      nblk + gcn_pending(x.get_device()).job.Mp <= chain_capacity(x.get_device())) {
    static_assert(GcnCoefFwdLds::BYTES <= CHAIN_LDS, "coefficient job LDS");
    gcn_coef_take(x.get_device(), A.cf, cf_keep);
    nblk += A.cf.Mp;
  }
  hipLaunchKernelGGL(train ? lstm_chain_fwd_kernel<true> : lstm_chain_fwd_kernel<false>, dim3(nblk), dim3(1024), 0, stream(), A);
  GQ_LAUNCH_CHECK();
  // drop the stream buffers from the result (the caching allocator orders their reuse)
  std::vector<at::Tensor> res;
  for (auto& t : out)
    if (t.scalar_type() != at::kLong) res.push_back(t);
  if (pk.defined()) res.push_back(pk);
  if (hb_t.defined()) res.push_back(hb_t);        // (headed launch: [.., pk, hb, h4, g4, c4, logits, loss])
  for (int i = 0; i < 5 && i < (int)t4out.size(); ++i) res.push_back(t4out[i]);
  return res;
}

std::vector<at::Tensor> lstm_chain_fwd(const at::Tensor& x, at::TensorList W, at::TensorList U, at::TensorList b,
                                       at::IntArrayRef pool, bool train) {
  return chain_fwd_impl(x, W, U, b, pool, train, nullptr, nullptr);
}

// The chain forward, whose spare workgroups also build the time4 kernel's fragment image of
// (Wt4 [Din, 512], Ut4 [128, 512]); the image is appended to the result.
std::vector<at::Tensor> lstm_chain_fwd_pack(const at::Tensor& x, at::TensorList W, at::TensorList U,
                                            at::TensorList b, at::IntArrayRef pool, bool train, const at::Tensor& Wt4,
                                            const at::Tensor& Ut4) {
  return chain_fwd_impl(x, W, U, b, pool, train, &Wt4, &Ut4);
}

// The chain forward with time4 (Wt4 [Din, 512], Ut4 [128, 512], bt4 [512], last state only) and the
// classifier head + weighted BCE (head = [W1, b1, W2, b2, W3, b3], y / mask [M]) as one more stage
// consuming the last chain stage's output, which must be max-pooled by 3 (chain_t4_stage). Returns
// lstm_chain_fwd_pack's result followed by [h4 [T4, Mp, 128], g4, c4, logits [M], loss [1]] (the
// outputs of time4_head_fwd); with sums / hist non-empty the metric accumulators are updated.
std::vector<at::Tensor> lstm_chain_head_fwd(const at::Tensor& x, at::TensorList W, at::TensorList U, at::TensorList b,
                                            at::IntArrayRef pool, bool train, const at::Tensor& Wt4,
                                            const at::Tensor& Ut4, const at::Tensor& bt4, at::TensorList head,
                                            const at::Tensor& y, const at::Tensor& mask, int64_t M, double alpha1,
                                            double alpha2, double w0, double w1, at::Tensor sums, at::Tensor hist) {
  T4Host h4{&bt4, head, &y, &mask, M, alpha1, alpha2, w0, w1, sums, hist};
  return chain_fwd_impl(x, W, U, b, pool, train, &Wt4, &Ut4, &h4);
}

int chain_fwd_occupancy() {
  return std::min(chain_occupancy(reinterpret_cast<const void*>(&lstm_chain_fwd_kernel<true>)),
                  chain_occupancy(reinterpret_cast<const void*>(&lstm_chain_fwd_kernel<false>)));
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("lstm_chain_fwd", &gq::lstm_chain_fwd);
  m.impl("lstm_chain_fwd_pack", &gq::lstm_chain_fwd_pack);
  m.impl("lstm_chain_head_fwd", &gq::lstm_chain_head_fwd);
}
