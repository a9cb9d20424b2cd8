// Cross-CU layer pipeline for the forward of a time-major LSTM stack (gfx950).
//
// The per-layer forward kernels (lstm_tm_fwd.hip) run one after another: with the CML batch a
// recurrence occupies 8 of the 256 CUs, and the stack's six recurrences (plus three pool
// launches) are a serial sum. Sequences never mix across layers, so tile j of layer k+1
// only needs tile j of layer k - and only up to the step it is at. This kernel runs all
// layers of the stack at once: workgroup (stage s, tile j) computes layer s of tile j on
// its own CU and consumes layer s-1's output AS IT IS PRODUCED, a few steps behind.
//
// Hand-off (MI355X_MICROARCH.md "Workgroup dispatch ... inter-workgroup visibility", R2
// granules): the producer writes every output element a second time as an 8-byte
// {value, tag} granule with an agent-scope (sc1, write-through) store; the consumer's
// prefetch ring loads granules with agent-scope (sc1, L1-bypassing) loads and checks the
// tag (launch epoch | time index) when it stages x_t into LDS; a wave whose granules are not
// there yet re-polls (bounded; a timeout sets a flag instead of hanging). The producer
// never waits, the consumer only when it catches up. An 8-byte granule is written and read
// untorn, so no fence or flag ordering is needed.
//
// The launch epoch lives in device memory (ctl[0]) and is advanced by the last workgroup
// to finish, so HIP-graph replays get fresh tags and stale granules of an earlier launch
// at the same address never match. All workgroups must be co-resident (grid <= 256 of
// 1024-thread workgroups, checked on the host): a consumer spins only on producers that
// are already running. Workgroups of stage s for tile j have the same blockIdx % 8, so
// under the observed round-robin placement one tile's whole stack shares an XCD (speed only).
//
// A MaxPooling1D(3) between two stages is done by the CONSUMER while staging its input
// (three granules per element, max + first-max argmax byte): the producer's own per-step
// pooling lengthened its serial chain by ~110 ns per step (58 -> 78 us for the first pooled
// CML layer), while the consumer, running at a third of the producer's step rate, has slack.
// Each stage also writes everything the per-layer kernels write (h, gate / cell state for
// the backward, pooled output + argmax bytes), so the backward is unchanged.
#include "chain_head.h"
#include "chain_wgrad.h"
#include "common.h"
#include "gcn_fused.h"
#include "lstm_grads_body.h"
#include "lstm_tm_common.h"

#include <cstdlib>
#include <type_traits>

namespace gq {

typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

static constexpr int CHAIN_MAX = 8;
static constexpr int CHAIN_SPIN = 1 << 20;
// granule ring depth of a non-pooling consumer: an sc1 load of a line another CU wrote
// through to memory takes microseconds under load, D steps of ~0.33 us each must cover it.
// D, LEAD1 and CHAINB_LEAD (below) from a same-box sweep of compile-time variants
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
#ifndef CHAIN_LD16
#define CHAIN_LD16 0         // 1: one 16-byte buffer load per granule pair (measured: stale reads, ~4.5k re-polls per launch)
#endif
#ifndef CHAIN_W_SLEEP
#define CHAIN_W_SLEEP 0      // chain_wait back-off: s_sleep argument (x 64 clocks) per nap unit (8 / 8: 0.284 ms/step,
#endif
#ifndef CHAIN_W_NAPMAX
#define CHAIN_W_NAPMAX 1     //   2 / 4: 0.278, 0 / 1: 0.275-0.277: lane 0's load latency paces the poll) and the largest nap
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

__device__ __forceinline__ unsigned long long ld_granule(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void st_granule(unsigned long long* p, float v, unsigned tag) {
  __hip_atomic_store(p, ((unsigned long long)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// slow path: lane 0 alone polls (its granule) with a growing back-off, then the wave checks
// every lane's granule. (All 64 lanes of every waiting wave polling back-to-back loaded the
// memory system enough to slow the running stages' own streams severalfold.)
template <bool INL>
__device__ __forceinline__ unsigned long long chain_wait_body(const unsigned long long* p, unsigned want, int* ctl);
__device__ __noinline__ unsigned long long chain_wait(const unsigned long long* p, unsigned want, int* ctl) {
  return chain_wait_body<false>(p, want, ctl);
}
// inlined form for the forward I/O waves: a call in their step loop made the compiler drain vmcnt
// at the tag checks (the whole x ring waited for each step)
__device__ __forceinline__ unsigned long long chain_wait_inl(const unsigned long long* p, unsigned want, int* ctl) {
  return chain_wait_body<true>(p, want, ctl);
}
template <bool INL>
__device__ __forceinline__ unsigned long long chain_wait_body(const unsigned long long* p, unsigned want, int* ctl) {
  unsigned long long v = 0;
  const bool l0 = (threadIdx.x & 63) == 0;
#ifdef GQ_CHAIN_PROF
  if (l0) __hip_atomic_fetch_add(ctl + 9, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-polls (diagnostics)
#endif
  int nap = 1;
  // ctl[6] != 0: a debug spin limit (tests force a timeout with it)
  const int lim0 = __hip_atomic_load(ctl + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int lim = lim0 > 0 ? lim0 : CHAIN_SPIN;
  for (int it = 0; it < lim; ++it) {
    unsigned t0 = want;
    if (l0) t0 = (unsigned)(ld_granule(p) >> 32);
    if ((unsigned)__builtin_amdgcn_readfirstlane((int)t0) == want) {
      v = ld_granule(p);
      if (__builtin_amdgcn_ballot_w64((unsigned)(v >> 32) != want) == 0) return v;
    }
    for (int k = 0; k < nap; ++k) __builtin_amdgcn_s_sleep(CHAIN_W_SLEEP);
    nap = min(nap * 2, CHAIN_W_NAPMAX);
  }
  __hip_atomic_store(ctl + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return v;
}

// one thread: wait (bounded, back-off) until the counter *p reaches n; the hand-off data behind it
// is read with agent-scope loads. A timeout flags the step (ctl[2]) as the granule waits do.
__device__ __forceinline__ void chain_wait_count(const int* p, int n, int* ctl) {
  const int lim0 = __hip_atomic_load(ctl + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int lim = lim0 > 0 ? lim0 : CHAIN_SPIN;
  int nap = 1;
  for (int it = 0; it < lim; ++it) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n) return;
    for (int k = 0; k < nap; ++k) __builtin_amdgcn_s_sleep(CHAIN_W_SLEEP);
    nap = min(nap * 2, CHAIN_W_NAPMAX);
  }
  __hip_atomic_store(ctl + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Per-step phase clocks of tile 0 (s_memtime: shader clock ticks) into pr[step][8] for the first
// CHAIN_PROF_STEPS steps; pr is workgroup-uniform (nullptr: off). Compiled in only with
// -DGQ_CHAIN_PROF (GNNQC_CHAIN_PROF_BUILD=1 at build time): even when off, the marks' clock reads
// and conditional stores kept the compiler from overlapping the step phases (chain forward 107 ->
// 131 us, backward 124 -> 155 us, measured).
static constexpr int CHAIN_PROF_STEPS = 64;
// (one more row per stage: word 0 counts the stage's re-poll rounds, all tiles)
static constexpr int CHAIN_PROF_ROWS = CHAIN_PROF_STEPS + 1;
#ifdef GQ_CHAIN_PROF
__device__ __forceinline__ void chain_mark(long long* pr, int step, int k) {
  if (pr != nullptr && threadIdx.x == 0 && step < CHAIN_PROF_STEPS)
    pr[step * 8 + k] = (long long)__builtin_amdgcn_s_memtime();
}
// (the same from lane 0 of the calling wave: the forward's I/O waves)
__device__ __forceinline__ void chain_mark_wave(long long* pr, int step, int k) {
  if (pr != nullptr && (threadIdx.x & 63) == 0 && step < CHAIN_PROF_STEPS)
    pr[step * 8 + k] = (long long)__builtin_amdgcn_s_memtime();
}
// (a clock read now, stored later: a mark's store must not sit in front of a wait that is being measured)
__device__ __forceinline__ long long chain_clock() { return (long long)__builtin_amdgcn_s_memtime(); }
__device__ __forceinline__ void chain_mark_wave_at(long long* pr, int step, int k, long long v) {
  if (pr != nullptr && (threadIdx.x & 63) == 0 && step < CHAIN_PROF_STEPS) pr[step * 8 + k] = v;
}
#else
__device__ __forceinline__ void chain_mark(long long*, int, int) {}
__device__ __forceinline__ void chain_mark_wave(long long*, int, int) {}
__device__ __forceinline__ long long chain_clock() { return 0; }
__device__ __forceinline__ void chain_mark_wave_at(long long*, int, int, long long) {}
#endif

// Tag base of a launch: (epoch mod (2^20 - 1)) + 1 in the high 20 bits of the 32-bit tag, the
// time index (< 4096) in the low 12. Never 0, so a zeroed granule (fresh or reused memory)
// can never pass as a valid one, whatever the epoch counter has wrapped to.
__device__ __forceinline__ unsigned chain_tag_base(unsigned E) { return ((E % 0xFFFFFu) + 1u) << 12; }

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
  // (SRC: L1-bypassing 16-byte buffer loads of the granule stream; byte offsets < 2^32, host-checked)
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned long long*>(SRC ? S.xin : nullptr), (short)0, 0x7fffffff, 0x00020000);
  auto load_x = [&](int r, int tx) {
#pragma unroll
    for (int q = 0; q < (SRC ? PIN : 1); ++q) {
      const size_t tb = xbase + (size_t)(SRC ? PIN * tx + q : tx) * xstep;
#pragma unroll
      for (int j = 0; j < NGL; ++j) {
        if constexpr (SRC) {
#if CHAIN_LD16
          const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)((tb + goff[j]) * 8), 0, 16);
          xq[r][j][q] = u64x2_t{((unsigned long long)v.y << 32) | v.x, ((unsigned long long)v.w << 32) | v.z};
#else
          xq[r][j][q] = u64x2_t{ld_granule(S.xin + tb + goff[j]), ld_granule(S.xin + tb + goff[j] + 1)};
#endif
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

__device__ __forceinline__ void chain_finish(int* ctl, int nblk) {
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(ctl + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == nblk - 1) {            // last workgroup: next launch gets a new epoch
      __hip_atomic_store(ctl + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ctl + 10, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (GCN producers)
      __hip_atomic_fetch_add(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
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

// =====================================================================================
// backward chain: the layers' reverse recurrences, top layer first. Stage k's dx (the
// gradient of the layer below's output, un-pooled by the CONSUMER with the forward's argmax
// bytes when a MaxPooling1D sits between them) is handed off as granules like the forward's
// h; every stage also writes its dz [T+1][Mp][4H] for the weight-gradient pass. The last
// stage writes its dx as plain fp32 (the GCN backward's input).
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
            vv[i] = dxs[buf][row][k];
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

// ---------------------------------------------------------------------------------------
// host
static long long* chain_trace_buf(int dev) {
  static long long* tr[64] = {nullptr};
  // [0, 512): per-workgroup start / end; [512, 768): stage-loop start (backward)
  if (!tr[dev]) TORCH_CHECK(hipMalloc(&tr[dev], 3 * 256 * sizeof(long long)) == hipSuccess,
                            "lstm_chain: trace");
  return tr[dev];
}

// tile 0's per-step phase clocks [CHAIN_MAX stages][CHAIN_PROF_ROWS][8] of the last launch with
// GNNQC_CHAIN_PROF=1 (forward and backward use the same buffer)
static long long* chain_prof_buf(int dev);
// zero the phase-clock buffer before a profiled launch: a stage with fewer than CHAIN_PROF_STEPS
// steps (or fewer marks) than the previous launch's would otherwise leave that launch's rows behind
// (the round-4 table's backward rows 0-1 and m6 columns were such leftovers)
static void chain_prof_clear(int dev) {
  long long* pb = chain_prof_buf(dev);
  if (pb != nullptr)
    TORCH_CHECK(hipMemsetAsync(pb, 0, CHAIN_MAX * CHAIN_PROF_ROWS * 8 * sizeof(long long), stream()) == hipSuccess,
                "chain prof clear");
}
static long long* chain_prof_buf(int dev) {
#ifdef GQ_CHAIN_PROF
  static const bool on = [] {
    const char* e = std::getenv("GNNQC_CHAIN_PROF");
    return e != nullptr && e[0] == '1';
  }();
#else
  const bool on = false;
#endif
  if (!on) return nullptr;
  static long long* pb[64] = {nullptr};
  if (!pb[dev]) {
    TORCH_CHECK(hipMalloc(&pb[dev], CHAIN_MAX * CHAIN_PROF_ROWS * 8 * sizeof(long long)) == hipSuccess, "chain prof");
    TORCH_CHECK(hipMemset(pb[dev], 0, CHAIN_MAX * CHAIN_PROF_ROWS * 8 * sizeof(long long)) == hipSuccess, "chain prof");
  }
  return pb[dev];
}

at::Tensor lstm_chain_prof(const at::Tensor& like) {
  c10::DeviceGuard guard(like.device());
  long long* p = chain_prof_buf(like.get_device());
  TORCH_CHECK(p != nullptr, "lstm_chain_prof: build with GNNQC_CHAIN_PROF_BUILD=1 and set GNNQC_CHAIN_PROF=1 "
                            "before the first chain launch");
  at::Tensor o = at::empty({CHAIN_MAX, CHAIN_PROF_ROWS, 8}, like.options().dtype(at::kLong));
  TORCH_CHECK(hipMemcpyAsync(o.data_ptr<int64_t>(), p, o.numel() * sizeof(long long), hipMemcpyDeviceToDevice,
                             stream()) == hipSuccess, "lstm_chain_prof");
  return o;
}

int* chain_ctl(int dev) {
  static int* ctl[64] = {nullptr};
  TORCH_CHECK(dev >= 0 && dev < 64, "lstm_chain: device index");
  if (!ctl[dev]) {
    hipStreamCaptureStatus cs;
    TORCH_CHECK(hipStreamIsCapturing(stream(), &cs) == hipSuccess && cs == hipStreamCaptureStatusNone,
                "lstm_chain: first use must not be inside a graph capture");
    int* p = nullptr;
    TORCH_CHECK(hipMalloc(&p, 16 * sizeof(int)) == hipSuccess, "lstm_chain: control word allocation");
    const int init[16] = {1, 0};     // epoch 1; [4], [5]: head tickets; [8]: head backward reduce arrivals
    TORCH_CHECK(hipMemcpy(p, init, sizeof(init), hipMemcpyHostToDevice) == hipSuccess, "lstm_chain: init");
    ctl[dev] = p;
  }
  return ctl[dev];
}

// Workgroups of the chain kernels that can be resident at once on this device: the CU count
// of the device (a partitioned MI355X exposes fewer) times the occupancy of the 1024-thread
// chain kernels (with their LDS and VGPR use). Every workgroup of a chain launch must be
// resident, or consumers spin on producers that are never scheduled.
static int chain_capacity(int dev) {
  static int cap[64] = {0};
  TORCH_CHECK(dev >= 0 && dev < 64, "lstm_chain: device index");
  if (cap[dev] == 0) {
    hipDeviceProp_t prop;
    TORCH_CHECK(hipGetDeviceProperties(&prop, dev) == hipSuccess, "lstm_chain: device properties");
    int occ = 1 << 30;
    const void* kernels[] = {reinterpret_cast<const void*>(&lstm_chain_fwd_kernel<true>),
                             reinterpret_cast<const void*>(&lstm_chain_fwd_kernel<false>),
                             reinterpret_cast<const void*>(&lstm_chain_bwd_kernel)};
    for (const void* k : kernels) {
      int n = 0;
      TORCH_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 1024, 0) == hipSuccess,
                  "lstm_chain: occupancy query");
      occ = std::min(occ, n);
    }
    cap[dev] = std::max(0, occ) * prop.multiProcessorCount;
  }
  return cap[dev];
}

int64_t lstm_chain_capacity(const at::Tensor& like) {
  TORCH_CHECK(like.is_cuda(), "lstm_chain_capacity: a GPU tensor names the device");
  return chain_capacity(like.get_device());
}

// The device's chain control words as an int32[16] view (no copy): [epoch, finished workgroups,
// spin-timeout flag, timeouts consumed by the gradient guard, time4/head kernel tickets (2),
// debug spin limit (0: default), a gradient producer saw a non-finite value, head backward
// reduce arrivals, 0...]. The optimiser's update reads and clears the flags inside the captured
// step (a timed-out or non-finite step is skipped, never applied).
at::Tensor lstm_chain_ctl(const at::Tensor& like) {
  TORCH_CHECK(like.is_cuda(), "lstm_chain_ctl: a GPU tensor names the device");
  c10::DeviceGuard guard(like.device());
  int* p = chain_ctl(like.get_device());
  return at::from_blob(p, {16}, like.options().dtype(at::kInt));
}

// x [T, Mp, Din] (Din % 4 == 0, 16-B aligned); per stage W [Dw, 4H], U [H, 4H], b [4H];
// pool[s] > 0: MaxPooling1D(pool[s]) after stage s. Returns per stage [h, g, c, pooled, idx].
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

// time4_head.hip: the forward head arguments (weights, labels, metric accumulators, ticket)
void t4_head_fwd_args(ChainHead& hd, at::TensorList head, const at::Tensor& y, const at::Tensor& mask, int64_t M,
                      int Mp, double alpha1, double alpha2, double w0, double w1, const at::Tensor& sums,
                      const at::Tensor& hist, at::Tensor& logits, at::Tensor& loss, at::Tensor& part);

static std::vector<at::Tensor> chain_fwd_impl(const at::Tensor& x, at::TensorList W, at::TensorList U,
                                              at::TensorList b, at::IntArrayRef pool, bool train, const at::Tensor* pkW,
                                              const at::Tensor* pkU, const T4Host* t4 = nullptr);

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

static std::vector<at::Tensor> chain_fwd_impl(const at::Tensor& x, at::TensorList W, at::TensorList U,
                                              at::TensorList b, at::IntArrayRef pool, bool train, const at::Tensor* pkW,
                                              const at::Tensor* pkU, const T4Host* t4) {
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
    {
      long long* pb = chain_prof_buf(x.get_device());
      S.prof = pb != nullptr ? pb + (size_t)s * CHAIN_PROF_ROWS * 8 : nullptr;
    }
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
  if (train)
    hipLaunchKernelGGL(lstm_chain_fwd_kernel<true>, dim3(nblk), dim3(1024), 0, stream(), A);
  else
    hipLaunchKernelGGL(lstm_chain_fwd_kernel<false>, dim3(nblk), dim3(1024), 0, stream(), A);
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

// Backward of a chain, stages listed TOP layer first. dh: gradient of the top layer's output
// (pooled if pool[0] > 0); per stage the forward's g / c, W, U, the argmax bytes of the pool
// after the layer (empty if none) and pool size; x_width[s]: channels of the layer's input
// layout. Returns [dz_0 .. dz_{n-1}, dx of the bottom layer].
static std::vector<at::Tensor> chain_bwd_setup(ChainBArgs& A, std::vector<at::Tensor>& keep, const at::Tensor& dh,
                                               at::TensorList g, at::TensorList c, at::TensorList W, at::TensorList U,
                                               at::TensorList pidx, at::IntArrayRef pool, at::IntArrayRef x_width,
                                               at::IntArrayRef T_in, int extra_blocks);

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

// time4_head.hip: the backward head arguments (weights, labels, dloss, gradient sinks, tickets)
void t4_head_bwd_args(ChainHead& hd, at::TensorList head, const at::Tensor& y, const at::Tensor& mask, int64_t M,
                      int Mp, double alpha1, double alpha2, double w0, double w1, const at::Tensor& dloss,
                      at::TensorList hgrads, at::Tensor& gpart);

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
    {
      long long* pb = chain_prof_buf(dh.get_device());
      S.prof = pb != nullptr ? pb + (size_t)s * CHAIN_PROF_ROWS * 8 : nullptr;
    }
  }
  dzs.push_back(dx.defined() ? dx.narrow(0, 0, (int)T_in[ns - 1]) : at::empty({0}, opt));
  return dzs;
}

// [epoch, finished, timeout flag, 0] of this device's chain control words (tests)
at::Tensor lstm_chain_status(const at::Tensor& like) {
  c10::DeviceGuard guard(like.device());
  int* p = chain_ctl(like.get_device());
  // [0] epoch, [1] finished workgroups, [2] spin timeout, [3] rejected steps, .., [9] consumer re-polls
  at::Tensor o = at::empty({12}, like.options().dtype(at::kInt));
  TORCH_CHECK(hipMemcpyAsync(o.data_ptr<int>(), p, 12 * sizeof(int), hipMemcpyDeviceToDevice, stream()) == hipSuccess,
              "lstm_chain_status");
  return o;
}

// [blocks, 2] start / end timestamps (s_memrealtime ticks) of the last chain launch (profiling)
at::Tensor lstm_chain_trace(const at::Tensor& like) {
  c10::DeviceGuard guard(like.device());
  long long* p = chain_trace_buf(like.get_device());
  at::Tensor o = at::empty({3 * 256}, like.options().dtype(at::kLong));
  TORCH_CHECK(hipMemcpyAsync(o.data_ptr<int64_t>(), p, o.numel() * sizeof(long long), hipMemcpyDeviceToDevice,
                             stream()) == hipSuccess, "lstm_chain_trace");
  return o;
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("lstm_chain_fwd", &gq::lstm_chain_fwd);
  m.impl("lstm_chain_fwd_pack", &gq::lstm_chain_fwd_pack);
  m.impl("lstm_chain_head_fwd", &gq::lstm_chain_head_fwd);
  m.impl("lstm_chain_status", &gq::lstm_chain_status);
  m.impl("lstm_chain_capacity", &gq::lstm_chain_capacity);
  m.impl("lstm_chain_ctl", &gq::lstm_chain_ctl);
  m.impl("lstm_chain_trace", &gq::lstm_chain_trace);
  m.impl("lstm_chain_prof", &gq::lstm_chain_prof);
  m.impl("lstm_chain_bwd", &gq::lstm_chain_bwd);
  m.impl("lstm_chain_head_bwd", &gq::lstm_chain_head_bwd);
}
