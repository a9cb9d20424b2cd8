// What the LSTM chain's two directions (lstm_chain_fwd.hip, lstm_chain_bwd.hip) share: the granule hand-off,
// its waits, the launch epoch, the phase clocks, and the host helpers of lstm_chain_ctl.hip.
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
#pragma once
#include "common.h"

#include <cstdlib>
#include <type_traits>

namespace gq {

typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

static constexpr int CHAIN_MAX = 8;
static constexpr int CHAIN_SPIN = 1 << 20;
// (the wait knobs are both directions': a variant of one rebuilds lstm_chain_fwd.hip and lstm_chain_bwd.hip)
#ifndef CHAIN_W_SLEEP
#define CHAIN_W_SLEEP 0      // chain_wait back-off: s_sleep argument (x 64 clocks) per nap unit (8 / 8: 0.284 ms/step,
#endif
#ifndef CHAIN_W_NAPMAX
#define CHAIN_W_NAPMAX 1     //   2 / 4: 0.278, 0 / 1: 0.275-0.277: lane 0's load latency paces the poll) and the largest nap
#endif

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
__device__ __noinline__ unsigned long long chain_wait(const unsigned long long* p, unsigned want, int* ctl) {
  return chain_wait_body<false>(p, want, ctl);
}
// inlined form for the forward I/O waves: a call in their step loop made the compiler drain vmcnt
// at the tag checks (the whole x ring waited for each step)
__device__ __forceinline__ unsigned long long chain_wait_inl(const unsigned long long* p, unsigned want, int* ctl) {
  return chain_wait_body<true>(p, want, ctl);
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

// ---- host: lstm_chain_ctl.hip (chain_ctl itself is declared in common.h)
long long* chain_trace_buf(int dev);
long long* chain_prof_buf(int dev);
void chain_prof_clear(int dev);
long long* chain_prof_rows(int dev, int stage);
int chain_capacity(int dev);
// resident 1024-thread workgroups of kernel k per CU; the least over each direction's kernels (its own file)
inline int chain_occupancy(const void* k) {
  int n = 0;
  TORCH_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 1024, 0) == hipSuccess, "lstm_chain: occupancy query");
  return n;
}
int chain_fwd_occupancy(), chain_bwd_occupancy();

}  // namespace gq
