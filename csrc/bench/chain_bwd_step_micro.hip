// Microbenchmark of the chain backward's serial H = 16 reverse step (lstm_chain_bwd.hip, chain_bwd_stage16
// <1, D, SRC, UP, XO>: one 16-sequence tile per workgroup, 4 compute waves with one cell per lane, 4 publisher
// waves, the dx wave, the dz wave): shader cycles per step for variants that remove or move one piece of the
// step at a time. One workgroup per tile, no waits between workgroups: the host writes the saved state, the
// arg-max bytes and a dh granule stream whose tags are all valid, so chain_wait is compiled in but never taken.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -Wno-unused-value csrc/bench/chain_bwd_step_micro.hip -o chain_bwd_step_micro
//   ./chain_bwd_step_micro            -> one JSON line per variant
//
// Bits of the variant V:
//   1   NOSTATE  no state loads in the step loop (the ring keeps the prologue's gates and c)
//   2   NOPRE    no cell_pre in the step loop (the six factors keep step 0's values)
//   4   NOSTAGE  no dh ring, no tag check, no un-pool select, no dh store (dhs keeps zeros)
//   8   NOAUX    no publisher, dx and dz waves (256 threads: nothing leaves the workgroup)
//   16  PREP     four prep waves keep both rings: they stage dh of step s + 2 and write the six factors of step
//                s + 2 into a double-buffered LDS image; the compute waves read dz, dh and the factors, run the
//                two MFMAs and cell_tail, and issue no global memory instruction
//   32  R        both K-block reads of dz ahead of the first MFMA
//   64  ACC      one accumulating MFMA pair instead of two independent ones (changes the rounding: timing only)
//   128 CPRIO    s_setprio 3 on the compute waves
//   256 NOPUB    the publisher waves join the barriers and store nothing
//   512 NODX     the dx wave joins the barriers and computes nothing
//   1024 NODZ    the dz wave joins the barriers and stores nothing
//   2048 PUBFIX  the publisher's wave index is a scalar and its LDS offsets are computed once: no division by
//                Din and no lane-masked branch in the step (the form lstm_chain_bwd.hip has since this file's
//                first figures, profiles/chain_bwd_step_micro.txt; without the bit: the publisher before it)
// DP: ring depth (reverse steps of prefetch) of the waves that keep the rings.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ float tanhf_fast(float x) {
  return 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)) - 1.0f;
}
__device__ __forceinline__ float4 gates_unpack(uint2 u) {
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ unsigned long long ld_granule(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_granule(unsigned long long* p, float v, unsigned tag) {
  __hip_atomic_store(p, ((unsigned long long)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
// the project's slow path (lstm_chain_common.h), bounded; never taken here
__device__ __noinline__ unsigned long long chain_wait(const unsigned long long* p, unsigned want, int* ctl) {
  unsigned long long v = 0;
  const bool l0 = (threadIdx.x & 63) == 0;
  for (int it = 0; it < (1 << 12); ++it) {
    unsigned t0 = want;
    if (l0) t0 = (unsigned)(ld_granule(p) >> 32);
    if ((unsigned)__builtin_amdgcn_readfirstlane((int)t0) == want) {
      v = ld_granule(p);
      if (__builtin_amdgcn_ballot_w64((unsigned)(v >> 32) != want) == 0) return v;
    }
    __builtin_amdgcn_s_sleep(0);
  }
  __hip_atomic_store(ctl + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return v;
}

constexpr int H = 16, G4 = 64, KB = 2, HP = H + 4, NW = 4, NT = 256, ZPAD = 16, XPAD = 1, KX = 1, NXB = 2;
constexpr int NPUB = 4, D = 4, PUBPRIO = 2, DXPRIO = 2, LEAD = 1;

struct Args {
  const unsigned long long* din;     // [Ts][Mp][H] granules, tag = tagb | source step
  const unsigned char* pidx;         // [Ts][Mp][H] arg-max bytes
  const __bf16* g;                   // [T + 1][ntiles][NW][64][4]
  const float* c;
  const float* W;
  const float* U;
  __bf16* dz;                        // [T + 1][Mp][G4]
  unsigned long long* sout;          // [T + 1][Mp][Din]
  long long* clk;
  int* ctl;
  int T, Din, Dw, P, Ts, Mp, ntiles;
  unsigned tagb;
};

// Workgroup barriers of one role for a sequence of T steps (the two of the prologue, one per step of the
// loop rounded up to the compute waves' unroll D, the closing one): every role runs exactly this many
__host__ __device__ constexpr int step_barriers(int T) { return (T + D - 1) / D * D; }

template <int V, int DP>
__global__ __launch_bounds__(1024) void bwd_step_kernel(const Args S) {
  constexpr bool NOSTATE = V & 1, NOPRE = V & 2, NOSTAGE = V & 4, AUX = !(V & 8), PREP = V & 16, RD2 = V & 32,
                 ACC = V & 64, CPRIO = V & 128, NOPUB = V & 256, NODX = V & 512, NODZ = V & 1024, PUBFIX = V & 2048;
  constexpr int RD = DP;                               // ring depth of the waves that keep the rings
  constexpr int PREP0 = AUX ? NT + 64 * NPUB + 128 : NT;
  static_assert(RD >= 4, "the prologue fills steps 0 .. 2 of the ring");
  __shared__ __attribute__((aligned(16))) __bf16 zs[2][16][G4 + ZPAD];
  __shared__ __attribute__((aligned(16))) float dhs[2][16][HP];
  __shared__ __attribute__((aligned(16))) float dxs[2][16][32 * KX + XPAD];
  __shared__ __attribute__((aligned(16))) float4 facA[2][NT];   // fo, ff, z0, z1 of the lane's cell
  __shared__ __attribute__((aligned(16))) float2 facB[2][NT];   // z2, z3

  const int T = S.T, Din = S.Din, Dw = S.Dw, P = S.P, Ts = S.Ts, Mp = S.Mp, ntiles = S.ntiles;
  const unsigned tagb = S.tagb;
  int* ctl = S.ctl;
  const int tid = threadIdx.x, lane = tid & 63;
  const int tile = blockIdx.x, row0 = tile * 16;
  const int nsteps = step_barriers(T);
  if (AUX && tid >= NT + 64 * NPUB + 64 && tid < NT + 64 * NPUB + 128) {   // dz wave
    if (PUBPRIO > 0) __builtin_amdgcn_s_setprio(PUBPRIO);
    __syncthreads();
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      lds_barrier();
      if (!NODZ && s < T) {
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
  if (AUX && tid >= NT + 64 * NPUB && tid < NT + 64 * NPUB + 64) {         // dx wave
    if (DXPRIO > 0) __builtin_amdgcn_s_setprio(DXPRIO);
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
    __syncthreads();
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      lds_barrier();
      if (!NODX && s < T) {
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
      }
    }
    __syncthreads();
    return;
  }
  if (AUX && tid >= NT && tid < NT + 64 * NPUB) {                          // publisher waves
    if (PUBPRIO > 0) __builtin_amdgcn_s_setprio(PUBPRIO);
    const int nx = 16 * Din;
    const size_t xstep = (size_t)Mp * Din;
    const int pj = (tid - NT) >> 6;
    constexpr int ESTR = 64 * NPUB;
    const int dq = ESTR / Din, dr = ESTR % Din;
    constexpr int PUBN = 4;
    auto publish = [&](int buf, int ts) {
      const unsigned tag = tagb | (unsigned)ts;
      for (int e0 = 64 * pj; e0 < nx; e0 += ESTR * PUBN) {
        const int niter = min((nx - e0 + ESTR - 1) / ESTR, PUBN);
        float vv[PUBN];
        int row = (lane + e0) / Din, k = (lane + e0) % Din;
#pragma unroll
        for (int i = 0; i < PUBN; ++i) {
          if (i < niter) vv[i] = dxs[buf][row][k];
          row += dq;
          k += dr;
          if (k >= Din) { k -= Din; ++row; }
        }
#pragma unroll
        for (int i = 0; i < PUBN; ++i) {
          if (i < niter) {
            const int e = e0 + lane + ESTR * i;
            st_granule(S.sout + (size_t)row0 * Din + e + (size_t)ts * xstep, vv[i], tag);
          }
        }
      }
    };
    // PUBFIX: the lane's elements 64 pj + lane + ESTR i of a dx tile, i < nfix (wave-uniform: 16 Din is a
    // multiple of 64), at fixed offsets of a dxs buffer
    static_assert(ESTR * PUBN >= 16 * 64, "one batch covers the widest dx tile (Din <= 64)");
    const int pjs = __builtin_amdgcn_readfirstlane(pj);
    const int nfix = min(max((nx - 64 * pjs + ESTR - 1) / ESTR, 0), PUBN);
    int lofs[PUBN];
    {
      int row = (lane + 64 * pjs) / Din, k = (lane + 64 * pjs) % Din;
#pragma unroll
      for (int i = 0; i < PUBN; ++i) {
        lofs[i] = row * (32 * KX + XPAD) + k;
        row += dq;
        k += dr;
        if (k >= Din) { k -= Din; ++row; }
      }
    }
    unsigned long long* const so = S.sout + (size_t)row0 * Din + 64 * pjs + lane;
    auto publish_fix = [&](int buf, int ts) {
      const unsigned tag = tagb | (unsigned)ts;
      const float* b = &dxs[buf][0][0];
      unsigned long long* o = so + (size_t)ts * xstep;
      float vv[PUBN];
#pragma unroll
      for (int i = 0; i < PUBN; ++i)
        if (i < nfix) vv[i] = b[lofs[i]];
#pragma unroll
      for (int i = 0; i < PUBN; ++i)
        if (i < nfix) st_granule(o + ESTR * i, vv[i], tag);
    };
    __syncthreads();
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      lds_barrier();
      if (!NOPUB && s >= 1 && s <= T) {
        if (PUBFIX) publish_fix((s - 1) & 1, T - s);
        else publish((s - 1) & 1, T - s);
      }
    }
    __syncthreads();
    if (!NOPUB) {
      if (PUBFIX) publish_fix((T - 1) & 1, 0);
      else publish((T - 1) & 1, 0);
    }
    return;
  }

  // compute waves (tid < NT) and, PREP, the prep waves: ct is the thread's index within its role
  const bool prep = PREP && tid >= PREP0;
  const int ct = prep ? tid - PREP0 : tid;
  const bool rings = PREP ? prep : true;                 // this wave keeps the state ring and the dh ring
  const int w = __builtin_amdgcn_readfirstlane(ct >> 6);
  const int col = lane & 15, quad = lane >> 4;
  const int unit = 4 * w + quad;

  if (rings)
    for (int i = ct; i < 2 * 16 * HP; i += NT) (&dhs[0][0][0])[i] = 0.f;

  bf16x8_t ufr[KB];
  if (!prep) {
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

  uint2 rg[RD];
  float rc[RD];
  unsigned long long rq[RD];
  unsigned ri[RD];
  const unsigned pmag = P > 1 ? 0xFFFFFFFFu / (unsigned)P + 1u : 0u;
  auto divp = [&](int tt) { return P > 1 ? (int)__umulhi((unsigned)tt, pmag) : tt; };
  auto src_t = [&](int tt) { return tt < Ts * P ? divp(tt) : -1; };
  const size_t eoff = (size_t)row0 * H + ct;
  const size_t hstep = (size_t)Mp * H;
  if (rings) {
    int tw = T - 1 - (D + LEAD);
    tw = max(tw, 0);
    const int st = src_t(tw);
    if (st >= 0) (void)chain_wait(S.din + eoff + (size_t)st * hstep, tagb | (unsigned)st, ctl);
  }
  constexpr unsigned NOSRC = 0xFFFFFFFFu;
  const unsigned lo8 = (unsigned)((tile * NW + w) * 64 + lane) * 8u;
  const unsigned gstr = (unsigned)(ntiles * NW * 64 * 8);
  const char* gbase = reinterpret_cast<const char*>(S.g);
  const char* cbase = reinterpret_cast<const char*>(S.c);
  int stt = T - 1;
  auto state_load = [&](int J) {
    const unsigned o = (unsigned)__builtin_amdgcn_readfirstlane(stt) * gstr + lo8;
    rg[J] = *reinterpret_cast<const uint2*>(gbase + o);
    rc[J] = *reinterpret_cast<const float*>(cbase + (o >> 1));
    stt = max(stt - 1, 0);
  };
  const unsigned eo = (unsigned)eoff;
  const unsigned hrow = (unsigned)hstep;
  const char* dbase = reinterpret_cast<const char*>(S.din);
  const char* pbase = reinterpret_cast<const char*>(S.pidx);
  int dtt = T - 1;
  int dst = min(divp(dtt), Ts - 1);
  int dph = dtt - dst * P;
  const unsigned dlim = (unsigned)(Ts * P);
  unsigned rinf[RD];
  auto ring_load = [&](int J) {
    const unsigned o = (unsigned)max(dst, 0) * hrow + eo;
    rq[J] = ld_granule(reinterpret_cast<const unsigned long long*>(dbase + o * 8u));
    ri[J] = (unsigned)*reinterpret_cast<const unsigned char*>(pbase + o);
    const unsigned inf = ((unsigned)dph << 12) | (unsigned)dst;
    rinf[J] = (unsigned)dtt < dlim ? inf : NOSRC;
    --dtt;
    const bool wrap = dph == 0;
    dst = wrap ? dst - 1 : dst;
    dph = wrap ? P - 1 : dph - 1;
  };
  auto stage = [&](int J) -> float {
    const unsigned inf = rinf[J];
    const bool has = inf != NOSRC;
    const unsigned want = tagb | (inf & 0xfffu);
    const bool bad = has && (unsigned)(rq[J] >> 32) != want;
    if (__builtin_amdgcn_ballot_w64(bad) != 0) {
      rq[J] = chain_wait(S.din + eoff + (size_t)(inf & 0xfffu) * hstep, want, ctl);
    }
    const float v = __uint_as_float((unsigned)rq[J]);
    const bool keep = has && ri[J] == (inf >> 12);
    return keep ? v : 0.f;
  };
  float tc, fo, ff, z0, z1, z2, z3;
  auto cell_pre_c = [&](int J) { tc = tanhf_fast(rc[J]); };
  auto cell_pre = [&](int J, int JN, int tt) {
    const float cp = rc[JN] * (tt > 0 ? 1.f : 0.f);
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
  auto put_factors = [&](int b) {
    facA[b][ct] = make_float4(fo, ff, z0, z1);
    facB[b][ct] = make_float2(z2, z3);
  };
  auto get_factors = [&](int b) {
    const float4 a = facA[b][ct];
    const float2 c2 = facB[b][ct];
    fo = a.x; ff = a.y; z0 = a.z; z1 = a.w; z2 = c2.x; z3 = c2.y;
  };

  if (prep) {
    // prep waves: dh of steps 0 and 1 and the factors of steps 0 and 1 in the prologue; after barrier s dh of
    // step s + 2 -> dhs[s & 1] and the factors of step s + 2 -> fac[s & 1] (both last read after barrier s - 1)
#pragma unroll
    for (int j = 0; j < RD; ++j) {
      state_load(j);
      ring_load(j);
    }
    __syncthreads();
    dhs[0][ct / H][ct % H] = stage(0);
    ring_load(0);
    dhs[1][ct / H][ct % H] = stage(1);
    ring_load(1);
    cell_pre_c(0);
    cell_pre(0, 1, T - 1);
    put_factors(0);
    state_load(0);
    cell_pre_c(1);
    cell_pre(1, 2, T - 2);
    put_factors(1);
    state_load(1);
    __syncthreads();
    for (int s0 = 0; s0 < nsteps; s0 += RD) {
#pragma unroll
      for (int j = 0; j < RD; ++j) {
        const int s = s0 + j;
        if (s >= nsteps) break;                        // (wave-uniform: RD need not divide the step count)
        const int p = s & 1;
        const int j2 = (j + 2) % RD, j3 = (j + 3) % RD;
        lds_barrier();
        if (!NOSTAGE) {
          dhs[p][ct / H][ct % H] = stage(j2);
          ring_load(j2);
        }
        if (!NOPRE) {
          cell_pre_c(j2);
          cell_pre(j2, j3, T - 3 - s);
          put_factors(p);
        }
        if (!NOSTATE) state_load(j2);
      }
    }
    __syncthreads();
    return;
  }

  if (CPRIO) __builtin_amdgcn_s_setprio(3);
  if (!PREP) {
#pragma unroll
    for (int j = 0; j < RD; ++j) {
      state_load(j);
      ring_load(j);
    }
  }
  __syncthreads();
  if (!PREP) {
    dhs[0][tid / H][tid % H] = stage(0);
    ring_load(0);
    dhs[1][tid / H][tid % H] = stage(1);
    ring_load(1);
  }
  __syncthreads();
  float dhn = dhs[0][col][unit];
  if (PREP) {
    get_factors(0);
  } else {
    cell_pre_c(0);
    cell_pre(0, 1, T - 1);
  }
  cell_tail(0, dhn);
  if (!PREP) state_load(0);

  long long t0 = 0;
  for (int s0 = 0; s0 < nsteps; s0 += RD) {
    if (s0 == RD && tid == 0) t0 = __builtin_amdgcn_s_memtime();
#pragma unroll
    for (int j = 0; j < RD; ++j) {
      const int s = s0 + j;
      if (s >= nsteps) break;
      const int p = s & 1;
      const int j1 = (j + 1) % RD, j2 = (j + 2) % RD;
      lds_barrier();
      const bf16x8_t bz0 = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][8 * quad]);
      bf16x8_t bz1;
      if (RD2) bz1 = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][32 + 8 * quad]);
      __builtin_amdgcn_sched_barrier(0);
      f32x4_t a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[0], bz0, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (!RD2) bz1 = *reinterpret_cast<const bf16x8_t*>(&zs[p][col][32 + 8 * quad]);
      dhn = dhs[p ^ 1][col][unit];
      if (PREP) {
        get_factors(p ^ 1);
      } else if (!NOSTAGE) {
        dhs[p][tid / H][tid % H] = stage(j2);
        ring_load(j2);
      }
      __builtin_amdgcn_sched_barrier(0);
      const f32x4_t a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr[1], bz1, ACC ? a0 : f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (!PREP && !NOPRE) {
        cell_pre_c(j1);
        cell_pre(j1, j2, T - 2 - s);
      }
      __builtin_amdgcn_sched_barrier(0);
      const float dhr = ACC ? a1[0] : a0[0] + a1[0];
      cell_tail(p ^ 1, dhn + dhr);
      if (!PREP && !NOSTATE) state_load(j1);
    }
  }
  if (tid == 0) S.clk[blockIdx.x] = (long long)__builtin_amdgcn_s_memtime() - t0;
  __syncthreads();
  if (dc == 12345.f) S.clk[8] = 1;   // keep the recurrence alive without the dz wave
}

static std::vector<unsigned short> g_ref_dz;   // dz and the dx granules of the full step (variant 0): the forms that keep
static std::vector<unsigned long long> g_ref_so;   // the arithmetic are compared with them

template <int V, int DP>
void run(const Args& A, size_t dz_elems) {
  const int nb = A.ntiles;
  const int nsteps = step_barriers(A.T);
  std::vector<double> cyc, us;
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  const int threads = 256 + ((V & 8) ? 0 : 64 * NPUB + 128) + ((V & 16) ? 256 : 0);
  hipMemset(A.dz, 0, dz_elems * 2);
  hipMemset(A.sout, 0, (size_t)(A.T + 1) * A.Mp * A.Din * 8);
  for (int rep = 0; rep < 30; ++rep) {
    hipEventRecord(a);
    hipLaunchKernelGGL((bwd_step_kernel<V, DP>), dim3(nb), dim3(threads), 0, 0, A);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    long long hc[8];
    hipMemcpy(hc, A.clk, sizeof(hc), hipMemcpyDeviceToHost);
    if (rep >= 5) {
      cyc.push_back((double)*std::max_element(hc, hc + nb) / (nsteps - DP));
      us.push_back(ms * 1e3);
    }
  }
  std::sort(cyc.begin(), cyc.end());
  std::sort(us.begin(), us.end());
  int flag[4] = {0, 0, 0, 0};
  hipMemcpy(flag, A.ctl, sizeof(flag), hipMemcpyDeviceToHost);
  const char* same = "n/a";
  const bool writes_dz = !(V & (8 | 1024)), same_math = !(V & (1 | 2 | 4 | 64));
  if (writes_dz && same_math) {
    std::vector<unsigned short> dz(dz_elems);
    hipMemcpy(dz.data(), A.dz, dz_elems * 2, hipMemcpyDeviceToHost);
    if (V == 0 && DP == D && g_ref_dz.empty()) g_ref_dz = dz;
    same = (!g_ref_dz.empty() && std::memcmp(dz.data(), g_ref_dz.data(), dz_elems * 2) == 0) ? "true" : "false";
  }
  const char* same_so = "n/a";
  if (writes_dz && same_math && !(V & (256 | 512))) {
    const size_t n = (size_t)(A.T + 1) * A.Mp * A.Din;
    std::vector<unsigned long long> so(n);
    hipMemcpy(so.data(), A.sout, n * 8, hipMemcpyDeviceToHost);
    if (V == 0 && DP == D && g_ref_so.empty()) g_ref_so = so;
    same_so = (!g_ref_so.empty() && std::memcmp(so.data(), g_ref_so.data(), n * 8) == 0) ? "true" : "false";
  }
  printf("{\"variant\": %d, \"ring\": %d, \"nostate\": %d, \"nopre\": %d, \"nostage\": %d, \"noaux\": %d, \"prep\": %d, "
         "\"reads_first\": %d, \"acc_pair\": %d, \"cprio\": %d, \"nopub\": %d, \"nodx\": %d, \"nodz\": %d, \"pubfix\": %d, \"threads\": %d, \"cycles_per_step\": %.1f, "
         "\"cycles_min\": %.1f, \"cycles_max\": %.1f, \"launch_us\": %.2f, \"timeout_flag\": %d, \"dz_equals_full\": \"%s\", \"dx_equals_full\": \"%s\"}\n",
         V, DP, !!(V & 1), !!(V & 2), !!(V & 4), !!(V & 8), !!(V & 16), !!(V & 32), !!(V & 64), !!(V & 128), !!(V & 256), !!(V & 512), !!(V & 1024), !!(V & 2048), threads,
         cyc[cyc.size() / 2], cyc.front(), cyc.back(), us[us.size() / 2], flag[2], same, same_so);
  fflush(stdout);
}

int main() {
  const int T = 181, P = 3, Ts = T / P, Mp = 128, ntiles = Mp / 16, Din = 16, Dw = 16;
  const unsigned tagb = 7u << 12;
  const size_t n_state = (size_t)(T + 1) * ntiles * NW * 64;
  const size_t n_src = (size_t)Ts * Mp * H;
  const size_t dz_elems = (size_t)(T + 1) * Mp * G4;
  std::vector<unsigned short> hg(n_state * 4);
  std::vector<float> hc(n_state), hw((size_t)Dw * G4), hu((size_t)H * G4);
  std::vector<unsigned long long> hd(n_src);
  std::vector<unsigned char> hp(n_src);
  auto bf = [](float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  };
  for (size_t i = 0; i < n_state; ++i) {
    hg[4 * i + 0] = bf(0.15f + 0.7f * (float)((i * 37) % 101) / 101.f);
    hg[4 * i + 1] = bf(0.15f + 0.7f * (float)((i * 53) % 103) / 103.f);
    hg[4 * i + 2] = bf(-0.8f + 1.6f * (float)((i * 29) % 107) / 107.f);
    hg[4 * i + 3] = bf(0.15f + 0.7f * (float)((i * 41) % 109) / 109.f);
    hc[i] = -1.f + 2.f * (float)((i * 31) % 113) / 113.f;
  }
  for (size_t i = 0; i < hw.size(); ++i) hw[i] = 0.3f * (float)((i * 37) % 17) / 17.f - 0.15f;
  for (size_t i = 0; i < hu.size(); ++i) hu[i] = 0.3f * (float)((i * 53) % 19) / 19.f - 0.15f;
  for (size_t i = 0; i < n_src; ++i) {
    const float v = 0.2f * (float)((i * 43) % 127) / 127.f - 0.1f;
    unsigned u;
    std::memcpy(&u, &v, 4);
    const unsigned st = (unsigned)(i / ((size_t)Mp * H));
    hd[i] = ((unsigned long long)(tagb | st) << 32) | u;
    hp[i] = (unsigned char)((i * 7) % P);
  }
  Args A{};
  void *din, *pidx, *g, *c, *W, *U, *dz, *sout, *clk, *ctl;
  hipMalloc(&din, n_src * 8);
  hipMalloc(&pidx, n_src);
  hipMalloc(&g, n_state * 8);
  hipMalloc(&c, n_state * 4);
  hipMalloc(&W, hw.size() * 4);
  hipMalloc(&U, hu.size() * 4);
  hipMalloc(&dz, dz_elems * 2);
  hipMalloc(&sout, (size_t)(T + 1) * Mp * Din * 8);
  hipMalloc(&clk, 64 * 8);
  hipMalloc(&ctl, 64 * 4);
  hipMemset(ctl, 0, 64 * 4);
  hipMemset(clk, 0, 64 * 8);
  hipMemcpy(din, hd.data(), n_src * 8, hipMemcpyHostToDevice);
  hipMemcpy(pidx, hp.data(), n_src, hipMemcpyHostToDevice);
  hipMemcpy(g, hg.data(), n_state * 8, hipMemcpyHostToDevice);
  hipMemcpy(c, hc.data(), n_state * 4, hipMemcpyHostToDevice);
  hipMemcpy(W, hw.data(), hw.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(U, hu.data(), hu.size() * 4, hipMemcpyHostToDevice);
  A.din = (const unsigned long long*)din;
  A.pidx = (const unsigned char*)pidx;
  A.g = (const __bf16*)g;
  A.c = (const float*)c;
  A.W = (const float*)W;
  A.U = (const float*)U;
  A.dz = (__bf16*)dz;
  A.sout = (unsigned long long*)sout;
  A.clk = (long long*)clk;
  A.ctl = (int*)ctl;
  A.T = T; A.Din = Din; A.Dw = Dw; A.P = P; A.Ts = Ts; A.Mp = Mp; A.ntiles = ntiles;
  A.tagb = tagb;
  run<0, 4>(A, dz_elems);                  // the step as it is
  run<1, 4>(A, dz_elems);
  run<2, 4>(A, dz_elems);
  run<4, 4>(A, dz_elems);
  run<1 + 2, 4>(A, dz_elems);
  run<1 + 2 + 4, 4>(A, dz_elems);          // the dependent chain with the publisher, dx and dz waves
  run<8, 4>(A, dz_elems);
  run<1 + 2 + 4 + 8, 4>(A, dz_elems);      // the dependent chain alone
  run<16, 4>(A, dz_elems);                 // PREP
  run<16, 6>(A, dz_elems);
  run<16, 8>(A, dz_elems);
  run<16 + 8, 4>(A, dz_elems);
  run<16 + 32, 4>(A, dz_elems);
  run<16 + 64, 4>(A, dz_elems);
  run<16 + 128, 4>(A, dz_elems);
  run<16 + 32 + 128, 4>(A, dz_elems);
  run<32, 4>(A, dz_elems);
  run<256, 4>(A, dz_elems);                // one of the publisher, dx and dz waves idle at a time, then two
  run<512, 4>(A, dz_elems);
  run<1024, 4>(A, dz_elems);
  run<256 + 512, 4>(A, dz_elems);
  run<256 + 1024, 4>(A, dz_elems);
  run<512 + 1024, 4>(A, dz_elems);
  run<256 + 512 + 1024, 4>(A, dz_elems);   // all three idle: what ten waves at the barrier cost
  run<7 + 256, 4>(A, dz_elems);            // the same under the bare dependent chain
  run<7 + 512, 4>(A, dz_elems);
  run<7 + 1024, 4>(A, dz_elems);
  run<16 + 256, 4>(A, dz_elems);           // PREP with one of them idle
  run<16 + 512, 4>(A, dz_elems);
  run<16 + 1024, 4>(A, dz_elems);
  run<16 + 256 + 512 + 1024, 4>(A, dz_elems);
  run<2048, 4>(A, dz_elems);               // the publisher's step without its division and masked branches
  run<2048 + 7, 4>(A, dz_elems);
  run<2048 + 16, 4>(A, dz_elems);          // ... and PREP on top of it
  run<2048 + 16, 6>(A, dz_elems);
  run<2048 + 16 + 32, 4>(A, dz_elems);
  run<2048 + 16 + 128, 4>(A, dz_elems);
  run<0, 4>(A, dz_elems);                  // (the full step again: drift across the run)
  return 0;
}
