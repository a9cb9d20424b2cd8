// Microbenchmark of the chain kernels' serial LSTM step (H = 16, one 16-sequence tile per
// workgroup, 4 compute waves, one cell per lane): shader cycles per step for variants that add
// the pieces of lstm_chain_fwd.hip's step loop one at a time, to find what sets the ~800-cycle step.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 csrc/bench/chain_step_micro.hip -o build/chain_step_micro
//   build/chain_step_micro            -> one JSON line per variant
//
// Bits of the variant V:
//   1  PRE    gate weights / bias pre-scaled by -log2(e) (-2 log2(e) for g): the MFMA result feeds exp2 directly
//   2  XPRE   x-part of the pre-activation precomputed (no x MFMA, no x LDS tile in the step)
//   4  STORE  compute waves store h (float4 via the fp32 LDS tile), packed gates and c every step
//   8  GRAN   compute waves publish h as 8-byte {value, tag} granules (agent-scope stores)
//   16 XRING  x streamed from global memory through a 6-deep register ring into LDS (stage 0)
//   32 CIN    h MFMA accumulates onto the x part (C operand) instead of a separate add
//   64 IOW    stores / granules / x ring issued by a 5th (I/O) wave instead of the compute waves
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

constexpr int H = 16, TS = 16, KP = 32, D = 6;

template <int V>
__global__ __launch_bounds__(320) void step_kernel(const float* __restrict__ W, const float* __restrict__ U,
                                                   const float* __restrict__ x, float* __restrict__ hout,
                                                   uint2* __restrict__ gout, float* __restrict__ cout,
                                                   unsigned long long* __restrict__ gran, long long* clk, int T,
                                                   int Mp) {
  constexpr bool PRE = V & 1, XPRE = V & 2, STORE = V & 4, GRAN = V & 8, XRING = V & 16, CIN = V & 32,
                 IOW = V & 64;
  __shared__ __bf16 hs[2][16][KP + 8];
  __shared__ __bf16 xs[2][16][KP + 8];
  __shared__ float hf[2][16][H + 4];
  __shared__ uint2 gst[2][256];
  __shared__ float cst[2][256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int tile = blockIdx.x, row0 = tile * 16;
  for (int i = tid; i < 2 * 16 * (KP + 8); i += blockDim.x) {
    (&hs[0][0][0])[i] = (__bf16)0.f;
    (&xs[0][0][0])[i] = (__bf16)0.f;
  }
  const bool compute = w < 4;
  const bool io = IOW ? (w == 4) : compute;
  const int gi = compute ? w : 0;
  const int au = 4 * gi + (col >> 2), ag = col & 3;
  const int unit = 4 * gi + quad;
  const float sc[4] = {PRE ? -1.4426950f : 1.f, PRE ? -1.4426950f : 1.f, PRE ? -2.8853901f : 1.f,
                       PRE ? -1.4426950f : 1.f};
  bf16x8_t ufr, wfr;
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * quad + j;
    ufr[j] = (__bf16)(k < H ? U[k * 64 + ag * H + au] * sc[ag] : 0.f);
    wfr[j] = (__bf16)(k < 20 ? W[k * 64 + ag * H + au] * sc[ag] : 0.f);
  }
  f32x4_t bias = {0.01f * sc[0], 0.02f * sc[1], 0.03f * sc[2], 0.04f * sc[3]};
  // x ring (stage 0 form): the [16][20] tile of step t, 80 float4 granules, lanes 0..79
  const int ioid = IOW ? tid - 256 : tid;
  const int gx = (ioid % 80) * 4;
  float4 xr[D];
  auto load_x = [&](int j, int t) { xr[j] = *reinterpret_cast<const float4*>(x + ((size_t)t * Mp + row0) * 20 + gx); };
  auto stage_x = [&](int buf, int j) {
    const int s = gx / 20, k = gx % 20;
    xs[buf][s][k] = (__bf16)xr[j].x;
    xs[buf][s][k + 1] = (__bf16)xr[j].y;
    xs[buf][s][k + 2] = (__bf16)xr[j].z;
    xs[buf][s][k + 3] = (__bf16)xr[j].w;
  };
  if (XRING && io && ioid < 80) {
    for (int j = 0; j < D; ++j) load_x(j, min(j, T - 1));
  }
  __syncthreads();
  if (XRING && io && ioid < 80) stage_x(0, 0);
  __syncthreads();
  const int gh = (ioid % 64) * 4;     // h store: float4 of the [16][16] tile
  float c = 0.f;
  long long t0 = 0;
  for (int tb = 0; tb < T; tb += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int t = tb + j;
      const int p = t & 1;
      if (t == 1 && tid == 0) t0 = __builtin_amdgcn_s_memtime();
      if (STORE && IOW && io && t >= 1) {      // the I/O wave stores the previous step's gates / c
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const size_t o = (((size_t)(t - 1) * 8 + tile) * 4 + q) * 64 + lane;
          gout[o] = gst[p ^ 1][q * 64 + lane];
          cout[o] = cst[p ^ 1][q * 64 + lane];
        }
      }
      if ((STORE || GRAN) && io && ioid < 64 && t >= 1) {
        const float4 v = *reinterpret_cast<const float4*>(&hf[p ^ 1][gh / H][gh % H]);
        if (STORE) *reinterpret_cast<float4*>(hout + ((size_t)(t - 1) * Mp + row0) * H + gh) = v;
        if (GRAN)
          __hip_atomic_store(gran + ((size_t)(t - 1) * Mp + row0) * H + gh,
                             ((unsigned long long)(t - 1) << 32) | __float_as_uint(v.x), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      }
      float hv = 0.f, iv = 0.f, fv = 0.f, gv = 0.f, ov = 0.f;
      if (compute) {
        f32x4_t accx = bias;
        if (!XPRE) {
          const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(&xs[p][col][8 * quad]);
          accx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr, bx, accx, 0, 0, 0);
        }
        const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(&hs[p][col][8 * quad]);
        f32x4_t acc;
        if (CIN) {
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr, bh, accx, 0, 0, 0);
        } else {
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ufr, bh, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0) + accx;
        }
        if (PRE) {
          iv = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(acc[0]));
          fv = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(acc[1]));
          gv = 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(acc[2])) - 1.f;
          ov = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(acc[3]));
          c = fv * c + iv * gv;
          const float r = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-2.8853901f * c));
          hv = (2.f * ov) * r - ov;
        } else {
          iv = __builtin_amdgcn_rcpf(1.f + __expf(-acc[0]));
          fv = __builtin_amdgcn_rcpf(1.f + __expf(-acc[1]));
          gv = 2.f * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * acc[2])) - 1.f;
          ov = __builtin_amdgcn_rcpf(1.f + __expf(-acc[3]));
          c = fv * c + iv * gv;
          hv = ov * (2.f * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * c)) - 1.f);
        }
        hs[p ^ 1][col][unit] = (__bf16)hv;
        hf[p][col][unit] = hv;
        if (STORE) {
          const size_t o = (((size_t)t * 8 + tile) * 4 + w) * 64 + lane;
          const __bf16 g4[4] = {(__bf16)iv, (__bf16)fv, (__bf16)gv, (__bf16)ov};
          if (IOW) {
            gst[p][tid] = *reinterpret_cast<const uint2*>(g4);
            cst[p][tid] = c;
          } else {
            gout[o] = *reinterpret_cast<const uint2*>(g4);
            cout[o] = c;
          }
        }
      }
      if (XRING && io && ioid < 80) {
        stage_x(p ^ 1, (j + 1) % D);
        load_x((j + 1) % D, min(t + 1 + D, T - 1));
      }
      lds_barrier();
    }
  }
  if (tid == 0) {
    const long long t1 = __builtin_amdgcn_s_memtime();
    clk[blockIdx.x] = t1 - t0;
  }
  if (hout != nullptr && c == 12345.f) hout[0] = c;   // keep the recurrence alive
}

template <int V>
void run(int T, const float* W, const float* U, const float* x, float* h, uint2* g, float* cc,
         unsigned long long* gr, long long* clk) {
  const int Mp = 128, nb = 8;
  std::vector<double> cyc, us;
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  const int threads = (V & 64) ? 320 : 256;
  for (int rep = 0; rep < 30; ++rep) {
    hipEventRecord(a);
    hipLaunchKernelGGL(step_kernel<V>, dim3(nb), dim3(threads), 0, 0, W, U, x, h, g, cc, gr, clk, T, Mp);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    long long hc[8];
    hipMemcpy(hc, clk, sizeof(hc), hipMemcpyDeviceToHost);
    if (rep >= 5) {
      cyc.push_back((double)*std::max_element(hc, hc + nb) / (T - 1));
      us.push_back(ms * 1e3);
    }
  }
  std::sort(cyc.begin(), cyc.end());
  std::sort(us.begin(), us.end());
  printf("{\"variant\": %d, \"pre\": %d, \"xpre\": %d, \"store\": %d, \"gran\": %d, \"xring\": %d, \"cin\": %d, "
         "\"iow\": %d, \"cycles_per_step\": %.1f, \"launch_us\": %.2f}\n",
         V, !!(V & 1), !!(V & 2), !!(V & 4), !!(V & 8), !!(V & 16), !!(V & 32), !!(V & 64), cyc[cyc.size() / 2],
         us[us.size() / 2]);
  fflush(stdout);
}

int main() {
  static_assert(180 % D == 0, "T must be a multiple of D");
  const int T = 180, Mp = 128;   // a multiple of the ring depth D: every step index < T
  float *W, *U, *x, *h, *cc;
  uint2* g;
  unsigned long long* gr;
  long long* clk;
  hipMalloc(&W, 20 * 64 * 4);
  hipMalloc(&U, 16 * 64 * 4);
  hipMalloc(&x, (size_t)T * Mp * 20 * 4);
  hipMalloc(&h, (size_t)(T + 8) * Mp * H * 4);
  hipMalloc(&g, (size_t)(T + 8) * 8 * 4 * 64 * 8);
  hipMalloc(&cc, (size_t)(T + 8) * 8 * 4 * 64 * 4);
  hipMalloc(&gr, (size_t)(T + 8) * Mp * H * 8);
  hipMalloc(&clk, 64 * 8);
  std::vector<float> hw(20 * 64), hu(16 * 64), hx((size_t)T * Mp * 20);
  for (size_t i = 0; i < hw.size(); ++i) hw[i] = 0.3f * (float)((i * 37) % 17) / 17.f - 0.15f;
  for (size_t i = 0; i < hu.size(); ++i) hu[i] = 0.3f * (float)((i * 53) % 19) / 19.f - 0.15f;
  for (size_t i = 0; i < hx.size(); ++i) hx[i] = (float)((i * 29) % 23) / 23.f - 0.5f;
  hipMemcpy(W, hw.data(), hw.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(U, hu.data(), hu.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice);
  run<0>(T, W, U, x, h, g, cc, gr, clk);
  run<1>(T, W, U, x, h, g, cc, gr, clk);
  run<2>(T, W, U, x, h, g, cc, gr, clk);
  run<3>(T, W, U, x, h, g, cc, gr, clk);
  run<35>(T, W, U, x, h, g, cc, gr, clk);
  run<16>(T, W, U, x, h, g, cc, gr, clk);
  run<4 + 16>(T, W, U, x, h, g, cc, gr, clk);
  run<4 + 8 + 16>(T, W, U, x, h, g, cc, gr, clk);
  run<1 + 4 + 8 + 16 + 32>(T, W, U, x, h, g, cc, gr, clk);
  run<1 + 4 + 8 + 16 + 32 + 64>(T, W, U, x, h, g, cc, gr, clk);
  run<1 + 2 + 4 + 8 + 32 + 64>(T, W, U, x, h, g, cc, gr, clk);
  run<1 + 2 + 4 + 8 + 32>(T, W, U, x, h, g, cc, gr, clk);
  return 0;
}
