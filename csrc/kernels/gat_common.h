// Device helpers and the instance table shared by the fused GATConv kernels: gat.hip (node pooling,
// N <= 64) and gat_node.hip (one LSTM sequence per node, N <= 256).
#pragma once
#include "common.h"

namespace gq {

at::Tensor colsum(const at::Tensor& partial);     // gcn.hip

constexpr float GAT_SLOPE = 0.2f;        // leaky_relu slope of the attention scores
enum { GAT_ACT_LINEAR = 0, GAT_ACT_PRELU = 1, GAT_ACT_RELU = 2 };

typedef unsigned long long gat_bits_t;

// Parameters in LDS (wave-uniform broadcast reads): W [Cin][H][C], bias [H*C], alpha [H*C],
// u_s [Cin][H], u_n [Cin][H]
template <int CIN, int C, int H>
struct GatParams {
  static constexpr int HC = H * C, NW = CIN * HC;
  static constexpr int SIZE = NW + 2 * HC + 2 * CIN * H;
  float* p;
  __device__ float W(int f, int h, int c) const { return p[(f * H + h) * C + c]; }
  __device__ float bias(int k) const { return p[NW + k]; }
  __device__ float alpha(int k) const { return p[NW + HC + k]; }
  __device__ float us(int f, int h) const { return p[NW + 2 * HC + f * H + h]; }
  __device__ float un(int f, int h) const { return p[NW + 2 * HC + CIN * H + f * H + h]; }
  __device__ void load(const float* __restrict__ Wg, const float* __restrict__ as, const float* __restrict__ an,
                       const float* __restrict__ bg, const float* __restrict__ alg) {
    const int tid = threadIdx.x;
    for (int i = tid; i < NW; i += blockDim.x) p[i] = Wg[i];
    for (int i = tid; i < HC; i += blockDim.x) {
      p[NW + i] = bg[i];
      p[NW + HC + i] = alg != nullptr ? alg[i] : 0.f;
    }
    if (tid < CIN * H) {
      const int f = tid / H, h = tid % H;
      float s = 0.f, n = 0.f;
      for (int c = 0; c < C; ++c) {
        const float w = Wg[(f * H + h) * C + c];
        s += w * as[c * H + h];
        n += w * an[c * H + h];
      }
      p[NW + 2 * HC + tid] = s;
      p[NW + 2 * HC + CIN * H + tid] = n;
    }
    __syncthreads();
  }
};

__device__ __forceinline__ float gat_leaky(float e) { return e > 0.f ? e : GAT_SLOPE * e; }

__device__ __forceinline__ float gat_act(float o, float al, int act) {
  if (act == GAT_ACT_PRELU) return o > 0.f ? o : al * o;
  if (act == GAT_ACT_RELU) return fmaxf(o, 0.f);
  return o;
}
__device__ __forceinline__ float gat_act_grad(float o, float al, int act) {
  if (act == GAT_ACT_PRELU) return o > 0.f ? 1.f : al;
  if (act == GAT_ACT_RELU) return o > 0.f ? 1.f : 0.f;
  return 1.f;
}

// ------------------------------------------------------------------ instance table
#define GQ_GAT_DISPATCH(CIN_RT, C_RT, H_RT, ...)                                         \
  do {                                                                                   \
    const int key__ = (int)(CIN_RT) * 1000 + (int)(C_RT) * 10 + (int)(H_RT);             \
    switch (key__) {                                                                     \
      GQ_GAT_CASES(1, __VA_ARGS__) GQ_GAT_CASES(2, __VA_ARGS__)                          \
      GQ_GAT_CASES(3, __VA_ARGS__) GQ_GAT_CASES(4, __VA_ARGS__)                          \
      default: TORCH_CHECK(false, "gat: Cin 1..4, C in {8, 16, 32}, H in {1, 2}");       \
    }                                                                                    \
  } while (0)
#define GQ_GAT_CASE(CI, CC, HH, ...) \
  case CI * 1000 + CC * 10 + HH: { constexpr int CIN = CI, C = CC, H = HH; __VA_ARGS__; } break;
#define GQ_GAT_CASES(CI, ...)                                                            \
  GQ_GAT_CASE(CI, 8, 1, __VA_ARGS__) GQ_GAT_CASE(CI, 16, 1, __VA_ARGS__)                 \
  GQ_GAT_CASE(CI, 32, 1, __VA_ARGS__) GQ_GAT_CASE(CI, 8, 2, __VA_ARGS__)                 \
  GQ_GAT_CASE(CI, 16, 2, __VA_ARGS__) GQ_GAT_CASE(CI, 32, 2, __VA_ARGS__)

inline int gat_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace gq
