// Integrated-gradients device steps (reference xai/libs/integrated_gradients.py
// :919-942 interpolation, :955-1004 per-step gradients, :1006-1015 trapezoid average, :1180-1208
// input scaling / negative-value policy).
//
// The explainer folds kk interpolation steps into the batch (gnnqc/xai/ig.py); these kernels are
// the elementwise ends of that pass, each ONE launch over all steps of a chunk:
//   ig_interp   out[i, b, e] = alpha[i] * v[b, e]                     (zero baseline path points)
//   ig_interp_base out[i, b, e] = fma(alpha[i], v[b, e] - b[b, e], b[b, e])  (any baseline; v at alpha 1)
//   ig_accum    acc[b, e]  += sum_i w[i] * g[i, b, e]                 (trapezoid weights, fixed
//                                                                     step order: deterministic)
//   ig_finalize out[b, e]   = policy(acc[b, e] * (scale ? v[b, e] : 1))  (keep / clip / abs)
// All three stream float4 granules when n % 4 == 0 (every step slice aligned), scalars otherwise.
#include "common.h"
#include "ig_gcn_body.h"

namespace gq {

__global__ __launch_bounds__(256) void ig_interp_kernel(const float* __restrict__ v, const float* __restrict__ alpha,
                                                        float* __restrict__ out, int kk, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  // float4 slices only when every step's slice out + s n stays 16-byte aligned (n % 4 == 0)
  const long n4 = n % 4 == 0 ? n / 4 : 0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 x = reinterpret_cast<const float4*>(v)[i];
    for (int s = 0; s < kk; ++s) {
      const float a = alpha[s];
      reinterpret_cast<float4*>(out + (size_t)s * n)[i] = make_float4(a * x.x, a * x.y, a * x.z, a * x.w);
    }
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride)
    for (int s = 0; s < kk; ++s) out[(size_t)s * n + i] = alpha[s] * v[i];
}

// out[s, i] = b[i] + alpha[s] (v[i] - b[i]); a step with alpha == 1 is v itself (the path's last point
// is the real input, bit for bit)
__device__ __forceinline__ float ig_lerp(float a, float v, float b) { return a == 1.f ? v : __fmaf_rn(a, v - b, b); }

__global__ __launch_bounds__(256) void ig_interp_base_kernel(const float* __restrict__ v, const float* __restrict__ b,
                                                             const float* __restrict__ alpha, float* __restrict__ out,
                                                             int kk, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long n4 = n % 4 == 0 ? n / 4 : 0;          // (as ig_interp: aligned step slices only)
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 x = reinterpret_cast<const float4*>(v)[i];
    const float4 y = reinterpret_cast<const float4*>(b)[i];
    for (int s = 0; s < kk; ++s) {
      const float a = alpha[s];
      reinterpret_cast<float4*>(out + (size_t)s * n)[i] =
          make_float4(ig_lerp(a, x.x, y.x), ig_lerp(a, x.y, y.y), ig_lerp(a, x.z, y.z), ig_lerp(a, x.w, y.w));
    }
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride)
    for (int s = 0; s < kk; ++s) out[(size_t)s * n + i] = ig_lerp(alpha[s], v[i], b[i]);
}

__global__ __launch_bounds__(256) void ig_accum_kernel(float* __restrict__ acc, const float* __restrict__ g,
                                                       const float* __restrict__ w, int kk, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long n4 = n % 4 == 0 ? n / 4 : 0;          // (as ig_interp: aligned step slices only)
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 a = reinterpret_cast<float4*>(acc)[i];
    for (int s = 0; s < kk; ++s) {
      const float ws = w[s];
      const float4 x = reinterpret_cast<const float4*>(g + (size_t)s * n)[i];
      a.x += ws * x.x;
      a.y += ws * x.y;
      a.z += ws * x.z;
      a.w += ws * x.w;
    }
    reinterpret_cast<float4*>(acc)[i] = a;
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
    float a = acc[i];
    for (int s = 0; s < kk; ++s) a += w[s] * g[(size_t)s * n + i];
    acc[i] = a;
  }
}

__global__ __launch_bounds__(256) void ig_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ v,
                                                          float* __restrict__ out, long n, int mode) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
    float r = acc[i] * (v != nullptr ? v[i] : 1.f);
    if (mode == 1) r = fmaxf(r, 0.f);
    else if (mode == 2) r = fabsf(r);
    out[i] = r;
  }
}

static int ig_grid(long n) { return (int)std::max<long>(1, std::min<long>((n / 4 + 255) / 256, 2048)); }

static void ig_check_aligned(const at::Tensor& t, const char* name) {
  check_f32_cuda(t, name);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "ig: ", name, " must be 16-byte aligned");
}

// v [B, ...] fp32, alpha [kk] -> [kk * B, ...]
at::Tensor ig_interp(const at::Tensor& v, const at::Tensor& alpha) {
  ig_check_aligned(v, "v");
  check_f32_cuda(alpha, "alpha");
  const int kk = (int)alpha.numel();
  TORCH_CHECK(kk >= 1 && v.dim() >= 1, "ig_interp: shapes");
  c10::DeviceGuard guard(v.device());
  std::vector<int64_t> shape(v.sizes().begin(), v.sizes().end());
  shape[0] *= kk;
  at::Tensor out = at::empty(shape, v.options());
  const long n = v.numel();
  if (n > 0)
    hipLaunchKernelGGL(ig_interp_kernel, dim3(ig_grid(n)), dim3(256), 0, stream(), v.data_ptr<float>(),
                       alpha.data_ptr<float>(), out.data_ptr<float>(), kk, n);
  GQ_LAUNCH_CHECK();
  return out;
}

// v, b [B, ...] fp32 (same shape), alpha [kk] -> [kk * B, ...]
at::Tensor ig_interp_base(const at::Tensor& v, const at::Tensor& b, const at::Tensor& alpha) {
  // (float4 granules are read only when numel % 4 == 0: only then must v and b be 16-byte aligned.
  // A draw cut from a stack of baselines starts numel * 4 bytes after the one before it.)
  if (v.numel() % 4 == 0) {
    ig_check_aligned(v, "v");
    ig_check_aligned(b, "b");
  } else {
    check_f32_cuda(v, "v");
    check_f32_cuda(b, "b");
  }
  check_f32_cuda(alpha, "alpha");
  const int kk = (int)alpha.numel();
  TORCH_CHECK(kk >= 1 && v.dim() >= 1 && b.sizes() == v.sizes(), "ig_interp_base: shapes");
  c10::DeviceGuard guard(v.device());
  std::vector<int64_t> shape(v.sizes().begin(), v.sizes().end());
  shape[0] *= kk;
  at::Tensor out = at::empty(shape, v.options());
  const long n = v.numel();
  if (n > 0)
    hipLaunchKernelGGL(ig_interp_base_kernel, dim3(ig_grid(n)), dim3(256), 0, stream(), v.data_ptr<float>(),
                       b.data_ptr<float>(), alpha.data_ptr<float>(), out.data_ptr<float>(), kk, n);
  GQ_LAUNCH_CHECK();
  return out;
}

// acc [B, ...] += sum_i w[i] g[i] with g [kk * B, ...] (step-major), w [kk]
void ig_accum(at::Tensor acc, const at::Tensor& g, const at::Tensor& w) {
  ig_check_aligned(acc, "acc");
  ig_check_aligned(g, "g");
  check_f32_cuda(w, "w");
  const int kk = (int)w.numel();
  TORCH_CHECK(kk >= 1 && g.numel() == acc.numel() * kk, "ig_accum: g must hold kk x acc elements");
  c10::DeviceGuard guard(acc.device());
  const long n = acc.numel();
  if (n > 0)
    hipLaunchKernelGGL(ig_accum_kernel, dim3(ig_grid(n)), dim3(256), 0, stream(), acc.data_ptr<float>(),
                       g.data_ptr<float>(), w.data_ptr<float>(), kk, n);
  GQ_LAUNCH_CHECK();
}

// policy(acc * v) (v empty: no input scaling); mode 0 keep, 1 clip at 0, 2 abs
at::Tensor ig_finalize(const at::Tensor& acc, const at::Tensor& v, int64_t mode) {
  check_f32_cuda(acc, "acc");
  TORCH_CHECK(mode >= 0 && mode <= 2, "ig_finalize: mode 0 keep / 1 clip / 2 abs");
  const float* vp = nullptr;
  if (v.numel() > 0) {
    check_f32_cuda(v, "v");
    TORCH_CHECK(v.numel() == acc.numel(), "ig_finalize: v / acc sizes");
    vp = v.data_ptr<float>();
  }
  c10::DeviceGuard guard(acc.device());
  at::Tensor out = at::empty_like(acc);
  const long n = acc.numel();
  if (n > 0)
    hipLaunchKernelGGL(ig_finalize_kernel, dim3(ig_grid(n * 4)), dim3(256), 0, stream(), acc.data_ptr<float>(), vp,
                       out.data_ptr<float>(), n, (int)mode);
  GQ_LAUNCH_CHECK();
  return out;
}

// =====================================================================================
// Path-folded GeneralConv + BatchNorm (eval) + PReLU + node pooling for the CML GCN (K10: the
// alpha scaling folded into the input load). The zero-baseline path point s of window b is
// x_s = alpha_s x_b, so its GCN pre-activation is z = alpha_s (x_b W) + bias: x W is computed
// ONCE per (window, step, node) and no kk x B copy of x (ig_interp: 430 MB per CML batch) or of
// the static adjacency / mask tensors exists. Rows of the time-major LSTM input are step-major
// (row = s * B + b), as the explainer's path batch.
//
// forward: out [T][Mp][Cp] = [alpha_s anom_b | sum_n w_bn prelu((alpha_s xW_bn + bias) sc + sh) | 0]
// backward: the input gradients of every path point, trapezoid-weighted and summed over the
// chunk's steps in ONE pass (ig_accum folded in, fixed step order: deterministic):
//   acc_x[b,t,n,k]  += sum_s wt_s sum_f W[k,f] m_n w_bn sc_f prelu'(y) g_f(s)
//   acc_a[b,t,c]    += sum_s wt_s g_c(s)           (g = dL/d out, rows s * B + b)
// The workgroup of (t, 256 / F windows) first stages every step's output-gradient rows of its
// windows (contiguous per step) in LDS, so all those loads are in flight at once.
// (constants and the device bodies, shared with the baseline kernels below: ig_gcn_body.h)
template <int Cin, int F, int NM>                  // NM >= N: node slots (unrolled)
__global__ __launch_bounds__(256) void ig_gcn_pool_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ anom,
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ prelu_a, const float* __restrict__ alphas,
    float* __restrict__ out, int B, int T, int N, int Ca, int kk, int Mp, int Cp) {
  extern __shared__ __attribute__((aligned(16))) float so[];   // [IGG_FSG][BB][Cp] output rows
  ig_gcn_pool_fwd_body<Cin, F, NM, false>(so, x, nullptr, w, anom, nullptr, W, bias, scale, shift, prelu_a, alphas,
                                          out, B, T, N, Ca, kk, Mp, Cp);
}

template <int Cin, int F>
__global__ __launch_bounds__(IGG_BWB * IGG_NMAX) void ig_gcn_pool_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ mask,
    const float* __restrict__ g, const float* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ prelu_a,
    const float* __restrict__ alphas, const float* __restrict__ wts, float* __restrict__ acc_x,
    float* __restrict__ acc_a, int B, int T, int N, int Ca, int kk, int s_off, int Mp, int Cp, int first) {
  extern __shared__ __attribute__((aligned(16))) float sP[];   // [IGG_BWB][kk + 1][PC]
  __shared__ float sA[IGG_KMAX];
  ig_gcn_pool_bwd_body<Cin, F, false>(sP, sA, x, nullptr, w, mask, g, W, bias, scale, shift, prelu_a, alphas, wts,
                                      acc_x, acc_a, B, T, N, Ca, kk, s_off, Mp, Cp, first);
}

// The same from a baseline (xb [B,T,N,Cin], ab [B,T,Ca]): path point s is xb + alpha_s (x - xb) and
// ab + alpha_s (anom - ab), the slope taken from x - xb and the offset A0_n per node (ig_gcn_body.h).
// acc_x and acc_a are the gradients at the path points, as above: the caller scales by x - xb.
template <int Cin, int F, int NM>
__global__ __launch_bounds__(256) void ig_gcn_pool_fwd_base_kernel(
    const float* __restrict__ x, const float* __restrict__ xbase, const float* __restrict__ w,
    const float* __restrict__ anom, const float* __restrict__ abase, const float* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ prelu_a, const float* __restrict__ alphas, float* __restrict__ out, int B, int T,
    int N, int Ca, int kk, int Mp, int Cp) {
  extern __shared__ __attribute__((aligned(16))) float so[];   // [IGG_FSG][BB][Cp] output rows
  ig_gcn_pool_fwd_body<Cin, F, NM, true>(so, x, xbase, w, anom, abase, W, bias, scale, shift, prelu_a, alphas, out, B,
                                         T, N, Ca, kk, Mp, Cp);
}

template <int Cin, int F>
__global__ __launch_bounds__(IGG_BWB * IGG_NMAX) void ig_gcn_pool_bwd_base_kernel(
    const float* __restrict__ x, const float* __restrict__ xbase, const float* __restrict__ w,
    const float* __restrict__ mask, const float* __restrict__ g, const float* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ prelu_a, const float* __restrict__ alphas, const float* __restrict__ wts,
    float* __restrict__ acc_x, float* __restrict__ acc_a, int B, int T, int N, int Ca, int kk, int s_off, int Mp,
    int Cp, int first) {
  extern __shared__ __attribute__((aligned(16))) float sP[];   // [IGG_BWB][kk + 1][PC]
  __shared__ float sA[IGG_KMAX];
  ig_gcn_pool_bwd_body<Cin, F, true>(sP, sA, x, xbase, w, mask, g, W, bias, scale, shift, prelu_a, alphas, wts, acc_x,
                                     acc_a, B, T, N, Ca, kk, s_off, Mp, Cp, first);
}

#define GQ_IGG_DISPATCH(CIN_RT, F_RT, ...)                                                         \
  do {                                                                                             \
    if (CIN_RT == 2 && F_RT == 16) { constexpr int CIN = 2, FF = 16; __VA_ARGS__; }                \
    else if (CIN_RT == 1 && F_RT == 16) { constexpr int CIN = 1, FF = 16; __VA_ARGS__; }           \
    else if (CIN_RT == 3 && F_RT == 16) { constexpr int CIN = 3, FF = 16; __VA_ARGS__; }           \
    else if (CIN_RT == 2 && F_RT == 32) { constexpr int CIN = 2, FF = 32; __VA_ARGS__; }           \
    else if (CIN_RT == 2 && F_RT == 8) { constexpr int CIN = 2, FF = 8; __VA_ARGS__; }             \
    else TORCH_CHECK(false, "ig_gcn_pool: unsupported Cin ", CIN_RT, " / F ", F_RT);               \
  } while (0)

bool ig_gcn_shape_ok(int64_t Cin, int64_t F, int64_t N) {
  return N >= 1 && N <= IGG_NMAX &&
         ((Cin == 2 && (F == 8 || F == 16 || F == 32)) || ((Cin == 1 || Cin == 3) && F == 16));
}

// x [B,T,N,Cin], w [B,N] pool weights (gcn_prep), anom [B,T,Ca] (or empty), st rows 2/3 = BN scale /
// shift (eval), alphas [kk]. Returns [T, Mp, Cp] with Mp = kk*B rounded up to 16.
// (xb / ab: the baseline of ig_gcn_pool_fwd_base, nullptr for the zero baseline)
static at::Tensor ig_gcn_pool_fwd_impl(const at::Tensor& x, const at::Tensor* xb, const at::Tensor& w,
                                       const at::Tensor& anom, const at::Tensor* ab, const at::Tensor& W,
                                       const at::Tensor& b, const at::Tensor& scale, const at::Tensor& shift,
                                       const at::Tensor& alpha, const at::Tensor& alphas, int64_t Cp) {
  for (auto* p : {&x, &w, &W, &b, &scale, &shift, &alpha, &alphas}) check_f32_cuda(*p, "ig_gcn_pool_fwd input");
  TORCH_CHECK(x.dim() == 4, "ig_gcn_pool_fwd: x must be [B,T,N,Cin]");
  const int B = x.size(0), T = x.size(1), N = x.size(2), Cin = x.size(3), F = W.size(1);
  TORCH_CHECK(ig_gcn_shape_ok(Cin, F, N) && W.size(0) == Cin, "ig_gcn_pool_fwd: unsupported shape");
  TORCH_CHECK(w.size(0) == B && w.size(1) == N && b.numel() == F && scale.numel() == F && shift.numel() == F &&
                  alpha.numel() == F, "ig_gcn_pool_fwd: parameter shapes");
  int Ca = 0;
  if (anom.numel() > 0) {
    check_f32_cuda(anom, "anom");
    TORCH_CHECK(anom.dim() == 3 && anom.size(0) == B && anom.size(1) == T, "ig_gcn_pool_fwd: anom must be [B,T,Ca]");
    Ca = anom.size(2);
  }
  TORCH_CHECK(Ca <= F && Cp >= Ca + F && Cp % 4 == 0, "ig_gcn_pool_fwd: Cp / Ca");
  if (xb != nullptr) {
    check_f32_cuda(*xb, "ig_gcn_pool_fwd_base xb");
    TORCH_CHECK(xb->sizes() == x.sizes(), "ig_gcn_pool_fwd_base: xb must have the shape of x");
    TORCH_CHECK(ab->numel() == anom.numel() && (Ca == 0 || ab->sizes() == anom.sizes()),
                "ig_gcn_pool_fwd_base: ab must have the shape of anom");
    if (Ca) check_f32_cuda(*ab, "ig_gcn_pool_fwd_base ab");
  }
  const int kk = (int)alphas.numel();
  TORCH_CHECK(kk >= 1, "ig_gcn_pool_fwd: no path points");
  const long Mp = ((long)kk * B + 15) / 16 * 16;
  c10::DeviceGuard guard(x.device());
  at::Tensor out = at::empty({T, Mp, Cp}, x.options());
#define GQ_IGG_FWD(NMV)                                                                                     \
  if (xb == nullptr)                                                                                        \
  hipLaunchKernelGGL((ig_gcn_pool_fwd_kernel<CIN, FF, NMV>), dim3((B + 256 / FF - 1) / (256 / FF), T), dim3(256), \
                     ((size_t)IGG_FSG * (256 / FF) * Cp + 2 * IGG_FSG * 256) * sizeof(float), stream(),           \
                     x.data_ptr<float>(),                                                                           \
                     w.data_ptr<float>(), Ca ? anom.data_ptr<float>() : nullptr, W.data_ptr<float>(),               \
                     b.data_ptr<float>(), scale.data_ptr<float>(), shift.data_ptr<float>(), alpha.data_ptr<float>(), \
                     alphas.data_ptr<float>(), out.data_ptr<float>(), B, T, N, Ca, kk, (int)Mp, (int)Cp);           \
  else                                                                                                      \
  hipLaunchKernelGGL((ig_gcn_pool_fwd_base_kernel<CIN, FF, NMV>), dim3((B + 256 / FF - 1) / (256 / FF), T),       \
                     dim3(256), ((size_t)IGG_FSG * (256 / FF) * Cp + 2 * IGG_FSG * 256) * sizeof(float), stream(), \
                     x.data_ptr<float>(), xb->data_ptr<float>(), w.data_ptr<float>(),                               \
                     Ca ? anom.data_ptr<float>() : nullptr, Ca ? ab->data_ptr<float>() : nullptr,                   \
                     W.data_ptr<float>(), b.data_ptr<float>(), scale.data_ptr<float>(), shift.data_ptr<float>(),    \
                     alpha.data_ptr<float>(), alphas.data_ptr<float>(), out.data_ptr<float>(), B, T, N, Ca, kk,     \
                     (int)Mp, (int)Cp)
  GQ_IGG_DISPATCH(Cin, F,
      if (N <= 8) { GQ_IGG_FWD(8); } else if (N <= 16) { GQ_IGG_FWD(16); } else if (N <= 24) { GQ_IGG_FWD(24); }
      else { GQ_IGG_FWD(32); });
#undef GQ_IGG_FWD
  GQ_LAUNCH_CHECK();
  return out;
}

at::Tensor ig_gcn_pool_fwd(const at::Tensor& x, const at::Tensor& w, const at::Tensor& anom, const at::Tensor& W,
                           const at::Tensor& b, const at::Tensor& scale, const at::Tensor& shift,
                           const at::Tensor& alpha, const at::Tensor& alphas, int64_t Cp) {
  return ig_gcn_pool_fwd_impl(x, nullptr, w, anom, nullptr, W, b, scale, shift, alpha, alphas, Cp);
}

// the path from the baseline xb [B,T,N,Cin] (contiguous) / ab [B,T,Ca] (empty exactly when anom is)
at::Tensor ig_gcn_pool_fwd_base(const at::Tensor& x, const at::Tensor& xb, const at::Tensor& w, const at::Tensor& anom,
                                const at::Tensor& ab, const at::Tensor& W, const at::Tensor& b,
                                const at::Tensor& scale, const at::Tensor& shift, const at::Tensor& alpha,
                                const at::Tensor& alphas, int64_t Cp) {
  return ig_gcn_pool_fwd_impl(x, &xb, w, anom, &ab, W, b, scale, shift, alpha, alphas, Cp);
}

// g = dL/d out [T, Mp, Cp] of ig_gcn_pool_fwd; accumulates into acc_x [B,T,N,Cin] and acc_a [B,T,Ca]
// (overwrite: the first launch writes them - uninitialised accumulators need no zero fill).
static void ig_gcn_pool_bwd_impl(const at::Tensor& x, const at::Tensor* xb, const at::Tensor& w,
                                 const at::Tensor& mask, const at::Tensor& g, const at::Tensor& W,
                                 const at::Tensor& b, const at::Tensor& scale, const at::Tensor& shift,
                                 const at::Tensor& alpha, const at::Tensor& alphas, const at::Tensor& wts,
                                 at::Tensor acc_x, at::Tensor acc_a, bool overwrite) {
  for (auto* p : {&x, &w, &mask, &g, &W, &b, &scale, &shift, &alpha, &alphas, &wts})
    check_f32_cuda(*p, "ig_gcn_pool_bwd input");
  check_f32_cuda(acc_x, "ig_gcn_pool_bwd acc_x");
  const int B = x.size(0), T = x.size(1), N = x.size(2), Cin = x.size(3), F = W.size(1);
  TORCH_CHECK(ig_gcn_shape_ok(Cin, F, N), "ig_gcn_pool_bwd: unsupported shape");
  const int kk = (int)alphas.numel();
  TORCH_CHECK(wts.numel() == kk && kk >= 1, "ig_gcn_pool_bwd: weights per path point");
  TORCH_CHECK(acc_x.sizes() == x.sizes() && mask.numel() == (long)B * N && w.numel() == (long)B * N,
              "ig_gcn_pool_bwd: accumulator / mask shapes");
  TORCH_CHECK(g.dim() == 3 && g.size(0) == T && g.size(1) >= (long)kk * B, "ig_gcn_pool_bwd: g must be [T, Mp, Cp]");
  const int Cp = g.size(2);
  int Ca = 0;
  if (acc_a.numel() > 0) {
    check_f32_cuda(acc_a, "acc_a");
    TORCH_CHECK(acc_a.dim() == 3 && acc_a.size(0) == B && acc_a.size(1) == T, "ig_gcn_pool_bwd: acc_a [B,T,Ca]");
    Ca = acc_a.size(2);
  }
  TORCH_CHECK(Cp >= Ca + F && Ca <= 4, "ig_gcn_pool_bwd: Cp / Ca");
  if (xb != nullptr) {
    check_f32_cuda(*xb, "ig_gcn_pool_bwd_base xb");
    TORCH_CHECK(xb->sizes() == x.sizes(), "ig_gcn_pool_bwd_base: xb must have the shape of x");
  }
  c10::DeviceGuard guard(x.device());
  // path points in slices of at most IGG_KMAX (the prefix table of a workgroup lives in LDS)
  for (int s0 = 0; s0 < kk; s0 += IGG_KMAX) {
    const int ks = std::min(IGG_KMAX, kk - s0);
    const size_t smem = (size_t)IGG_BWB * (ks + 1) * (F + 4) * sizeof(float);
    GQ_IGG_DISPATCH(Cin, F,
        if (xb == nullptr)
        hipLaunchKernelGGL((ig_gcn_pool_bwd_kernel<CIN, FF>), dim3((B + IGG_BWB - 1) / IGG_BWB, T),
                           dim3(IGG_BWB * IGG_NMAX), smem, stream(), x.data_ptr<float>(), w.data_ptr<float>(),
                           mask.data_ptr<float>(), g.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                           scale.data_ptr<float>(), shift.data_ptr<float>(), alpha.data_ptr<float>(),
                           alphas.data_ptr<float>() + s0, wts.data_ptr<float>() + s0, acc_x.data_ptr<float>(),
                           Ca ? acc_a.data_ptr<float>() : nullptr, B, T, N, Ca, ks, s0, (int)g.size(1), Cp,
                           (overwrite && s0 == 0) ? 1 : 0);
        else
        hipLaunchKernelGGL((ig_gcn_pool_bwd_base_kernel<CIN, FF>), dim3((B + IGG_BWB - 1) / IGG_BWB, T),
                           dim3(IGG_BWB * IGG_NMAX), smem, stream(), x.data_ptr<float>(), xb->data_ptr<float>(),
                           w.data_ptr<float>(), mask.data_ptr<float>(), g.data_ptr<float>(), W.data_ptr<float>(),
                           b.data_ptr<float>(), scale.data_ptr<float>(), shift.data_ptr<float>(),
                           alpha.data_ptr<float>(), alphas.data_ptr<float>() + s0, wts.data_ptr<float>() + s0,
                           acc_x.data_ptr<float>(), Ca ? acc_a.data_ptr<float>() : nullptr, B, T, N, Ca, ks, s0,
                           (int)g.size(1), Cp, (overwrite && s0 == 0) ? 1 : 0));
    GQ_LAUNCH_CHECK();
  }
}

void ig_gcn_pool_bwd(const at::Tensor& x, const at::Tensor& w, const at::Tensor& mask, const at::Tensor& g,
                     const at::Tensor& W, const at::Tensor& b, const at::Tensor& scale, const at::Tensor& shift,
                     const at::Tensor& alpha, const at::Tensor& alphas, const at::Tensor& wts, at::Tensor acc_x,
                     at::Tensor acc_a, bool overwrite) {
  ig_gcn_pool_bwd_impl(x, nullptr, w, mask, g, W, b, scale, shift, alpha, alphas, wts, acc_x, acc_a, overwrite);
}

void ig_gcn_pool_bwd_base(const at::Tensor& x, const at::Tensor& xb, const at::Tensor& w, const at::Tensor& mask,
                          const at::Tensor& g, const at::Tensor& W, const at::Tensor& b, const at::Tensor& scale,
                          const at::Tensor& shift, const at::Tensor& alpha, const at::Tensor& alphas,
                          const at::Tensor& wts, at::Tensor acc_x, at::Tensor acc_a, bool overwrite) {
  ig_gcn_pool_bwd_impl(x, &xb, w, mask, g, W, b, scale, shift, alpha, alphas, wts, acc_x, acc_a, overwrite);
}
#undef GQ_IGG_DISPATCH

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("ig_gcn_pool_fwd", &gq::ig_gcn_pool_fwd);
  m.impl("ig_gcn_pool_bwd", &gq::ig_gcn_pool_bwd);
  m.impl("ig_gcn_pool_fwd_base", &gq::ig_gcn_pool_fwd_base);
  m.impl("ig_gcn_pool_bwd_base", &gq::ig_gcn_pool_bwd_base);
  m.impl("ig_interp", &gq::ig_interp);
  m.impl("ig_interp_base", &gq::ig_interp_base);
  m.impl("ig_accum", &gq::ig_accum);
  m.impl("ig_finalize", &gq::ig_finalize);
}
