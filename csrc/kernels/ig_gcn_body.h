// Device bodies of the path-folded integrated-gradients GCN kernels (ig.hip), shared between the
// zero-baseline kernels (BASE = false: x_s = alpha_s x, one offset A0 per channel) and the
// baseline kernels (BASE = true: x_s = xb + alpha_s (x - xb), a per-node offset). Everything the
// kernels exploit is "the pre-activation is linear in alpha":
//   y_n(s) = alpha_s xs_n + A0_n
//   xs_n   = ((x_n - xb_n) . W_f) sc_f                        (slope)
//   A0_n   = (xb_n . W_f) sc_f + bias_f sc_f + shift_f        (offset; A0 alone when xb = 0)
// y_n(s) stays monotone in s, so PReLU still flips at most once per (node, channel). The BASE =
// false instances are the code the zero-baseline kernels had before the baseline ones existed.
#pragma once
#include "common.h"

namespace gq {

constexpr int IGG_NMAX = 32;      // nodes per window (lanes of the backward's node axis)
constexpr int IGG_SCH = 32;       // path points staged per LDS pass of the backward
constexpr int IGG_FSG = 8;        // path points per coalesced store pass of the forward
constexpr int IGG_KMAX = 128;     // path points per launch (the host splits longer chunks)
constexpr int IGG_BWB = 4;        // windows per backward workgroup (128 threads: lanes = nodes)

// Slope and offset of one (node, channel) from a baseline: explicit fused multiply-adds in one
// order, so the forward and the backward evaluate the flip predicate on bitwise equal operands.
template <int Cin>
__device__ __forceinline__ void igg_slope_offset(const float* __restrict__ xp, const float* __restrict__ xq,
                                                 const float (&wk)[Cin], float sc, float A0, float& xs,
                                                 float& A0n) {
  float zd = 0.f, zb = 0.f;
#pragma unroll
  for (int k = 0; k < Cin; ++k) {
    const float q = xq[k];
    zd = __fmaf_rn(xp[k] - q, wk[k], zd);
    zb = __fmaf_rn(q, wk[k], zb);
  }
  xs = zd * sc;
  A0n = __fmaf_rn(zb, sc, A0);
}

// forward: out [T][Mp][Cp] = [anomaly channels | sum_n w_bn prelu(y_n(s)) | 0] (see ig.hip)
template <int Cin, int F, int NM, bool BASE>        // NM >= N: node slots (unrolled)
__device__ __forceinline__ void ig_gcn_pool_fwd_body(
    float* __restrict__ so, const float* __restrict__ x, const float* __restrict__ xbase,
    const float* __restrict__ w, const float* __restrict__ anom, const float* __restrict__ abase,
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ prelu_a, const float* __restrict__ alphas,
    float* __restrict__ out, int B, int T, int N, int Ca, int kk, int Mp, int Cp) {
  constexpr int BB = 256 / F;                       // windows per workgroup
  const int f = threadIdx.x % F, bl = threadIdx.x / F;
  const int t = blockIdx.y, b0 = blockIdx.x * BB, b = b0 + bl;
  const int nb = min(BB, B - b0);
  if (blockIdx.x == 0) {                            // zero the padding rows kk*B .. Mp-1 of step t
    const long z0 = ((long)t * Mp + (long)kk * B) * Cp, z1 = ((long)t + 1) * Mp * Cp;
    for (long e = z0 + threadIdx.x; e < z1; e += 256) out[e] = 0.f;
  }
  const bool live = b < B;
  float wk[Cin];
#pragma unroll
  for (int k = 0; k < Cin; ++k) wk[k] = W[k * F + f];
  const float sc = scale[f], A0 = bias[f] * sc + shift[f], al = prelu_a[f];
  // y_n(s) = alpha_s * xs_n + A0 with xs_n = (x_bn . W_f) sc (zero baseline only; a baseline keeps
  // no per-node arrays: its loop below works on scalars. Declared here, not inside the branch, so
  // that the zero-baseline instances keep their statement order and with it their registers.)
  [[maybe_unused]] float xs[NM], wn[NM];
  const float* xp = x + ((long)(live ? b : 0) * T + t) * (long)N * Cin;
  if constexpr (!BASE) {
#pragma unroll
    for (int n = 0; n < NM; ++n) {
      float z = 0.f;
      if (n < N) {
#pragma unroll
        for (int k = 0; k < Cin; ++k) z += xp[n * Cin + k] * wk[k];
      }
      xs[n] = z * sc;
      wn[n] = (live && n < N) ? w[(long)b * N + n] : 0.f;
    }
  }
  const float a_in = (live && f < Ca) ? anom[((long)b * T + t) * Ca + f] : 0.f;
  // Piecewise-linear form over the path (see the backward): prelu(y_n(s)) = c_n(s) y_n(s) with
  // c_n in {1, al} flipping at most once, at j_n, so out(s) = alpha_s S1(s) + S0(s) where
  // S1 = sum_n w_n c_n(s) xs_n and S0 = sum_n w_n c_n(s) A0_n change only at the flips: per node one
  // binary search, then a running sum over the steps (O(N log kk + kk) per thread, not O(N kk)).
  // (Zero baseline: A0_n = A0 for every node, S0 carries sum_n w_n c_n(s) and A0 multiplies it.)
  const float a_first = alphas[0], a_last = alphas[kk - 1];
  float S1 = 0.f, S0 = 0.f;
  int jn[NM];
  float d1[NM], d0[NM];
  if constexpr (!BASE) {
#pragma unroll
    for (int n = 0; n < NM; ++n) {
      const bool p0 = a_first * xs[n] + A0 > 0.f, p1 = a_last * xs[n] + A0 > 0.f;
      const float c0 = p0 ? 1.f : al, c1 = p1 ? 1.f : al;
      S1 += wn[n] * c0 * xs[n];
      S0 += wn[n] * c0;
      int j = kk;                                     // no flip along the path
      if (p0 != p1) {
        int lo = 0, hi = kk - 1;                      // p(lo) == p0, p(hi) != p0
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if ((alphas[mid] * xs[n] + A0 > 0.f) == p0) lo = mid;
          else hi = mid;
        }
        j = hi;
      }
      jn[n] = j;
      d1[n] = wn[n] * (c1 - c0) * xs[n];
      d0[n] = wn[n] * (c1 - c0);
    }
  } else {
    // The same loop with a per-node offset A0n in the place of A0 (it lives only inside this loop: it
    // folds into d0[n] and the initial S0). The flip search and the d1 / d0 bookkeeping of the two
    // branches must stay identical apart from that offset; they are two copies so that the
    // zero-baseline instances keep the code they had.
    const float* xq = xbase + ((long)(live ? b : 0) * T + t) * (long)N * Cin;
#pragma unroll
    for (int n = 0; n < NM; ++n) {
      float xsn = 0.f, A0n = A0;
      if (n < N) igg_slope_offset<Cin>(xp + n * Cin, xq + n * Cin, wk, sc, A0, xsn, A0n);
      const float wnn = (live && n < N) ? w[(long)b * N + n] : 0.f;
      const bool p0 = a_first * xsn + A0n > 0.f, p1 = a_last * xsn + A0n > 0.f;
      const float c0 = p0 ? 1.f : al, c1 = p1 ? 1.f : al;
      S1 += wnn * c0 * xsn;
      S0 += wnn * c0 * A0n;
      int j = kk;                                     // no flip along the path
      if (p0 != p1) {
        int lo = 0, hi = kk - 1;                      // p(lo) == p0, p(hi) != p0
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if ((alphas[mid] * xsn + A0n > 0.f) == p0) lo = mid;
          else hi = mid;
        }
        j = hi;
      }
      jn[n] = j;
      d1[n] = wnn * (c1 - c0) * xsn;
      d0[n] = wnn * (c1 - c0) * A0n;
    }
  }
  float a_b = 0.f, a_d = 0.f;                       // baseline and slope of the anomaly channel
  if constexpr (BASE) {
    a_b = (live && f < Ca) ? abase[((long)b * T + t) * Ca + f] : 0.f;
    a_d = a_in - a_b;
  }
  float* D1 = so + IGG_FSG * BB * Cp + threadIdx.x;  // this thread's flip deltas [IGG_FSG][256]
  float* D0 = D1 + IGG_FSG * 256;
  const int rowf = nb * Cp;                         // floats of one step's rows (contiguous)
  for (int s0 = 0; s0 < kk; s0 += IGG_FSG) {
    const int ns = min(IGG_FSG, kk - s0);
#pragma unroll
    for (int q = 0; q < IGG_FSG; ++q) {
      D1[q * 256] = 0.f;
      D0[q * 256] = 0.f;
    }
#pragma unroll
    for (int n = 0; n < NM; ++n) {
      const int r = jn[n] - s0;
      if (r >= 0 && r < IGG_FSG) {
        D1[r * 256] += d1[n];
        D0[r * 256] += d0[n];
      }
    }
    for (int si = 0; si < ns; ++si) {
      const float a = alphas[s0 + si];
      S1 += D1[si * 256];
      S0 += D0[si * 256];
      float* o = so + (si * BB + bl) * Cp;
      if constexpr (BASE) {
        o[Ca + f] = a * S1 + S0;
        // (alpha == 1 writes the input itself: the path's last point is the real window)
        if (f < Ca) o[f] = a == 1.f ? a_in : __fmaf_rn(a, a_d, a_b);
      } else {
        o[Ca + f] = a * S1 + A0 * S0;
        if (f < Ca) o[f] = a * a_in;
      }
      for (int c = Ca + F + f; c < Cp; c += F) o[c] = 0.f;
    }
    __syncthreads();
    // coalesced float4 stores of the ns x nb rows (Cp % 4 == 0: every row starts 16-byte aligned)
    const int r4 = rowf / 4;
    for (int e = threadIdx.x; e < ns * r4; e += 256) {
      const int si = e / r4, q = e - si * r4;
      const float4 v = reinterpret_cast<const float4*>(so + si * BB * Cp)[q];
      reinterpret_cast<float4*>(out + ((long)t * Mp + (long)(s0 + si) * B + b0) * Cp)[q] = v;
    }
    __syncthreads();
  }
}

// Backward in closed form over the path. For a node n and channel f, y(s) = alpha_s xw + A0_n is
// monotone in s (alphas ascending), so prelu'(y(s)) takes one value c0 before a single flip index j
// and another, c1, after it. With the prefix sums P(j) = sum_{s<j} wt_s g_f(s) (Q = P(kk)):
//   sum_s wt_s prelu'(y(s)) g_f(s) = c0 P(j) + c1 (Q - P(j)),
// j found by a binary search on the same predicate (y > 0, same fma) the forward evaluated. Per
// (window, step) that is kk F prefix adds + N F log2(kk) compares instead of N F kk terms.
template <int Cin, int F, bool BASE>
__device__ __forceinline__ void ig_gcn_pool_bwd_body(
    float* __restrict__ sP, float* __restrict__ sA, const float* __restrict__ x,
    const float* __restrict__ xbase, const float* __restrict__ w, const float* __restrict__ mask,
    const float* __restrict__ g, const float* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ prelu_a,
    const float* __restrict__ alphas, const float* __restrict__ wts, float* __restrict__ acc_x,
    float* __restrict__ acc_a, int B, int T, int N, int Ca, int kk, int s_off, int Mp, int Cp, int first) {
  constexpr int PC = F + 4;                         // prefix channels: F GCN + 4 anomaly slots
  const int tid = threadIdx.x;
  const int n = tid % IGG_NMAX, bl = tid / IGG_NMAX;
  const int t = blockIdx.y, b0 = blockIdx.x * IGG_BWB, b = b0 + bl;
  const int rowp = (kk + 1) * PC;
  for (int e = tid; e < kk; e += IGG_BWB * IGG_NMAX) sA[e] = alphas[e];
  // prefix sums over the path points of wt_s g_c(s): thread (window, channel)
  for (int e = tid; e < IGG_BWB * PC; e += IGG_BWB * IGG_NMAX) {
    const int wb = e / PC, c = e - wb * PC, bb = b0 + wb;
    const int ch = c < F ? Ca + c : (c - F < Ca ? c - F : -1);
    float* P = sP + wb * rowp + c;
    float acc = 0.f;
    P[0] = 0.f;
    if (bb < B && ch >= 0) {
      const float* gp = g + ((long)t * Mp + (long)s_off * B + bb) * Cp + ch;
      const long stride = (long)B * Cp;
#pragma unroll 8
      for (int s = 0; s < kk; ++s) {
        acc += wts[s] * gp[s * stride];
        P[(s + 1) * PC] = acc;
      }
    } else {
      for (int s = 0; s < kk; ++s) P[(s + 1) * PC] = 0.f;
    }
  }
  __syncthreads();
  if (b >= B) return;
  const float* P = sP + bl * rowp;
  // (first: this launch writes the accumulators instead of adding - no zero-fill pass before it)
  if (n < Ca) {
    float* oa = acc_a + ((long)b * T + t) * Ca + n;
    *oa = (first ? 0.f : *oa) + P[kk * PC + F + n];
  }
  if (n >= N) return;
  float xv[Cin], qv[Cin];
#pragma unroll
  for (int k = 0; k < Cin; ++k) {
    xv[k] = x[(((long)b * T + t) * N + n) * Cin + k];
    qv[k] = BASE ? xbase[(((long)b * T + t) * N + n) * Cin + k] : 0.f;
  }
  const float mw = (mask[(long)b * N + n] != 0.f ? 1.f : 0.f) * w[(long)b * N + n];
  const float a_first = sA[0], a_last = sA[kk - 1];
  float d[Cin];
#pragma unroll
  for (int k = 0; k < Cin; ++k) d[k] = 0.f;
#pragma unroll 4
  for (int f = 0; f < F; ++f) {
    const float sc = scale[f];
    float wp[Cin];
    float xw, A0;
    const float al = prelu_a[f];
    if constexpr (BASE) {
      float wk[Cin];
#pragma unroll
      for (int k = 0; k < Cin; ++k) {
        wk[k] = W[k * F + f];
        wp[k] = wk[k] * sc;
      }
      igg_slope_offset<Cin>(xv, qv, wk, sc, bias[f] * sc + shift[f], xw, A0);
    } else {
      float z = 0.f;
#pragma unroll
      for (int k = 0; k < Cin; ++k) {
        const float wkf = W[k * F + f];
        z += xv[k] * wkf;
        wp[k] = wkf * sc;
      }
      xw = z * sc;
      A0 = bias[f] * sc + shift[f];
    }
    const bool p0 = a_first * xw + A0 > 0.f;
    const bool p1 = a_last * xw + A0 > 0.f;
    int lo = 0, hi = kk;                            // p(lo) == p0; first flip in (lo, hi]
    if (p1 != p0) {
      hi = kk - 1;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((sA[mid] * xw + A0 > 0.f) == p0) lo = mid;
        else hi = mid;
      }
    }
    const float Pj = P[hi * PC + f], Q = P[kk * PC + f];
    const float H = (p0 ? 1.f : al) * Pj + (p1 ? 1.f : al) * (Q - Pj);
#pragma unroll
    for (int k = 0; k < Cin; ++k) d[k] += wp[k] * H;
  }
  float* o = acc_x + (((long)b * T + t) * N + n) * Cin;
#pragma unroll
  for (int k = 0; k < Cin; ++k) o[k] = (first ? 0.f : o[k]) + mw * d[k];
}

}  // namespace gq
