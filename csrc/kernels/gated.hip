// Fused GatedGraphConv + node pooling + concat for the CML front end.
//
// spektral GatedGraphConv(channels, n_layers) with a Keras GRUCell(reset_after=True, gate order z, r, h)
// on a dense per-sample graph, followed by `timeseries_pooling` and Concatenate([flagged series,
// pooled]) (gnnqc/models/graphconv.py GatedGraphConv is the eager form). For a row (b, t), node i
// and nb_i = { j : adj_ij > 0 }:
//
//   h_i^0     = [x_i | 0]                                        (Cin values, zero-padded to C)
//   p_j       = h_j^l W_l,   m_i = sum_{j in nb_i} p_j           (no self loop, mask not folded in)
//   a = m_i K + bias[0],     g = h_i^l R + bias[1]               K, R: [C, 3C]
//   z = sig(a_z + g_z), r = sig(a_r + g_r), c = tanh(a_h + r g_h)
//   h_i^{l+1} = z h_i^l + (1 - z) c
//   out       = [anom | sum_i pw_i act(h_i^L)]                   pw: node pool weights (mask included)
//
// Mapping (all kernels, as in gat.hip / edge.hip / agnn.hip): one lane per (row = (b, t), node i); a
// row's NP = pow2 >= N lanes are adjacent lanes of one wave, so the node pool is a shuffle reduction
// and N <= 64. The neighbour words are edge_adj_bits' (edge.hip): the row word for m, the transposed
// word for the backward's dp. Every lane walks every layer (a masked node still sends its message).
//
// Where the products run.
//  * The per-node products (h W_l, m K, h R and the backward's three transposed ones) are per-lane
//    fmaf chains over register arrays. The weights are wave-uniform reads through const __restrict__
//    kernel arguments: scalar loads, the operand of the v_fma comes from an SGPR, no LDS staging.
//    Layer 0 multiplies only the first 4 rows of W_0 and R (h^0 is zero past Cin <= 4).
//  * The parameter gradients dK = m^T da, dR = h^T dg, dW_l = h^T dp are sums of outer products over
//    lanes. Every lane stages [m | h^l | one C-wide slice of da / dg / dp] in LDS, one row per lane,
//    and the waves read it back as the A / B operands of the exact-f32 MFMA 16x16x4 (A[m][k] =
//    X[lane k][m], B[k][n] = Y[lane k][n], one step per 4 lanes). The 10 slices [dK (3) | dR (3) |
//    dW_0..3] are C x C each; the four waves split them so that a wave keeps ONE 16x16 tile per slice
//    in registers over the workgroup's passes, 40 accumulator registers at every C: at C = 32 wave w
//    owns tile w of the 2 x 2 tiles over all 256 rows, at C <= 16 it owns rows [64 w, 64 w + 64) of
//    the single tile (all 160 tile registers per wave spilled at C = 32). dbias and dalpha are column
//    sums of the same staged slices (64 reads per lane). The staging pitch is 48 floats (C <= 16) or
//    112 (C = 32): both = 16 or 48 mod 64, so the four 16-lane groups of an operand read (rows 4s ..
//    4s + 3) fall on four different bank quarters.
//  * The recomputed states: the backward re-walks the layers from h^0 for every l (L (L + 1) / 2
//    layer evaluations instead of L). Keeping h^0 .. h^L would take (L + 1) C registers per lane (160
//    at C = 32, L = 4) or 128 KB of LDS next to the 148 KB already used at C = 32 (36 KB slab + 112 KB
//    staging; 20 + 48 KB at C = 16); the re-walk needs neither and costs nothing at L = 1 and one
//    extra layer at L = 2.
//  * The message slab: one node's p (forward) or dm (backward) per lane at a pitch of C + 4 floats,
//    i.e. C/4 + 1 sixteen-byte slots, an odd number: 16 consecutive nodes never share a slot.
//
// The end of gated_pool_bwd adds the waves' partial tiles in a fixed order and writes ONE record per
// workgroup, laid out like the parameters: [dW (L C C) | dK (C 3C) | dR (C 3C) | dbias (2 3C) |
// dalpha (C)]. A fixed-order column sum and gated_bwd_finalize follow. gated_pool_bwd_input is the
// same walk without the staging and writes dx = dh^0[:Cin]; each dp and dx element is written by one
// lane. No float atomics anywhere: results are bitwise reproducible.
#include "gat_common.h"

namespace gq {

constexpr int GATED_MAX_N = 64;
constexpr int GATED_MAX_L = 4;
constexpr int GATED_GRID_CAP = 256;      // workgroups per launch: more rows take several passes

typedef float gated_f4 __attribute__((ext_vector_type(4)));

template <int C>
struct Gated {
  static constexpr int PP = C + 4;                               // message slab pitch (floats)
  static constexpr int CW = C < 16 ? 16 : C;                     // slice width padded to MFMA tiles
  static constexpr int TT = CW / 16;                             // tiles per side of a C x C slice
  static constexpr int SP = 3 * CW + (C == 32 ? 16 : 0);         // staging pitch: [X1 | X2 | Y]
  static constexpr int NT = TT * TT;
  static constexpr int RG = 4 / NT;                              // row groups the waves split into
  static constexpr int GR = 256 / RG;                            // staged rows per group
};

__device__ __forceinline__ float gated_sig(float v) { return 1.f / (1.f + __expf(-v)); }
__device__ __forceinline__ float gated_tanh(float v) { return 2.f / (1.f + __expf(-2.f * v)) - 1.f; }

// y[c] += sum_{k < KN} v[k] M[k ld + c]   (M wave-uniform: scalar loads)
template <int C, int KN>
__device__ __forceinline__ void gated_mv(const float (&v)[C], const float* __restrict__ M, int ld, float (&y)[C]) {
#pragma unroll
  for (int k = 0; k < KN; ++k) {
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = fmaf(v[k], M[k * ld + c], y[c]);
  }
}

// y[k] += sum_c v[c] M[k ld + c]
template <int C>
__device__ __forceinline__ void gated_mvT(const float (&v)[C], const float* __restrict__ M, int ld, float (&y)[C]) {
#pragma unroll
  for (int k = 0; k < C; ++k) {
    float s = y[k];
#pragma unroll
    for (int c = 0; c < C; ++c) s = fmaf(v[c], M[k * ld + c], s);
    y[k] = s;
  }
}

template <int C>
__device__ __forceinline__ void gated_put(float* s, const float (&v)[C]) {
#pragma unroll
  for (int q = 0; q < C / 4; ++q)
    reinterpret_cast<float4*>(s)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// m = sum of the slabs of the set bits of w
template <int C>
__device__ __forceinline__ void gated_gather(gat_bits_t w, const float* sr, float (&m)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) m[c] = 0.f;
  for (; w; w &= w - 1) {
    const int j = __ffsll((long long)w) - 1;
    const float4* p = reinterpret_cast<const float4*>(sr + j * Gated<C>::PP);
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
      const float4 v = p[q];
      m[4 * q] += v.x, m[4 * q + 1] += v.y, m[4 * q + 2] += v.z, m[4 * q + 3] += v.w;
    }
  }
}

// One message round: h -> hn, with the intermediates the backward needs. FIRST: h is h^0, zero past
// channel 4, so only 4 rows of W_l and R are multiplied. sme: this lane's slab, sr: its row's slabs.
// Every lane of the workgroup calls this (two barriers inside).
template <int C, bool FIRST>
__device__ __forceinline__ void gated_layer(const float* __restrict__ Wl, const float* __restrict__ K,
                                            const float* __restrict__ R, const float* __restrict__ bias,
                                            gat_bits_t nb, float* sme, const float* sr, const float (&h)[C],
                                            float (&m)[C], float (&z)[C], float (&r)[C], float (&cc)[C],
                                            float (&gh)[C], float (&hn)[C]) {
  constexpr int KN = FIRST ? 4 : C;
  {
    float p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.f;
    gated_mv<C, KN>(h, Wl, C, p);
    __syncthreads();                                // the previous round's readers are done
    gated_put<C>(sme, p);
    __syncthreads();
  }
  gated_gather<C>(nb, sr, m);
  float s[C];
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = bias[c] + bias[3 * C + c];
  gated_mv<C, C>(m, K, 3 * C, s);
  gated_mv<C, KN>(h, R, 3 * C, s);
#pragma unroll
  for (int c = 0; c < C; ++c) z[c] = gated_sig(s[c]);
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = bias[C + c] + bias[4 * C + c];
  gated_mv<C, C>(m, K + C, 3 * C, s);
  gated_mv<C, KN>(h, R + C, 3 * C, s);
#pragma unroll
  for (int c = 0; c < C; ++c) r[c] = gated_sig(s[c]);
#pragma unroll
  for (int c = 0; c < C; ++c) gh[c] = bias[5 * C + c], s[c] = bias[2 * C + c];
  gated_mv<C, KN>(h, R + 2 * C, 3 * C, gh);
  gated_mv<C, C>(m, K + 2 * C, 3 * C, s);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    cc[c] = gated_tanh(s[c] + r[c] * gh[c]);
    hn[c] = z[c] * h[c] + (1.f - z[c]) * cc[c];
  }
}

// ------------------------------------------------------------------ forward
// out: Mp > 0: time-major LSTM input [T][Mp][Cp] (rows b >= B and channels >= Ca + C zero), else
// [B][T][Ca + C] (the host passes Cp = Ca + C then). pw [B][N]: node pool weights (mask included).
template <int C>
__global__ __launch_bounds__(256) void gated_pool_fwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const float* __restrict__ pw,
    const float* __restrict__ anom, const float* __restrict__ Wl, const float* __restrict__ K,
    const float* __restrict__ R, const float* __restrict__ bias, const float* __restrict__ alpha,
    float* __restrict__ out, int B, int T, int N, int NP, int Cin, int L, int Ca, int act, int Mp, int Cp) {
  using G = Gated<C>;
  __shared__ __align__(16) float sp[256 * G::PP];
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const int Fo = Ca + C;
  const long rows = (long)B * T;
  const long vrows = Mp > 0 ? (long)Mp * T : rows;        // virtual rows incl. zero padding rows
  float* sme = sp + tid * G::PP;
  const float* sr = sp + rl * NP * G::PP;
  for (long row0 = (long)blockIdx.x * rpw; row0 < vrows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const bool real = row < rows && i < N;
    float h[C];
#pragma unroll
    for (int c = 0; c < C; ++c) h[c] = 0.f;
    gat_bits_t nb = 0;
    float pwv = 0.f;
    if (real) {
      const long bn = (row / T) * N + i;
      nb = bits[bn] & (N == 64 ? ~0ull : (1ull << N) - 1);   // (a neighbour index stays inside the row's slabs)
      pwv = pw[bn];
#pragma unroll
      for (int f = 0; f < 4; ++f)
        if (f < Cin) h[f] = x[(row * N + i) * Cin + f];
    }
    for (int l = 0; l < L; ++l) {
      float m[C], z[C], r[C], cc[C], gh[C], hn[C];
      if (l == 0) gated_layer<C, true>(Wl, K, R, bias, nb, sme, sr, h, m, z, r, cc, gh, hn);
      else gated_layer<C, false>(Wl + l * C * C, K, R, bias, nb, sme, sr, h, m, z, r, cc, gh, hn);
#pragma unroll
      for (int c = 0; c < C; ++c) h[c] = hn[c];
    }
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = pwv * gat_act(h[c], act == GAT_ACT_PRELU ? alpha[c] : 0.f, act);
    // node pool: sum over the row's NP lanes (every lane of the wave takes part)
    for (int o = NP >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += __shfl_xor(acc[c], o, 64);
    }
    if (row >= vrows) continue;
    float* op = Mp > 0 ? out + ((row % T) * (long)Mp + row / T) * Cp : out + row * (long)Fo;
    if (row >= rows) {                            // (time-major only) padding row
      for (int c = i; c < Cp; c += NP) op[c] = 0.f;
      continue;
    }
    for (int c = i; c < Ca; c += NP) op[c] = anom[row * Ca + c];
#pragma unroll
    for (int c = 0; c < C; ++c)                   // (every lane of the row holds the sums)
      if ((c & (NP - 1)) == i) op[Ca + c] = acc[c];
    for (int c = Fo + i; c < Cp; c += NP) op[c] = 0.f;
  }
}

// ------------------------------------------------------------------ backward
// acc += this wave's share of the C x C slice X^T Y over the staged rows; X at column xcol. The four
// waves split the work so that the accumulators are a quarter of the slice set: at C = 32 wave w owns
// tile w of the 2 x 2 tiles over all 256 rows; at C <= 16 (one tile) it owns rows [64 w, 64 w + 64),
// and the four partial tiles are added in a fixed order when the record is written.
template <int C>
__device__ __forceinline__ void gated_outer(const float* sg, int xcol, gated_f4& acc) {
  using G = Gated<C>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lm = lane & 15, lq = lane >> 4;
  const int tile = wv % G::NT, grp = wv / G::NT;
  const float* rp = sg + (grp * G::GR + lq) * G::SP + lm;
  const int xo = xcol + 16 * (tile / G::TT), yo = 2 * G::CW + 16 * (tile % G::TT);
#pragma unroll 8
  for (int s = 0; s < G::GR / 4; ++s)
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(rp[4 * s * G::SP + xo], rp[4 * s * G::SP + yo], acc, 0, 0, 0);
}

// column c = lane of the staged Y slice summed over the wave's 64 rows (lanes >= C: 0)
template <int C>
__device__ __forceinline__ float gated_colsum(const float* sw) {
  using G = Gated<C>;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  if (lane < C) {
#pragma unroll 8
    for (int q = 0; q < 64; ++q) s += sw[q * G::SP + 2 * G::CW + lane];
  }
  return s;
}

// PARAMS: outp = partial [gridDim.x][REC], REC = L C C + 6 C C + 6 C + C (see the header);
// else outp = dx [B][T][N][Cin]. dout: [B][T][dstride], or time-major [T][dmp][dstride] when dmp > 0;
// the layer's channels start at c_off.
template <int C, bool PARAMS>
__global__ __launch_bounds__(256) void gated_pool_bwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const gat_bits_t* __restrict__ bitsT,
    const float* __restrict__ pw, const float* __restrict__ dout, const float* __restrict__ Wl,
    const float* __restrict__ K, const float* __restrict__ R, const float* __restrict__ bias,
    const float* __restrict__ alpha, float* __restrict__ outp, int B, int T, int N, int NP, int Cin, int L, int act,
    int c_off, int dstride, int dmp) {
  using G = Gated<C>;
  __shared__ __align__(16) float sp[256 * G::PP];
  __shared__ __align__(16) float sg[PARAMS ? 4 * 64 * G::SP : 4];
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const int lane = tid & 63, wv = tid >> 6;
  const long rows = (long)B * T;
  float* sme = sp + tid * G::PP;
  const float* sr = sp + rl * NP * G::PP;
  float* sw = sg + (PARAMS ? wv * 64 * G::SP : 0);
  float* swl = sw + (PARAMS ? lane * G::SP : 0);
  gated_f4 aK[3], aR[3], aW[GATED_MAX_L];          // this wave's share of the slices (gated_outer)
  float bs[4] = {0.f, 0.f, 0.f, 0.f}, as = 0.f;
#pragma unroll
  for (int g = 0; g < 3; ++g) aK[g] = aR[g] = gated_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < GATED_MAX_L; ++g) aW[g] = gated_f4{0.f, 0.f, 0.f, 0.f};
  for (long row0 = (long)blockIdx.x * rpw; row0 < rows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const bool real = row < rows && i < N;
    float x0[4] = {0.f, 0.f, 0.f, 0.f};
    gat_bits_t nb = 0, nbT = 0;
    float pwv = 0.f;
    if (real) {
      const long bn = (row / T) * N + i;
      const gat_bits_t valid = N == 64 ? ~0ull : (1ull << N) - 1;
      nb = bits[bn] & valid;
      nbT = bitsT[bn] & valid;
      pwv = pw[bn];
#pragma unroll
      for (int f = 0; f < 4; ++f)
        if (f < Cin) x0[f] = x[(row * N + i) * Cin + f];
    }
    float dh[C];
#pragma unroll
    for (int c = 0; c < C; ++c) dh[c] = 0.f;
    for (int l = L - 1; l >= 0; --l) {
      // h^l and layer l's intermediates, re-walked from h^0
      float hl[C], m[C], z[C], r[C], cc[C], gh[C], hn[C];
#pragma unroll
      for (int c = 0; c < C; ++c) hn[c] = c < 4 ? x0[c] : 0.f;
      for (int q = 0; q <= l; ++q) {
#pragma unroll
        for (int c = 0; c < C; ++c) hl[c] = hn[c];
        if (q == 0) gated_layer<C, true>(Wl, K, R, bias, nb, sme, sr, hl, m, z, r, cc, gh, hn);
        else gated_layer<C, false>(Wl + q * C * C, K, R, bias, nb, sme, sr, hl, m, z, r, cc, gh, hn);
      }
      if constexpr (PARAMS) {                         // (m is dead from here on)
        __syncthreads();
        gated_put<C>(swl, m);
        gated_put<C>(swl + G::CW, hl);
      }
      if (l == L - 1) {
        const long dro = dmp > 0 ? ((row % T) * (long)dmp + row / T) * dstride : row * (long)dstride;
        const bool live = real && pwv != 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float al = act == GAT_ACT_PRELU ? alpha[c] : 0.f;
          dh[c] = live ? gat_act_grad(hn[c], al, act) * pwv * dout[dro + c_off + c] : 0.f;
        }
        if constexpr (PARAMS) {
          if (act == GAT_ACT_PRELU) {                 // dalpha: the column sums of (h^L <= 0) h^L pw dout
            float ga[C];
#pragma unroll
            for (int c = 0; c < C; ++c) ga[c] = live && !(hn[c] > 0.f) ? hn[c] * pwv * dout[dro + c_off + c] : 0.f;
            gated_put<C>(swl + 2 * G::CW, ga);
            __syncthreads();
            as += gated_colsum<C>(sw);
            __syncthreads();
          }
        }
      }
      float dz[C], dr[C], dc[C], dcr[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        dc[c] = dh[c] * (1.f - z[c]) * (1.f - cc[c] * cc[c]);
        dz[c] = dh[c] * (hl[c] - cc[c]) * z[c] * (1.f - z[c]);
        dcr[c] = dc[c] * r[c];
        dr[c] = dc[c] * gh[c] * r[c] * (1.f - r[c]);
        dh[c] *= z[c];
      }
      if constexpr (PARAMS) {
        gated_put<C>(swl + 2 * G::CW, dz);
        __syncthreads();
        gated_outer<C>(sg, 0, aK[0]);
        gated_outer<C>(sg, G::CW, aR[0]);
        bs[0] += gated_colsum<C>(sw);
        __syncthreads();
        gated_put<C>(swl + 2 * G::CW, dr);
        __syncthreads();
        gated_outer<C>(sg, 0, aK[1]);
        gated_outer<C>(sg, G::CW, aR[1]);
        bs[1] += gated_colsum<C>(sw);
        __syncthreads();
        gated_put<C>(swl + 2 * G::CW, dc);
        __syncthreads();
        gated_outer<C>(sg, 0, aK[2]);
        bs[2] += gated_colsum<C>(sw);
        __syncthreads();
        gated_put<C>(swl + 2 * G::CW, dcr);
        __syncthreads();
        gated_outer<C>(sg, G::CW, aR[2]);
        bs[3] += gated_colsum<C>(sw);
      }
      // dm = da K^T into the slab; dh += dg R^T
      {
        float dm[C];
#pragma unroll
        for (int c = 0; c < C; ++c) dm[c] = 0.f;
        gated_mvT<C>(dz, K, 3 * C, dm);
        gated_mvT<C>(dr, K + C, 3 * C, dm);
        gated_mvT<C>(dc, K + 2 * C, 3 * C, dm);
        __syncthreads();                              // the layer's gather is done
        gated_put<C>(sme, dm);
        __syncthreads();
      }
      gated_mvT<C>(dz, R, 3 * C, dh);
      gated_mvT<C>(dr, R + C, 3 * C, dh);
      gated_mvT<C>(dcr, R + 2 * C, 3 * C, dh);
      // dp_j = sum over the nodes that have j as a neighbour: the transposed word
      float dp[C];
      gated_gather<C>(nbT, sr, dp);
      if constexpr (PARAMS) {
        __syncthreads();
        gated_put<C>(swl + 2 * G::CW, dp);
        __syncthreads();
        switch (l) {                                // (compile-time tile indices: registers)
          case 0: gated_outer<C>(sg, G::CW, aW[0]); break;
          case 1: gated_outer<C>(sg, G::CW, aW[1]); break;
          case 2: gated_outer<C>(sg, G::CW, aW[2]); break;
          default: gated_outer<C>(sg, G::CW, aW[3]); break;
        }
      }
      gated_mvT<C>(dp, Wl + l * C * C, C, dh);
    }
    if constexpr (!PARAMS) {
      if (real) {
#pragma unroll
        for (int f = 0; f < 4; ++f)
          if (f < Cin) outp[(row * N + i) * Cin + f] = dh[f];
      }
    }
  }
  if constexpr (PARAMS) {
    // the workgroup's record: the four waves' tiles in a fixed order
    const int lm = lane & 15, lq = lane >> 4;
    const int REC = L * C * C + 6 * C * C + 7 * C;
    float* rec = outp + (long)blockIdx.x * REC;
    auto flush = [&](const gated_f4& t, int off, int ld) {
      constexpr int WS = 64 * G::SP;
      const int tile = wv % G::NT, grp = wv / G::NT;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q)
        sg[grp * WS + (16 * (tile / G::TT) + 4 * lq + q) * G::CW + 16 * (tile % G::TT) + lm] = t[q];
      __syncthreads();
      for (int e = tid; e < C * C; e += 256) {
        const int k = e / C, c = e % C, idx = k * G::CW + c;
        float v = sg[idx];
#pragma unroll
        for (int g = 1; g < G::RG; ++g) v += sg[g * WS + idx];
        rec[off + k * ld + c] = v;
      }
    };
    if (L > 0) flush(aW[0], 0, C);
    if (L > 1) flush(aW[1], C * C, C);
    if (L > 2) flush(aW[2], 2 * C * C, C);
    if (L > 3) flush(aW[3], 3 * C * C, C);
    const int oK = L * C * C, oR = oK + 3 * C * C, oB = oR + 3 * C * C;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      flush(aK[g], oK + g * C, 3 * C);
      flush(aR[g], oR + g * C, 3 * C);
    }
    __syncthreads();
    if (lane < C) {
#pragma unroll
      for (int g = 0; g < 4; ++g) sw[g * C + lane] = bs[g];
      sw[4 * C + lane] = as;
    }
    __syncthreads();
    if (tid < 5 * C) {
      constexpr int WS = 64 * G::SP;
      const int g = tid / C, c = tid % C;
      const float v = (sg[tid] + sg[WS + tid]) + (sg[2 * WS + tid] + sg[3 * WS + tid]);
      if (g < 2) rec[oB + g * C + c] = rec[oB + 3 * C + g * C + c] = v;   // d(a_z) = d(g_z), d(a_r) = d(g_r)
      else if (g == 2) rec[oB + 2 * C + c] = v;
      else if (g == 3) rec[oB + 5 * C + c] = v;
      else rec[oB + 6 * C + c] = v;
    }
  }
}

// tot [REC]: the summed records. Adds each segment into its gradient buffer (nullptr: not needed); a
// non-finite value that goes into one raises the step's non-finite flag (chain control word 7), like
// the other gradient producers.
__global__ __launch_bounds__(256) void gated_bwd_finalize_kernel(const float* __restrict__ tot, int LCC, int CC3,
                                                                 int C, float* __restrict__ dW,
                                                                 float* __restrict__ dK, float* __restrict__ dR,
                                                                 float* __restrict__ dbias,
                                                                 float* __restrict__ dalpha, int* nf) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int o1 = LCC, o2 = o1 + CC3, o3 = o2 + CC3, o4 = o3 + 6 * C, o5 = o4 + C;
  if (e >= o5) return;
  float* dst = e < o1 ? (dW ? dW + e : nullptr)
             : e < o2 ? (dK ? dK + (e - o1) : nullptr)
             : e < o3 ? (dR ? dR + (e - o2) : nullptr)
             : e < o4 ? (dbias ? dbias + (e - o3) : nullptr)
                      : (dalpha ? dalpha + (e - o4) : nullptr);
  if (dst == nullptr) return;
  const float v = tot[e];
  *dst += v;
  if (!isfinite(v)) __hip_atomic_store(nf, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ instance table
#define GQ_GATED_DISPATCH(C_RT, ...)                         \
  switch (C_RT) {                                            \
    case 8: { constexpr int C = 8; __VA_ARGS__; } break;     \
    case 16: { constexpr int C = 16; __VA_ARGS__; } break;   \
    case 32: { constexpr int C = 32; __VA_ARGS__; } break;   \
    default: TORCH_CHECK(false, "gated: C in {8, 16, 32}");  \
  }

// ------------------------------------------------------------------ host
struct GatedDims {
  int B, T, N, Cin, NP, rpw, C, L;
};

// shapes shared by the kernels: x [B,T,N,Cin], bits [2,B,N], pw [B,N], Wl [L,C,C], K and R [C,3C],
// bias [2,3C], alpha [C] or empty
static GatedDims gated_check(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& Wl,
                             const at::Tensor& K, const at::Tensor& R, const at::Tensor& bias,
                             const at::Tensor& alpha, int64_t act) {
  for (auto* p : {&x, &pw, &Wl, &K, &R, &bias}) check_f32_cuda(*p, "gated input");
  TORCH_CHECK(x.dim() == 4, "gated: x must be [B,T,N,Cin]");
  TORCH_CHECK(Wl.dim() == 3 && Wl.size(1) == Wl.size(2), "gated: kernel must be [L,C,C]");
  GatedDims d;
  d.B = x.size(0), d.T = x.size(1), d.N = x.size(2), d.Cin = x.size(3);
  d.L = Wl.size(0), d.C = Wl.size(1);
  TORCH_CHECK(d.N >= 1 && d.N <= GATED_MAX_N, "gated: 1..64 nodes");
  TORCH_CHECK(d.C == 8 || d.C == 16 || d.C == 32, "gated: C in {8, 16, 32}");
  TORCH_CHECK(d.Cin >= 1 && d.Cin <= 4 && d.Cin <= d.C, "gated: Cin 1..4");
  TORCH_CHECK(d.L >= 1 && d.L <= GATED_MAX_L, "gated: 1..4 layers");
  TORCH_CHECK(bits.is_cuda() && bits.scalar_type() == at::kLong && bits.is_contiguous() &&
              bits.numel() == 2L * d.B * d.N, "gated: bits must be int64 [2,B,N]");
  TORCH_CHECK(pw.numel() == (long)d.B * d.N, "gated: pool weights must be [B,N]");
  TORCH_CHECK(K.numel() == 3L * d.C * d.C && R.numel() == 3L * d.C * d.C && bias.numel() == 6L * d.C,
              "gated: rnn kernels must be [C,3C], bias [2,3C]");
  TORCH_CHECK(act >= GAT_ACT_LINEAR && act <= GAT_ACT_RELU, "gated: activation code");
  if (act == GAT_ACT_PRELU) {
    check_f32_cuda(alpha, "alpha");
    TORCH_CHECK(alpha.numel() == d.C, "gated: alpha must be [C]");
  }
  d.NP = gat_pow2(d.N);
  d.rpw = 256 / d.NP;
  return d;
}

static int gated_grid(long rows, int rpw) {
  return (int)std::max<long>(1, std::min<long>((rows + rpw - 1) / rpw, GATED_GRID_CAP));
}

static const gat_bits_t* gated_bits_ptr(const at::Tensor& bits) {
  return reinterpret_cast<const gat_bits_t*>(bits.data_ptr<int64_t>());
}

at::Tensor gated_pool_fwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& anom,
                          const at::Tensor& Wl, const at::Tensor& K, const at::Tensor& R, const at::Tensor& bias,
                          const at::Tensor& alpha, int64_t act, int64_t Mp, int64_t Cp) {
  const GatedDims d = gated_check(x, bits, pw, Wl, K, R, bias, alpha, act);
  int Ca = 0;
  if (anom.numel() > 0) {
    check_f32_cuda(anom, "anom");
    TORCH_CHECK(anom.dim() == 3 && anom.size(0) == d.B && anom.size(1) == d.T, "gated: anom must be [B,T,Ca]");
    Ca = anom.size(2);
  }
  const int Fo = Ca + d.C;
  TORCH_CHECK(Mp == 0 || (Mp >= d.B && Mp % 16 == 0 && Cp >= Fo), "gated_pool_fwd: time-major Mp / Cp");
  c10::DeviceGuard guard(x.device());
  at::Tensor out = Mp > 0 ? at::empty({d.T, Mp, Cp}, x.options()) : at::empty({d.B, d.T, Fo}, x.options());
  const long vrows = Mp > 0 ? (long)Mp * d.T : (long)d.B * d.T;
  if (vrows == 0) return out;
  const float* anom_p = Ca ? anom.data_ptr<float>() : nullptr;
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  GQ_GATED_DISPATCH(d.C,
      hipLaunchKernelGGL((gated_pool_fwd_kernel<C>), dim3(gated_grid(vrows, d.rpw)), dim3(256), 0, stream(),
                         x.data_ptr<float>(), gated_bits_ptr(bits), pw.data_ptr<float>(), anom_p,
                         Wl.data_ptr<float>(), K.data_ptr<float>(), R.data_ptr<float>(), bias.data_ptr<float>(), al_p,
                         out.data_ptr<float>(), d.B, d.T, d.N, d.NP, d.Cin, d.L, Ca, (int)act, (int)Mp,
                         Mp > 0 ? (int)Cp : Fo));
  GQ_LAUNCH_CHECK();
  return out;
}

static void gated_check_dout(const at::Tensor& dout, const GatedDims& d, int64_t c_off, bool time_major) {
  check_f32_cuda(dout, "dout");
  TORCH_CHECK(dout.dim() == 3 && c_off >= 0 &&
              (time_major ? (dout.size(0) == d.T && dout.size(1) >= d.B && dout.size(2) >= c_off + d.C)
                          : (dout.size(0) == d.B && dout.size(1) == d.T && dout.size(2) >= c_off + d.C)),
              "gated: dout shape");
}

template <bool PARAMS>
static void gated_launch_bwd(const GatedDims& d, int nblk, const at::Tensor& x, const at::Tensor& bits,
                             const at::Tensor& pw, const at::Tensor& dout, const at::Tensor& Wl, const at::Tensor& K,
                             const at::Tensor& R, const at::Tensor& bias, const at::Tensor& alpha, int64_t act,
                             int64_t c_off, bool time_major, float* outp) {
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  const gat_bits_t* bp = gated_bits_ptr(bits);
  GQ_GATED_DISPATCH(d.C,
      hipLaunchKernelGGL((gated_pool_bwd_kernel<C, PARAMS>), dim3(nblk), dim3(256), 0, stream(), x.data_ptr<float>(),
                         bp, bp + (long)d.B * d.N, pw.data_ptr<float>(), dout.data_ptr<float>(), Wl.data_ptr<float>(),
                         K.data_ptr<float>(), R.data_ptr<float>(), bias.data_ptr<float>(), al_p, outp, d.B, d.T, d.N,
                         d.NP, d.Cin, d.L, (int)act, (int)c_off, (int)dout.size(2),
                         time_major ? (int)dout.size(1) : 0));
  GQ_LAUNCH_CHECK();
}

// the summed record [L C C + 6 C C + 7 C] of the parameter gradients (see gated_pool_bwd_kernel)
at::Tensor gated_pool_bwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& dout,
                          const at::Tensor& Wl, const at::Tensor& K, const at::Tensor& R, const at::Tensor& bias,
                          const at::Tensor& alpha, int64_t act, int64_t c_off, bool time_major) {
  const GatedDims d = gated_check(x, bits, pw, Wl, K, R, bias, alpha, act);
  gated_check_dout(dout, d, c_off, time_major);
  c10::DeviceGuard guard(x.device());
  const int REC = d.L * d.C * d.C + 6 * d.C * d.C + 7 * d.C;
  const long rows = (long)d.B * d.T;
  if (rows == 0) return at::zeros({REC}, x.options());
  const int nblk = gated_grid(rows, d.rpw);
  at::Tensor partial = at::empty({nblk, REC}, x.options());
  gated_launch_bwd<true>(d, nblk, x, bits, pw, dout, Wl, K, R, bias, alpha, act, c_off, time_major,
                         partial.data_ptr<float>());
  return nblk == 1 ? partial.view({REC}) : colsum(partial);          // fixed order: deterministic
}

static float* gated_sink(const at::Tensor& t, long n, const char* name) {
  if (t.numel() == 0) return nullptr;
  check_f32_cuda(t, name);
  TORCH_CHECK(t.numel() == n, "gated_bwd_finalize: ", name, " size");
  return t.data_ptr<float>();
}

void gated_bwd_finalize(const at::Tensor& tot, int64_t L, int64_t C, at::Tensor dW, at::Tensor dK, at::Tensor dR,
                        at::Tensor dbias, at::Tensor dalpha) {
  check_f32_cuda(tot, "tot");
  const long REC = L * C * C + 6 * C * C + 7 * C;
  TORCH_CHECK(tot.dim() == 1 && tot.numel() == REC, "gated_bwd_finalize: tot must be [L C C + 6 C C + 7 C]");
  c10::DeviceGuard guard(tot.device());
  hipLaunchKernelGGL(gated_bwd_finalize_kernel, dim3((int)((REC + 255) / 256)), dim3(256), 0, stream(),
                     tot.data_ptr<float>(), (int)(L * C * C), (int)(3 * C * C), (int)C, gated_sink(dW, L * C * C, "dW"),
                     gated_sink(dK, 3 * C * C, "dK"), gated_sink(dR, 3 * C * C, "dR"),
                     gated_sink(dbias, 6 * C, "dbias"), gated_sink(dalpha, C, "dalpha"),
                     chain_ctl(tot.get_device()) + 7);
  GQ_LAUNCH_CHECK();
}

at::Tensor gated_pool_bwd_input(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw,
                                const at::Tensor& dout, const at::Tensor& Wl, const at::Tensor& K,
                                const at::Tensor& R, const at::Tensor& bias, const at::Tensor& alpha, int64_t act,
                                int64_t c_off, bool time_major) {
  const GatedDims d = gated_check(x, bits, pw, Wl, K, R, bias, alpha, act);
  gated_check_dout(dout, d, c_off, time_major);
  c10::DeviceGuard guard(x.device());
  at::Tensor dx = at::empty_like(x);
  const long rows = (long)d.B * d.T;
  if (rows == 0) return dx;
  gated_launch_bwd<false>(d, gated_grid(rows, d.rpw), x, bits, pw, dout, Wl, K, R, bias, alpha, act, c_off,
                          time_major, dx.data_ptr<float>());
  return dx;
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("gated_pool_fwd", &gq::gated_pool_fwd);
  m.impl("gated_pool_bwd", &gq::gated_pool_bwd);
  m.impl("gated_bwd_finalize", &gq::gated_bwd_finalize);
  m.impl("gated_pool_bwd_input", &gq::gated_pool_bwd_input);
}
