// Fused GATConv + node pooling + concat for the CML front end.
//
// spektral GATConv(channels, attn_heads, concat_heads=True, add_self_loops=True) on a dense
// per-sample graph, followed by `timeseries_pooling` and Concatenate([flagged series, pooled])
// (gnnqc/models/graphconv.py GATConv is the eager form). With W [Cin, H, C] and the attention
// kernels a_s, a_n [C, H] the layer collapses into the Cin-dimensional input space:
//
//   s_self[i,h] = x_i . u_s[:,h]      u_s[f,h] = sum_c W[f,h,c] a_s[c,h]
//   s_nb[j,h]   = x_j . u_n[:,h]      u_n likewise
//   att[i,j,h]  = softmax_j over the neighbours of i of leaky_relu(s_self[i,h] + s_nb[j,h], 0.2)
//   out[i,h,:]  = act((sum_j att[i,j,h] x_j) W[:,h,:] + bias[h,:]) * mask_i
//
// so a node costs N scalar exp per head plus one Cin x C product, and the attention is never
// stored: the backward recomputes it from x. Mapping (all three kernels): one lane per
// (row = (b, t), node i); a row's NP = pow2 >= N lanes are adjacent lanes of one wave, so the
// node pool is a shuffle reduction; a lane walks the set bits of its node's 64-bit neighbour mask
// (gat_adj_bits, once per batch) over the row's x and s_nb in LDS. Hence N <= 64.
//
// The backward (gat_pool_bwd) keeps every parameter gradient of a workgroup in registers over its
// passes and writes ONE record per (workgroup, head): [dW (Cin x C) | dbias | dalpha | du_s | du_n];
// a fixed-order column sum and gat_bwd_finalize (the u_s / u_n fold into dW, da_s, da_n) follow.
// No float atomics anywhere: results are bitwise reproducible.
#include "gat_common.h"

namespace gq {

constexpr int GAT_MAX_N = 64;
constexpr int GAT_GRID_CAP = 256;        // workgroups per launch: more rows take several passes

// bits[0][b][i]: neighbours j of node i ((adj + I * mask) > 0); bits[1][b][i]: nodes that have i
// as a neighbour (the transposed mask, for the input gradient)
__global__ void gat_adj_bits_kernel(const float* __restrict__ adj, const float* __restrict__ mask,
                                    gat_bits_t* __restrict__ bits, int B, int N) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= (long)B * N) return;
  const int b = (int)(e / N), i = (int)(e % N);
  const float* a = adj + (long)b * N * N;
  gat_bits_t r = 0, c = 0;
  for (int j = 0; j < N; ++j) {
    if (a[i * N + j] > 0.f) r |= 1ull << j;
    if (a[j * N + i] > 0.f) c |= 1ull << j;
  }
  if (mask[e] > 0.f) {
    r |= 1ull << i;
    c |= 1ull << i;
  }
  bits[e] = r;
  bits[(long)B * N + e] = c;
}

// Masked edge softmax of one (node, head) and its input-space aggregate: m = max_j e_j,
// inv = 1 / sum_j exp(e_j - m) (0 for a node without neighbours: the aggregate is then zero, as
// in the eager layer), z[f] = sum_j att_j x_j[f]. The aggregate is formed around the node's own
// features, z = x_i + zc with zc = sum_j att_j (x_j - x_i) (sum_j att_j = 1): neighbourhoods of
// similar series lose no digits to the cancellation, and where all x_j are equal zc and the
// softmax's gradient are exactly zero. xi: x_i; xr / nr: the row's x [NP][CIN] and s_nb [NP][hs]
// (this head's column) in LDS.
template <int CIN>
__device__ __forceinline__ void gat_attend(gat_bits_t nb, float ss, const float (&xi)[CIN], const float* xr,
                                           const float* nr, int hs, float& m, float& inv, float (&zc)[CIN],
                                           float (&z)[CIN]) {
  m = -3.0e38f;
  for (gat_bits_t w = nb; w; w &= w - 1) {
    const int j = __ffsll((long long)w) - 1;
    m = fmaxf(m, gat_leaky(ss + nr[j * hs]));
  }
  float den = 0.f;
#pragma unroll
  for (int f = 0; f < CIN; ++f) zc[f] = 0.f;
  for (gat_bits_t w = nb; w; w &= w - 1) {
    const int j = __ffsll((long long)w) - 1;
    const float p = __expf(gat_leaky(ss + nr[j * hs]) - m);
    den += p;
#pragma unroll
    for (int f = 0; f < CIN; ++f) zc[f] += p * (xr[j * CIN + f] - xi[f]);
  }
  inv = den > 0.f ? 1.f / den : 0.f;
#pragma unroll
  for (int f = 0; f < CIN; ++f) {
    zc[f] *= inv;
    z[f] = den > 0.f ? xi[f] + zc[f] : 0.f;
  }
}

// ------------------------------------------------------------------ forward
// out: Mp > 0: time-major LSTM input [T][Mp][Cp] (rows b >= B and channels >= Ca + H*C zero),
// else [B][T][Ca + H*C] (the host passes Cp = Ca + H*C then). pw [B][N]: node pool weights
// (mask included: a masked node has weight 0).
template <int CIN, int C, int H>
__global__ __launch_bounds__(256) void gat_pool_fwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const float* __restrict__ pw,
    const float* __restrict__ anom, const float* __restrict__ W, const float* __restrict__ as,
    const float* __restrict__ an, const float* __restrict__ bias, const float* __restrict__ alpha,
    float* __restrict__ out, int B, int T, int N, int NP, int Ca, int act, int Mp, int Cp) {
  using P = GatParams<CIN, C, H>;
  constexpr int HC = H * C;
  __shared__ float sp[P::SIZE];
  __shared__ float sx[256 * CIN];
  __shared__ float snb[256 * H];
  P prm{sp};
  prm.load(W, as, an, bias, alpha);
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const int Fo = Ca + HC;
  const long rows = (long)B * T;
  const long vrows = Mp > 0 ? (long)Mp * T : rows;        // virtual rows incl. zero padding rows
  for (long row0 = (long)blockIdx.x * rpw; row0 < vrows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const bool real = row < rows && i < N;
    float xi[CIN], p = 0.f;
    gat_bits_t nb = 0;
#pragma unroll
    for (int f = 0; f < CIN; ++f) xi[f] = 0.f;
    if (real) {
      const long bn = (row / T) * N + i;
      p = pw[bn];
      nb = bits[bn];
#pragma unroll
      for (int f = 0; f < CIN; ++f) xi[f] = x[(row * N + i) * CIN + f];
    }
    float ss[H];
    __syncthreads();                              // the previous pass's readers are done
#pragma unroll
    for (int f = 0; f < CIN; ++f) sx[tid * CIN + f] = xi[f];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float s = 0.f, n = 0.f;
#pragma unroll
      for (int f = 0; f < CIN; ++f) {
        s += xi[f] * prm.us(f, h);
        n += xi[f] * prm.un(f, h);
      }
      ss[h] = s;
      snb[tid * H + h] = n;
    }
    __syncthreads();
    float acc[HC];
#pragma unroll
    for (int k = 0; k < HC; ++k) acc[k] = 0.f;
    if (real && p != 0.f) {
      const float* xr = sx + rl * NP * CIN;
      const float* nr = snb + rl * NP * H;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float m, inv, zc[CIN], z[CIN];
        gat_attend<CIN>(nb, ss[h], xi, xr, nr + h, H, m, inv, zc, z);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          float o = prm.bias(h * C + c);
#pragma unroll
          for (int f = 0; f < CIN; ++f) o += z[f] * prm.W(f, h, c);
          acc[h * C + c] = p * gat_act(o, prm.alpha(h * C + c), act);
        }
      }
    }
    // node pool: sum over the row's NP lanes (every lane of the wave takes part)
    for (int o = NP >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < HC; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    if (row >= vrows) continue;
    float* op = Mp > 0 ? out + ((row % T) * (long)Mp + row / T) * Cp : out + row * (long)Fo;
    if (row >= rows) {                            // (time-major only) padding row
      for (int c = i; c < Cp; c += NP) op[c] = 0.f;
      continue;
    }
    for (int c = i; c < Ca; c += NP) op[c] = anom[row * Ca + c];
#pragma unroll
    for (int k = 0; k < HC; ++k)
      if ((k & (NP - 1)) == i) op[Ca + k] = acc[k];
    for (int c = Fo + i; c < Cp; c += NP) op[c] = 0.f;
  }
}

// ------------------------------------------------------------------ backward, shared part
// One (node i, head h) of the backward up to the aggregate's gradient: recomputes the softmax
// (m, inv, zc, z), the head's output o, and from g[c] = pool weight * upstream gradient gives
// dout[c] = dL/d(z W + bias)[c] and dz[f] = dL/dz[f]. nrh / hs: this head's s_nb column in LDS
// and its stride.
template <int CIN, int C, int H>
__device__ __forceinline__ void gat_head_bwd(const GatParams<CIN, C, H>& prm, int h, gat_bits_t nb, float ss,
                                             const float (&xi)[CIN], const float* xr, const float* nrh, int hs,
                                             const float (&g)[C], int act, float& m, float& inv, float (&zc)[CIN],
                                             float (&z)[CIN], float (&o)[C], float (&dout)[C], float (&dz)[CIN]) {
  gat_attend<CIN>(nb, ss, xi, xr, nrh, hs, m, inv, zc, z);
#pragma unroll
  for (int f = 0; f < CIN; ++f) dz[f] = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float v = prm.bias(h * C + c);
#pragma unroll
    for (int f = 0; f < CIN; ++f) v += z[f] * prm.W(f, h, c);
    o[c] = v;
    dout[c] = g[c] * gat_act_grad(v, prm.alpha(h * C + c), act);
#pragma unroll
    for (int f = 0; f < CIN; ++f) dz[f] += prm.W(f, h, c) * dout[c];
  }
}

// ------------------------------------------------------------------ backward (parameters)
// grid (workgroups, H): workgroup (k, h) handles head h of its rows. partial [gridDim.x][H][R],
// R = CIN*C + 2C + 2CIN: dW[f][c] | dbias[c] | dalpha[c] | du_s[f] | du_n[f].
// dout: [B][T][dstride], or time-major [T][dmp][dstride] when dmp > 0; the layer's channels
// start at c_off.
template <int CIN, int C, int H>
__global__ __launch_bounds__(256) void gat_pool_bwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const float* __restrict__ pw,
    const float* __restrict__ dout, const float* __restrict__ W, const float* __restrict__ as,
    const float* __restrict__ an, const float* __restrict__ bias, const float* __restrict__ alpha,
    float* __restrict__ partial, int B, int T, int N, int NP, int act, int c_off, int dstride, int dmp) {
  using P = GatParams<CIN, C, H>;
  constexpr int R = CIN * C + 2 * C + 2 * CIN;
  __shared__ float sp[P::SIZE];
  __shared__ float sx[256 * CIN];
  __shared__ float snb[256];
  __shared__ float red[4][R];
  P prm{sp};
  prm.load(W, as, an, bias, alpha);
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const int h = blockIdx.y;
  const long rows = (long)B * T;
  float aW[CIN][C], ab[C], aal[C], aus[CIN], aun[CIN];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    ab[c] = aal[c] = 0.f;
#pragma unroll
    for (int f = 0; f < CIN; ++f) aW[f][c] = 0.f;
  }
#pragma unroll
  for (int f = 0; f < CIN; ++f) aus[f] = aun[f] = 0.f;
  for (long row0 = (long)blockIdx.x * rpw; row0 < rows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const bool real = row < rows && i < N;
    float xi[CIN], p = 0.f;
    gat_bits_t nb = 0;
#pragma unroll
    for (int f = 0; f < CIN; ++f) xi[f] = 0.f;
    if (real) {
      const long bn = (row / T) * N + i;
      p = pw[bn];
      nb = bits[bn];
#pragma unroll
      for (int f = 0; f < CIN; ++f) xi[f] = x[(row * N + i) * CIN + f];
    }
    float ss = 0.f, sn = 0.f;
#pragma unroll
    for (int f = 0; f < CIN; ++f) {
      ss += xi[f] * prm.us(f, h);
      sn += xi[f] * prm.un(f, h);
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < CIN; ++f) sx[tid * CIN + f] = xi[f];
    snb[tid] = sn;
    __syncthreads();
    if (!(real && p != 0.f)) continue;            // (no barrier or shuffle below in the loop)
    const float* xr = sx + rl * NP * CIN;
    const float* nr = snb + rl * NP;
    const long dro = dmp > 0 ? ((row % T) * (long)dmp + row / T) * dstride : row * (long)dstride;
    float g[C], o[C], dO[C], zc[CIN], z[CIN], dz[CIN], m, inv;
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = p * dout[dro + c_off + h * C + c];
    // (s_nb has stride 1 here: one head per workgroup)
    gat_head_bwd<CIN, C, H>(prm, h, nb, ss, xi, xr, nr, 1, g, act, m, inv, zc, z, o, dO, dz);
    float dzc = 0.f;
#pragma unroll
    for (int f = 0; f < CIN; ++f) dzc += dz[f] * zc[f];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      ab[c] += dO[c];
      if (act == GAT_ACT_PRELU) aal[c] += o[c] > 0.f ? 0.f : g[c] * o[c];
#pragma unroll
      for (int f = 0; f < CIN; ++f) aW[f][c] += z[f] * dO[c];
    }
    // softmax backward: ds_j = att_j (dz . (x_j - x_i) - dz . zc) leaky'(s_self + s_nb_j)
    float sds = 0.f;
    for (gat_bits_t w = nb; w; w &= w - 1) {
      const int j = __ffsll((long long)w) - 1;
      const float e = ss + nr[j];
      const float att = __expf(gat_leaky(e) - m) * inv;
      float da = -dzc;
#pragma unroll
      for (int f = 0; f < CIN; ++f) da += dz[f] * (xr[j * CIN + f] - xi[f]);
      const float ds = att * da * (e > 0.f ? 1.f : GAT_SLOPE);
      sds += ds;
#pragma unroll
      for (int f = 0; f < CIN; ++f) aun[f] += ds * xr[j * CIN + f];
    }
#pragma unroll
    for (int f = 0; f < CIN; ++f) aus[f] += sds * xi[f];
  }
  // the workgroup's record: wave sums by shuffles, then the 4 wave partials in order
  const int lane = tid & 63, wv = tid >> 6;
  auto put = [&](int e, float v) {
    v = wave_sum(v);
    if (lane == 0) red[wv][e] = v;
  };
#pragma unroll
  for (int f = 0; f < CIN; ++f) {
#pragma unroll
    for (int c = 0; c < C; ++c) put(f * C + c, aW[f][c]);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    put(CIN * C + c, ab[c]);
    put(CIN * C + C + c, aal[c]);
  }
#pragma unroll
  for (int f = 0; f < CIN; ++f) {
    put(CIN * C + 2 * C + f, aus[f]);
    put(CIN * C + 2 * C + CIN + f, aun[f]);
  }
  __syncthreads();
  for (int e = tid; e < R; e += blockDim.x)
    partial[((long)blockIdx.x * H + h) * R + e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

// tot [H][R]: the summed records. Adds dW[f,h,c] = tot dW + du_s[f,h] a_s[c,h] + du_n[f,h] a_n[c,h],
// da_s[c,h] = sum_f W[f,h,c] du_s[f,h] (da_n likewise), dbias, dalpha into the gradient buffers
// (nullptr: not needed).
__global__ __launch_bounds__(256) void gat_bwd_finalize_kernel(
    const float* __restrict__ tot, const float* __restrict__ W, const float* __restrict__ as,
    const float* __restrict__ an, int CIN, int C, int H, float* __restrict__ dW, float* __restrict__ das,
    float* __restrict__ dan, float* __restrict__ dbias, float* __restrict__ dalpha) {
  const int R = CIN * C + 2 * C + 2 * CIN;
  const int oU = CIN * C + 2 * C;
  for (int e = threadIdx.x; e < CIN * H * C; e += blockDim.x) {
    const int c = e % C, h = (e / C) % H, f = e / (C * H);
    const float* t = tot + h * R;
    if (dW) dW[e] += t[f * C + c] + t[oU + f] * as[c * H + h] + t[oU + CIN + f] * an[c * H + h];
  }
  for (int e = threadIdx.x; e < C * H; e += blockDim.x) {
    const int h = e % H, c = e / H;
    const float* t = tot + h * R;
    float s = 0.f, n = 0.f;
    for (int f = 0; f < CIN; ++f) {
      const float w = W[(f * H + h) * C + c];
      s += w * t[oU + f];
      n += w * t[oU + CIN + f];
    }
    if (das) das[e] += s;
    if (dan) dan[e] += n;
  }
  for (int e = threadIdx.x; e < H * C; e += blockDim.x) {
    const int c = e % C, h = e / C;
    const float* t = tot + h * R;
    if (dbias) dbias[e] += t[CIN * C + c];
    if (dalpha) dalpha[e] += t[CIN * C + C + c];
  }
}

// ------------------------------------------------------------------ backward (input)
// Phase 1, lane (row, i): the softmax state of node i and dL/dz_i per head, parked in LDS, and
// the s_self part of dx_i. Phase 2, lane (row, j): gathers over the nodes i that have j as a
// neighbour (transposed mask): dx_j += att_ij dz_i + ds_ij u_n. Every dx element is written by
// exactly one lane: no atomics.
template <int CIN, int C, int H>
__global__ __launch_bounds__(256) void gat_pool_bwd_input_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const gat_bits_t* __restrict__ bitsT,
    const float* __restrict__ pw, const float* __restrict__ dout, const float* __restrict__ W,
    const float* __restrict__ as, const float* __restrict__ an, const float* __restrict__ bias,
    const float* __restrict__ alpha, float* __restrict__ dx, int B, int T, int N, int NP, int act, int c_off,
    int dstride, int dmp) {
  using P = GatParams<CIN, C, H>;
  __shared__ float sp[P::SIZE];
  __shared__ float sx[256 * CIN];
  __shared__ float snb[256 * H];
  __shared__ float sdz[256 * H * CIN];
  __shared__ float sst[256 * H * 4];            // s_self, m, inv, dz . zc
  P prm{sp};
  prm.load(W, as, an, bias, alpha);
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const long rows = (long)B * T;
  for (long row0 = (long)blockIdx.x * rpw; row0 < rows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const bool real = row < rows && i < N;
    float xi[CIN], p = 0.f;
    gat_bits_t nb = 0, nbT = 0;
#pragma unroll
    for (int f = 0; f < CIN; ++f) xi[f] = 0.f;
    if (real) {
      const long bn = (row / T) * N + i;
      p = pw[bn];
      nb = bits[bn];
      nbT = bitsT[bn];
#pragma unroll
      for (int f = 0; f < CIN; ++f) xi[f] = x[(row * N + i) * CIN + f];
    }
    float ss[H], sn[H];
    __syncthreads();
#pragma unroll
    for (int f = 0; f < CIN; ++f) sx[tid * CIN + f] = xi[f];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float s = 0.f, n = 0.f;
#pragma unroll
      for (int f = 0; f < CIN; ++f) {
        s += xi[f] * prm.us(f, h);
        n += xi[f] * prm.un(f, h);
      }
      ss[h] = s;
      sn[h] = n;
      snb[tid * H + h] = n;
    }
    __syncthreads();
    const float* xr = sx + rl * NP * CIN;
    const float* nr = snb + rl * NP * H;
    float dxi[CIN];
#pragma unroll
    for (int f = 0; f < CIN; ++f) dxi[f] = 0.f;
    const bool on = real && p != 0.f;
    const long dro = dmp > 0 ? ((row % T) * (long)dmp + row / T) * dstride : row * (long)dstride;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float m = 0.f, inv = 0.f, dzc = 0.f, dz[CIN];
#pragma unroll
      for (int f = 0; f < CIN; ++f) dz[f] = 0.f;
      if (on) {
        float g[C], o[C], dO[C], zc[CIN], z[CIN];
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = p * dout[dro + c_off + h * C + c];
        gat_head_bwd<CIN, C, H>(prm, h, nb, ss[h], xi, xr, nr + h, H, g, act, m, inv, zc, z, o, dO, dz);
#pragma unroll
        for (int f = 0; f < CIN; ++f) dzc += dz[f] * zc[f];
        float sds = 0.f;
        for (gat_bits_t w = nb; w; w &= w - 1) {
          const int j = __ffsll((long long)w) - 1;
          const float e = ss[h] + nr[j * H + h];
          const float att = __expf(gat_leaky(e) - m) * inv;
          float da = -dzc;
#pragma unroll
          for (int f = 0; f < CIN; ++f) da += dz[f] * (xr[j * CIN + f] - xi[f]);
          sds += att * da * (e > 0.f ? 1.f : GAT_SLOPE);
        }
#pragma unroll
        for (int f = 0; f < CIN; ++f) dxi[f] += sds * prm.us(f, h);
      }
      float* st = sst + (tid * H + h) * 4;
      st[0] = ss[h];
      st[1] = m;
      st[2] = inv;                                // 0: node i contributes nothing
      st[3] = dzc;
#pragma unroll
      for (int f = 0; f < CIN; ++f) sdz[(tid * H + h) * CIN + f] = dz[f];
    }
    __syncthreads();
    if (!real) continue;                          // (no barrier or shuffle below in the loop)
    for (gat_bits_t w = nbT; w; w &= w - 1) {
      const int k = __ffsll((long long)w) - 1;    // node k attends to this lane's node
      const int lk = rl * NP + k;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float* st = sst + (lk * H + h) * 4;
        const float inv = st[2];
        if (inv == 0.f) continue;
        const float e = st[0] + sn[h];
        const float att = __expf(gat_leaky(e) - st[1]) * inv;
        const float* dzk = sdz + (lk * H + h) * CIN;
        float da = -st[3];                    // dz_k . (x_j - x_k) - dz_k . zc_k
#pragma unroll
        for (int f = 0; f < CIN; ++f) da += dzk[f] * (xi[f] - sx[lk * CIN + f]);
        const float ds = att * da * (e > 0.f ? 1.f : GAT_SLOPE);
#pragma unroll
        for (int f = 0; f < CIN; ++f) dxi[f] += att * dzk[f] + ds * prm.un(f, h);
      }
    }
#pragma unroll
    for (int f = 0; f < CIN; ++f) dx[(row * N + i) * CIN + f] = dxi[f];
  }
}

// ------------------------------------------------------------------ host
struct GatDims {
  int B, T, N, Cin, C, H, NP, rpw;
};

// shapes shared by the three kernels: x [B,T,N,Cin], bits [2,B,N], pw [B,N], W [Cin,H,C],
// a_s / a_n [C,H(,1)], bias [H*C], alpha [H*C] or empty
static GatDims gat_check(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& W,
                         const at::Tensor& as, const at::Tensor& an, const at::Tensor& bias,
                         const at::Tensor& alpha, int64_t act) {
  for (auto* p : {&x, &pw, &W, &as, &an, &bias}) check_f32_cuda(*p, "gat input");
  TORCH_CHECK(x.dim() == 4 && W.dim() == 3, "gat: x must be [B,T,N,Cin], W [Cin,H,C]");
  GatDims d;
  d.B = x.size(0), d.T = x.size(1), d.N = x.size(2), d.Cin = x.size(3), d.H = W.size(1), d.C = W.size(2);
  TORCH_CHECK(d.N >= 1 && d.N <= GAT_MAX_N, "gat: 1..64 nodes");
  TORCH_CHECK(W.size(0) == d.Cin, "gat: W must be [Cin,H,C]");
  TORCH_CHECK(bits.is_cuda() && bits.scalar_type() == at::kLong && bits.is_contiguous() &&
              bits.numel() == 2L * d.B * d.N, "gat: bits must be int64 [2,B,N]");
  TORCH_CHECK(pw.numel() == (long)d.B * d.N, "gat: pool weights must be [B,N]");
  TORCH_CHECK(as.numel() == d.C * d.H && an.numel() == d.C * d.H, "gat: attention kernels must be [C,H]");
  TORCH_CHECK(bias.numel() == d.H * d.C, "gat: bias must be [H*C]");
  TORCH_CHECK(act >= GAT_ACT_LINEAR && act <= GAT_ACT_RELU, "gat: activation code");
  if (act == GAT_ACT_PRELU) {
    check_f32_cuda(alpha, "alpha");
    TORCH_CHECK(alpha.numel() == d.H * d.C, "gat: alpha must be [H*C]");
  }
  d.NP = gat_pow2(d.N);
  d.rpw = 256 / d.NP;
  return d;
}

static int gat_grid(long rows, int rpw) {
  return (int)std::max<long>(1, std::min<long>((rows + rpw - 1) / rpw, GAT_GRID_CAP));
}

static const gat_bits_t* gat_bits_ptr(const at::Tensor& bits) {
  return reinterpret_cast<const gat_bits_t*>(bits.data_ptr<int64_t>());
}

at::Tensor gat_adj_bits(const at::Tensor& adj, const at::Tensor& mask) {
  check_f32_cuda(adj, "adj");
  check_f32_cuda(mask, "mask");
  TORCH_CHECK(adj.dim() == 3 && adj.size(1) == adj.size(2), "gat: adj must be [B,N,N]");
  const int B = adj.size(0), N = adj.size(1);
  TORCH_CHECK(N >= 1 && N <= GAT_MAX_N, "gat: 1..64 nodes");
  TORCH_CHECK(mask.dim() == 2 && mask.size(0) == B && mask.size(1) == N, "gat: mask must be [B,N]");
  c10::DeviceGuard guard(adj.device());
  at::Tensor bits = at::empty({2, B, N}, adj.options().dtype(at::kLong));
  if (B == 0) return bits;
  hipLaunchKernelGGL(gat_adj_bits_kernel, dim3(((long)B * N + 255) / 256), dim3(256), 0, stream(),
                     adj.data_ptr<float>(), mask.data_ptr<float>(),
                     reinterpret_cast<gat_bits_t*>(bits.data_ptr<int64_t>()), B, N);
  GQ_LAUNCH_CHECK();
  return bits;
}

at::Tensor gat_pool_fwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& anom,
                        const at::Tensor& W, const at::Tensor& as, const at::Tensor& an, const at::Tensor& bias,
                        const at::Tensor& alpha, int64_t act, int64_t Mp, int64_t Cp) {
  const GatDims d = gat_check(x, bits, pw, W, as, an, bias, alpha, act);
  int Ca = 0;
  if (anom.numel() > 0) {
    check_f32_cuda(anom, "anom");
    TORCH_CHECK(anom.dim() == 3 && anom.size(0) == d.B && anom.size(1) == d.T, "gat: anom must be [B,T,Ca]");
    Ca = anom.size(2);
  }
  const int Fo = Ca + d.H * d.C;
  TORCH_CHECK(Mp == 0 || (Mp >= d.B && Mp % 16 == 0 && Cp >= Fo), "gat_pool_fwd: time-major Mp / Cp");
  c10::DeviceGuard guard(x.device());
  at::Tensor out = Mp > 0 ? at::empty({d.T, Mp, Cp}, x.options()) : at::empty({d.B, d.T, Fo}, x.options());
  const long vrows = Mp > 0 ? (long)Mp * d.T : (long)d.B * d.T;
  if (vrows == 0) return out;
  const float* anom_p = Ca ? anom.data_ptr<float>() : nullptr;
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  GQ_GAT_DISPATCH(d.Cin, d.C, d.H,
      hipLaunchKernelGGL((gat_pool_fwd_kernel<CIN, C, H>), dim3(gat_grid(vrows, d.rpw)), dim3(256), 0, stream(),
                         x.data_ptr<float>(), gat_bits_ptr(bits), pw.data_ptr<float>(), anom_p, W.data_ptr<float>(),
                         as.data_ptr<float>(), an.data_ptr<float>(), bias.data_ptr<float>(), al_p,
                         out.data_ptr<float>(), d.B, d.T, d.N, d.NP, Ca, (int)act, (int)Mp,
                         Mp > 0 ? (int)Cp : Fo));
  GQ_LAUNCH_CHECK();
  return out;
}

static void gat_check_dout(const at::Tensor& dout, const GatDims& d, int64_t c_off, bool time_major) {
  check_f32_cuda(dout, "dout");
  const int HC = d.H * d.C;
  TORCH_CHECK(dout.dim() == 3 && c_off >= 0 &&
              (time_major ? (dout.size(0) == d.T && dout.size(1) >= d.B && dout.size(2) >= c_off + HC)
                          : (dout.size(0) == d.B && dout.size(1) == d.T && dout.size(2) >= c_off + HC)),
              "gat: dout shape");
}

// the summed records [H, R] of the parameter gradients (see gat_pool_bwd_kernel)
at::Tensor gat_pool_bwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& dout,
                        const at::Tensor& W, const at::Tensor& as, const at::Tensor& an, const at::Tensor& bias,
                        const at::Tensor& alpha, int64_t act, int64_t c_off, bool time_major) {
  const GatDims d = gat_check(x, bits, pw, W, as, an, bias, alpha, act);
  gat_check_dout(dout, d, c_off, time_major);
  c10::DeviceGuard guard(x.device());
  const int R = d.Cin * d.C + 2 * d.C + 2 * d.Cin;
  const long rows = (long)d.B * d.T;
  if (rows == 0) return at::zeros({d.H, R}, x.options());
  const int nblk = gat_grid(rows, d.rpw);
  at::Tensor partial = at::empty({nblk, d.H, R}, x.options());
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  GQ_GAT_DISPATCH(d.Cin, d.C, d.H,
      hipLaunchKernelGGL((gat_pool_bwd_kernel<CIN, C, H>), dim3(nblk, d.H), dim3(256), 0, stream(),
                         x.data_ptr<float>(), gat_bits_ptr(bits), pw.data_ptr<float>(), dout.data_ptr<float>(),
                         W.data_ptr<float>(), as.data_ptr<float>(), an.data_ptr<float>(), bias.data_ptr<float>(),
                         al_p, partial.data_ptr<float>(), d.B, d.T, d.N, d.NP, (int)act, (int)c_off,
                         (int)dout.size(2), time_major ? (int)dout.size(1) : 0));
  GQ_LAUNCH_CHECK();
  return nblk == 1 ? partial.view({d.H, R}) : colsum(partial);       // fixed order: deterministic
}

static float* gat_sink(const at::Tensor& t, long n, const char* name) {
  if (t.numel() == 0) return nullptr;
  check_f32_cuda(t, name);
  TORCH_CHECK(t.numel() == n, "gat_bwd_finalize: ", name, " size");
  return t.data_ptr<float>();
}

void gat_bwd_finalize(const at::Tensor& tot, const at::Tensor& W, const at::Tensor& as, const at::Tensor& an,
                      at::Tensor dW, at::Tensor das, at::Tensor dan, at::Tensor dbias, at::Tensor dalpha) {
  for (auto* p : {&tot, &W, &as, &an}) check_f32_cuda(*p, "gat finalize input");
  TORCH_CHECK(W.dim() == 3, "gat: W must be [Cin,H,C]");
  const int Cin = W.size(0), H = W.size(1), C = W.size(2);
  const int R = Cin * C + 2 * C + 2 * Cin;
  TORCH_CHECK(tot.numel() == (long)H * R, "gat_bwd_finalize: tot must be [H,R]");
  TORCH_CHECK(as.numel() == C * H && an.numel() == C * H, "gat: attention kernels must be [C,H]");
  c10::DeviceGuard guard(W.device());
  hipLaunchKernelGGL(gat_bwd_finalize_kernel, dim3(1), dim3(256), 0, stream(), tot.data_ptr<float>(),
                     W.data_ptr<float>(), as.data_ptr<float>(), an.data_ptr<float>(), Cin, C, H,
                     gat_sink(dW, (long)Cin * H * C, "dW"), gat_sink(das, C * H, "da_s"), gat_sink(dan, C * H, "da_n"),
                     gat_sink(dbias, H * C, "dbias"), gat_sink(dalpha, H * C, "dalpha"));
  GQ_LAUNCH_CHECK();
}

at::Tensor gat_pool_bwd_input(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw,
                              const at::Tensor& dout, const at::Tensor& W, const at::Tensor& as,
                              const at::Tensor& an, const at::Tensor& bias, const at::Tensor& alpha, int64_t act,
                              int64_t c_off, bool time_major) {
  const GatDims d = gat_check(x, bits, pw, W, as, an, bias, alpha, act);
  gat_check_dout(dout, d, c_off, time_major);
  c10::DeviceGuard guard(x.device());
  at::Tensor dx = at::empty_like(x);
  const long rows = (long)d.B * d.T;
  if (rows == 0) return dx;
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  const gat_bits_t* bp = gat_bits_ptr(bits);
  GQ_GAT_DISPATCH(d.Cin, d.C, d.H,
      hipLaunchKernelGGL((gat_pool_bwd_input_kernel<CIN, C, H>), dim3(gat_grid(rows, d.rpw)), dim3(256), 0, stream(),
                         x.data_ptr<float>(), bp, bp + (long)d.B * d.N, pw.data_ptr<float>(), dout.data_ptr<float>(),
                         W.data_ptr<float>(), as.data_ptr<float>(), an.data_ptr<float>(), bias.data_ptr<float>(),
                         al_p, dx.data_ptr<float>(), d.B, d.T, d.N, d.NP, (int)act, (int)c_off, (int)dout.size(2),
                         time_major ? (int)dout.size(1) : 0));
  GQ_LAUNCH_CHECK();
  return dx;
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("gat_adj_bits", &gq::gat_adj_bits);
  m.impl("gat_pool_fwd", &gq::gat_pool_fwd);
  m.impl("gat_pool_bwd", &gq::gat_pool_bwd);
  m.impl("gat_bwd_finalize", &gq::gat_bwd_finalize);
  m.impl("gat_pool_bwd_input", &gq::gat_pool_bwd_input);
}
