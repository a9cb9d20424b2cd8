// Fused GATConv front end of the network-wide SoilNet layout: every node becomes its own LSTM
// sequence (no node pooling), and the kernel writes the time-major LSTM input itself.
//
// The math is gat.hip's (scores and the aggregate in the Cin-dimensional input space, the attention
// recomputed in the backward and never stored, parameter gradients kept in registers and written as
// one record per (workgroup, head)); see the header of gat.hip for the derivation. What differs:
//
//   * N <= 256: a node's neighbour mask is ceil(N / 64) 64-bit words (gat_node_adj_bits, once per
//     batch). A lane keeps GATN_WORDS = 4 words in registers, the words past the node count zero,
//     and walks them in ascending j with one fixed, fully unrolled word loop: an empty word costs
//     one compare, and the instances need no template on the word count.
//   * the output is per node: out [T][Mp][Cp], row m = b * N + i, channels [H*C GAT | Cin raw x |
//     0 pad], rows M = B*N .. Mp zero. This is gcn_node_fwd's layout, the input of
//     TimeLayer.forward_time_major(h, B*N). Each lane writes its own row with 16-byte stores;
//     adjacent lanes hold adjacent rows, so a wave's stores are one contiguous run.
//   * the upstream gradient of node i is g[c] = mask_i * dout[t][b*N+i][h*C+c] (gat.hip: pool weight
//     times the pooled row's gradient), and dx gets the raw channels' gradient passed through.
//
// Mapping: one lane per (row = (b, t), node i); a row's NP = pow2 >= N lanes are adjacent, a
// workgroup of 256 lanes holds 256 / NP rows per pass (one row at N > 128) with the row's x and
// s_nb in LDS. A pass is a few dependent memory round trips (mask, bits and x in; barrier; LDS walk;
// stores out, drained at the next barrier) with little arithmetic between them, so a launch is
// latency bound and wants every workgroup slot of the 256 CUs filled: the grid caps below are 256 x
// the workgroups per CU that the SoilNet instance <3, 16, 1> fits by registers (forward 57 VGPRs: 8;
// input backward 157: 3, rounded up to 4; parameter backward 218: 2). More row blocks than the cap
// take several passes per workgroup. The SoilNet step (B*T = 10784 rows of N = 210, one row per
// pass) runs 5.3 / 10.5 / 21.1 passes per workgroup there, and the backward writes 512 * H records (82 and
// 174 us of a 2.67 ms step; with one workgroup per CU, 42 passes each, they took 221 and 317 us:
// profiles/gat_node_ab.txt). No float atomics: results are bitwise reproducible.
#include "gat_common.h"

namespace gq {

constexpr int GATN_MAX_N = 256;
constexpr int GATN_WORDS = GATN_MAX_N / 64;
constexpr int GATN_FWD_WGS = 2048;       // workgroups per launch of gat_node_fwd,
constexpr int GATN_BWD_IN_WGS = 1024;    // gat_node_bwd_input
constexpr int GATN_BWD_WGS = 512;        // and gat_node_bwd (= its records per head)

// bits [2][B][N][NWD]: bits[0][b][i]: the neighbours j of node i ((adj + I * mask) > 0), bit j % 64
// of word j / 64; bits[1][b][i]: the nodes that have i as a neighbour (the transposed mask, for
// the input gradient). One thread per (b, i, word).
__global__ void gat_node_adj_bits_kernel(const float* __restrict__ adj, const float* __restrict__ mask,
                                         gat_bits_t* __restrict__ bits, int B, int N, int NWD) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= (long)B * N * NWD) return;
  const int w = (int)(e % NWD), i = (int)((e / NWD) % N), b = (int)(e / ((long)NWD * N));
  const float* a = adj + (long)b * N * N;
  gat_bits_t r = 0, c = 0;
  const int j1 = min(N, w * 64 + 64);
  for (int j = w * 64; j < j1; ++j) {
    if (a[(long)i * N + j] > 0.f) r |= 1ull << (j & 63);
    if (a[(long)j * N + i] > 0.f) c |= 1ull << (j & 63);
  }
  if ((i >> 6) == w && mask[(long)b * N + i] > 0.f) {
    r |= 1ull << (i & 63);
    c |= 1ull << (i & 63);
  }
  bits[e] = r;
  bits[(long)B * N * NWD + e] = c;
}

// a node's mask words into registers (the words past NWD stay zero)
__device__ __forceinline__ void gatn_load_bits(const gat_bits_t* __restrict__ p, int NWD,
                                               gat_bits_t (&nb)[GATN_WORDS]) {
#pragma unroll
  for (int w = 0; w < GATN_WORDS; ++w) nb[w] = w < NWD ? p[w] : 0;
}

// the set bits of nb[0..GATN_WORDS) in ascending j
#define GATN_WALK(nb, j)                                          \
  _Pragma("unroll") for (int w__ = 0; w__ < GATN_WORDS; ++w__)    \
    for (gat_bits_t m__ = (nb)[w__]; m__; m__ &= m__ - 1)         \
      if (const int j = w__ * 64 + __ffsll((long long)m__) - 1; true)

// gat.hip's gat_attend over mask words: m = max_j e_j, inv = 1 / sum_j exp(e_j - m) (0 for a node
// without neighbours: the aggregate is then zero, as in the eager layer), and the aggregate formed
// around the node's own features, z = x_i + zc, zc = sum_j att_j (x_j - x_i).
template <int CIN>
__device__ __forceinline__ void gatn_attend(const gat_bits_t (&nb)[GATN_WORDS], float ss, const float (&xi)[CIN],
                                            const float* xr, const float* nr, int hs, float& m, float& inv,
                                            float (&zc)[CIN], float (&z)[CIN]) {
  m = -3.0e38f;
  GATN_WALK(nb, j) m = fmaxf(m, gat_leaky(ss + nr[j * hs]));
  float den = 0.f;
#pragma unroll
  for (int f = 0; f < CIN; ++f) zc[f] = 0.f;
  GATN_WALK(nb, j) {
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

// One (node i, head h) of the backward up to the aggregate's gradient (gat.hip's gat_head_bwd):
// from g[c] = mask_i * upstream gradient gives dout[c] = dL/d(z W + bias)[c] and dz[f] = dL/dz[f].
template <int CIN, int C, int H>
__device__ __forceinline__ void gatn_head_bwd(const GatParams<CIN, C, H>& prm, int h,
                                              const gat_bits_t (&nb)[GATN_WORDS], float ss, const float (&xi)[CIN],
                                              const float* xr, const float* nrh, int hs, const float (&g)[C], int act,
                                              float& m, float& inv, float (&zc)[CIN], float (&z)[CIN], float (&o)[C],
                                              float (&dout)[C], float (&dz)[CIN]) {
  gatn_attend<CIN>(nb, ss, xi, xr, nrh, hs, m, inv, zc, z);
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

// ------------------------------------------------------------------ forward
// out [T][Mp][Cp]: row b*N+i of step t = [act(z W + bias) * mask_i (H*C) | x_i (CIN) | 0]; the rows
// B*N .. Mp of a step are zeroed by the lanes of its (B-1, t) row.
template <int CIN, int C, int H>
__global__ __launch_bounds__(256) void gat_node_fwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const float* __restrict__ mask,
    const float* __restrict__ W, const float* __restrict__ as, const float* __restrict__ an,
    const float* __restrict__ bias, const float* __restrict__ alpha, float* __restrict__ out, int B, int T, int N,
    int NP, int NWD, int act, int Mp, int Cp) {
  using P = GatParams<CIN, C, H>;
  constexpr int HC = H * C;
  __shared__ float sp[P::SIZE];
  __shared__ float sx[256 * CIN];
  __shared__ float snb[256 * H];
  P prm{sp};
  prm.load(W, as, an, bias, alpha);
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const long rows = (long)B * T;
  const int M = B * N;
  for (long row0 = (long)blockIdx.x * rpw; row0 < rows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const bool real = row < rows && i < N;
    float xi[CIN], mk = 0.f;
    gat_bits_t nb[GATN_WORDS] = {0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < CIN; ++f) xi[f] = 0.f;
    if (real) {
      const long bn = (row / T) * N + i;
      mk = mask[bn];
      gatn_load_bits(bits + bn * NWD, NWD, nb);         // (not behind the mask load: one round trip less)
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
    if (row >= rows) continue;                    // (no barrier or shuffle below in the loop)
    const int b = (int)(row / T), t = (int)(row % T);
    float* orow = out + (long)t * Mp * Cp;
    if (b == B - 1) {                             // this step's padding rows
      for (int pr = M + i; pr < Mp; pr += NP)
        for (int c = 0; c < Cp; c += 4) *reinterpret_cast<float4*>(orow + (long)pr * Cp + c) = make_float4(0, 0, 0, 0);
    }
    if (i >= N) continue;
    float acc[HC];
#pragma unroll
    for (int k = 0; k < HC; ++k) acc[k] = 0.f;
    if (mk != 0.f) {
      const float* xr = sx + rl * NP * CIN;
      const float* nr = snb + rl * NP * H;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float m, inv, zc[CIN], z[CIN];
        gatn_attend<CIN>(nb, ss[h], xi, xr, nr + h, H, m, inv, zc, z);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          float o = prm.bias(h * C + c);
#pragma unroll
          for (int f = 0; f < CIN; ++f) o += z[f] * prm.W(f, h, c);
          acc[h * C + c] = mk * gat_act(o, prm.alpha(h * C + c), act);
        }
      }
    }
    float* op = orow + ((long)b * N + i) * Cp;
#pragma unroll
    for (int k = 0; k < HC; k += 4)
      *reinterpret_cast<float4*>(op + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
    // (Cp >= HC + CIN, a multiple of 4, and CIN <= 4: the raw channels sit in the first tail chunk)
    *reinterpret_cast<float4*>(op + HC) = make_float4(xi[0], CIN > 1 ? xi[CIN > 1 ? 1 : 0] : 0.f,
                                                      CIN > 2 ? xi[CIN > 2 ? 2 : 0] : 0.f,
                                                      CIN > 3 ? xi[CIN > 3 ? 3 : 0] : 0.f);
    for (int c = HC + 4; c < Cp; c += 4) *reinterpret_cast<float4*>(op + c) = make_float4(0, 0, 0, 0);
  }
}

// ------------------------------------------------------------------ backward (parameters)
// grid (workgroups, H): workgroup (k, h) handles head h of its rows. partial [gridDim.x][H][R],
// R = CIN*C + 2C + 2CIN: dW[f][c] | dbias[c] | dalpha[c] | du_s[f] | du_n[f] (gat.hip's record:
// the fixed-order column sum and gat_bwd_finalize take it as it is). dout [T][Mp][Cp].
template <int CIN, int C, int H>
__global__ __launch_bounds__(256) void gat_node_bwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const float* __restrict__ mask,
    const float* __restrict__ dout, const float* __restrict__ W, const float* __restrict__ as,
    const float* __restrict__ an, const float* __restrict__ bias, const float* __restrict__ alpha,
    float* __restrict__ partial, int B, int T, int N, int NP, int NWD, int act, int Mp, int Cp) {
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
    float xi[CIN], mk = 0.f;
    gat_bits_t nb[GATN_WORDS] = {0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < CIN; ++f) xi[f] = 0.f;
    if (real) {
      const long bn = (row / T) * N + i;
      mk = mask[bn];
      gatn_load_bits(bits + bn * NWD, NWD, nb);         // (not behind the mask load: one round trip less)
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
    if (!(real && mk != 0.f)) continue;           // (no barrier or shuffle below in the loop)
    const float* xr = sx + rl * NP * CIN;
    const float* nr = snb + rl * NP;
    const long dro = ((row % T) * (long)Mp + (row / T) * N + i) * Cp;
    float g[C], o[C], dO[C], zc[CIN], z[CIN], dz[CIN], m, inv;
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = mk * dout[dro + h * C + c];
    // (s_nb has stride 1 here: one head per workgroup)
    gatn_head_bwd<CIN, C, H>(prm, h, nb, ss, xi, xr, nr, 1, g, act, m, inv, zc, z, o, dO, dz);
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
    GATN_WALK(nb, j) {
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

// ------------------------------------------------------------------ backward (input)
// dx_j = dout[raw channels of j] + the GAT term. Phase 1, lane (row, i): the softmax state of node i
// and dL/dz_i per head, parked in LDS, and the s_self part of dx_i. Phase 2, lane (row, j): gathers
// over the nodes i that have j as a neighbour (transposed mask): dx_j += att_ij dz_i + ds_ij u_n.
// Every dx element is written by exactly one lane: no atomics.
template <int CIN, int C, int H>
__global__ __launch_bounds__(256) void gat_node_bwd_input_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const gat_bits_t* __restrict__ bitsT,
    const float* __restrict__ mask, const float* __restrict__ dout, const float* __restrict__ W,
    const float* __restrict__ as, const float* __restrict__ an, const float* __restrict__ bias,
    const float* __restrict__ alpha, float* __restrict__ dx, int B, int T, int N, int NP, int NWD, int act, int Mp,
    int Cp) {
  using P = GatParams<CIN, C, H>;
  constexpr int HC = H * C;
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
    float xi[CIN], mk = 0.f;
    gat_bits_t nb[GATN_WORDS] = {0, 0, 0, 0}, nbT[GATN_WORDS] = {0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < CIN; ++f) xi[f] = 0.f;
    if (real) {
      const long bn = (row / T) * N + i;
      mk = mask[bn];
      gatn_load_bits(bits + bn * NWD, NWD, nb);         // (not behind the mask load: one round trip less)
      gatn_load_bits(bitsT + bn * NWD, NWD, nbT);
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
    const bool on = real && mk != 0.f;
    const long dro = real ? ((row % T) * (long)Mp + (row / T) * N + i) * Cp : 0;
    if (real) {
#pragma unroll
      for (int f = 0; f < CIN; ++f) dxi[f] = dout[dro + HC + f];      // the raw channels pass through
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float m = 0.f, inv = 0.f, dzc = 0.f, dz[CIN];
#pragma unroll
      for (int f = 0; f < CIN; ++f) dz[f] = 0.f;
      if (on) {
        float g[C], o[C], dO[C], zc[CIN], z[CIN];
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = mk * dout[dro + h * C + c];
        gatn_head_bwd<CIN, C, H>(prm, h, nb, ss[h], xi, xr, nr + h, H, g, act, m, inv, zc, z, o, dO, dz);
#pragma unroll
        for (int f = 0; f < CIN; ++f) dzc += dz[f] * zc[f];
        float sds = 0.f;
        GATN_WALK(nb, j) {
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
    GATN_WALK(nbT, k) {                           // node k attends to this lane's node
      const int lk = rl * NP + k;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float* st = sst + (lk * H + h) * 4;
        const float inv = st[2];
        if (inv == 0.f) continue;
        const float e = st[0] + sn[h];
        const float att = __expf(gat_leaky(e) - st[1]) * inv;
        const float* dzk = sdz + (lk * H + h) * CIN;
        float da = -st[3];                        // dz_k . (x_j - x_k) - dz_k . zc_k
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
struct GatNodeDims {
  int B, T, N, Cin, C, H, NP, rpw, NWD;
};

// shapes shared by the three kernels: x [B,T,N,Cin], bits [2,B,N,NWD], mask [B,N], W [Cin,H,C],
// a_s / a_n [C,H(,1)], bias [H*C], alpha [H*C] or empty
static GatNodeDims gat_node_check(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& mask,
                                  const at::Tensor& W, const at::Tensor& as, const at::Tensor& an,
                                  const at::Tensor& bias, const at::Tensor& alpha, int64_t act) {
  for (auto* p : {&x, &mask, &W, &as, &an, &bias}) check_f32_cuda(*p, "gat_node input");
  TORCH_CHECK(x.dim() == 4 && W.dim() == 3, "gat_node: x must be [B,T,N,Cin], W [Cin,H,C]");
  GatNodeDims d;
  d.B = x.size(0), d.T = x.size(1), d.N = x.size(2), d.Cin = x.size(3), d.H = W.size(1), d.C = W.size(2);
  TORCH_CHECK(d.N >= 1 && d.N <= GATN_MAX_N, "gat_node: 1..256 nodes");
  TORCH_CHECK(W.size(0) == d.Cin, "gat_node: W must be [Cin,H,C]");
  d.NWD = (d.N + 63) / 64;
  TORCH_CHECK(bits.is_cuda() && bits.scalar_type() == at::kLong && bits.is_contiguous() &&
              bits.numel() == 2L * d.B * d.N * d.NWD, "gat_node: bits must be int64 [2,B,N,ceil(N/64)]");
  TORCH_CHECK(mask.numel() == (long)d.B * d.N, "gat_node: mask must be [B,N]");
  TORCH_CHECK((long)d.B * d.N + 15 < (1L << 31), "gat_node: B*N too large");
  TORCH_CHECK(as.numel() == d.C * d.H && an.numel() == d.C * d.H, "gat_node: attention kernels must be [C,H]");
  TORCH_CHECK(bias.numel() == d.H * d.C, "gat_node: bias must be [H*C]");
  TORCH_CHECK(act >= GAT_ACT_LINEAR && act <= GAT_ACT_RELU, "gat_node: activation code");
  if (act == GAT_ACT_PRELU) {
    check_f32_cuda(alpha, "alpha");
    TORCH_CHECK(alpha.numel() == d.H * d.C, "gat_node: alpha must be [H*C]");
  }
  d.NP = gat_pow2(d.N);
  d.rpw = 256 / d.NP;
  return d;
}

static int gat_node_grid(long rows, int rpw, int cap) {
  return (int)std::max<long>(1, std::min<long>((rows + rpw - 1) / rpw, cap));
}

static const gat_bits_t* gat_node_bits_ptr(const at::Tensor& bits) {
  return reinterpret_cast<const gat_bits_t*>(bits.data_ptr<int64_t>());
}

// dout [T, Mp, Cp] as the forward wrote it
static void gat_node_check_dout(const at::Tensor& dout, const GatNodeDims& d) {
  check_f32_cuda(dout, "dout");
  TORCH_CHECK(dout.dim() == 3 && dout.size(0) == d.T && dout.size(1) >= (long)d.B * d.N &&
              dout.size(2) >= d.H * d.C + d.Cin, "gat_node: dout must be [T, Mp >= B*N, Cp >= H*C + Cin]");
}

at::Tensor gat_node_adj_bits(const at::Tensor& adj, const at::Tensor& mask) {
  check_f32_cuda(adj, "adj");
  check_f32_cuda(mask, "mask");
  TORCH_CHECK(adj.dim() == 3 && adj.size(1) == adj.size(2), "gat_node: adj must be [B,N,N]");
  const int B = adj.size(0), N = adj.size(1);
  TORCH_CHECK(N >= 1 && N <= GATN_MAX_N, "gat_node: 1..256 nodes");
  TORCH_CHECK(mask.dim() == 2 && mask.size(0) == B && mask.size(1) == N, "gat_node: mask must be [B,N]");
  const int NWD = (N + 63) / 64;
  c10::DeviceGuard guard(adj.device());
  at::Tensor bits = at::empty({2, B, N, NWD}, adj.options().dtype(at::kLong));
  if (B == 0) return bits;
  hipLaunchKernelGGL(gat_node_adj_bits_kernel, dim3(((long)B * N * NWD + 255) / 256), dim3(256), 0, stream(),
                     adj.data_ptr<float>(), mask.data_ptr<float>(),
                     reinterpret_cast<gat_bits_t*>(bits.data_ptr<int64_t>()), B, N, NWD);
  GQ_LAUNCH_CHECK();
  return bits;
}

at::Tensor gat_node_fwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& mask, const at::Tensor& W,
                        const at::Tensor& as, const at::Tensor& an, const at::Tensor& bias, const at::Tensor& alpha,
                        int64_t act, int64_t Mp, int64_t Cp) {
  const GatNodeDims d = gat_node_check(x, bits, mask, W, as, an, bias, alpha, act);
  const long M = (long)d.B * d.N;
  TORCH_CHECK(Mp >= M && Mp % 16 == 0 && Mp < M + 16 && Cp % 4 == 0 && Cp >= d.H * d.C + d.Cin,
              "gat_node_fwd: Mp must be B*N rounded up to 16, Cp a multiple of 4 >= H*C + Cin");
  c10::DeviceGuard guard(x.device());
  at::Tensor out = at::empty({d.T, Mp, Cp}, x.options());
  const long rows = (long)d.B * d.T;
  if (rows == 0) return out.zero_();
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  GQ_GAT_DISPATCH(d.Cin, d.C, d.H,
      hipLaunchKernelGGL((gat_node_fwd_kernel<CIN, C, H>), dim3(gat_node_grid(rows, d.rpw, GATN_FWD_WGS)), dim3(256), 0,
                         stream(), x.data_ptr<float>(), gat_node_bits_ptr(bits), mask.data_ptr<float>(), W.data_ptr<float>(),
                         as.data_ptr<float>(), an.data_ptr<float>(), bias.data_ptr<float>(), al_p,
                         out.data_ptr<float>(), d.B, d.T, d.N, d.NP, d.NWD, (int)act, (int)Mp, (int)Cp));
  GQ_LAUNCH_CHECK();
  return out;
}

// the summed records [H, R] of the parameter gradients (see gat_node_bwd_kernel)
at::Tensor gat_node_bwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& mask, const at::Tensor& dout,
                        const at::Tensor& W, const at::Tensor& as, const at::Tensor& an, const at::Tensor& bias,
                        const at::Tensor& alpha, int64_t act) {
  const GatNodeDims d = gat_node_check(x, bits, mask, W, as, an, bias, alpha, act);
  gat_node_check_dout(dout, d);
  c10::DeviceGuard guard(x.device());
  const int R = d.Cin * d.C + 2 * d.C + 2 * d.Cin;
  const long rows = (long)d.B * d.T;
  if (rows == 0) return at::zeros({d.H, R}, x.options());
  const int nblk = gat_node_grid(rows, d.rpw, GATN_BWD_WGS);
  at::Tensor partial = at::empty({nblk, d.H, R}, x.options());
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  GQ_GAT_DISPATCH(d.Cin, d.C, d.H,
      hipLaunchKernelGGL((gat_node_bwd_kernel<CIN, C, H>), dim3(nblk, d.H), dim3(256), 0, stream(),
                         x.data_ptr<float>(), gat_node_bits_ptr(bits), mask.data_ptr<float>(), dout.data_ptr<float>(),
                         W.data_ptr<float>(), as.data_ptr<float>(), an.data_ptr<float>(), bias.data_ptr<float>(),
                         al_p, partial.data_ptr<float>(), d.B, d.T, d.N, d.NP, d.NWD, (int)act, (int)dout.size(1),
                         (int)dout.size(2)));
  GQ_LAUNCH_CHECK();
  return nblk == 1 ? partial.view({d.H, R}) : colsum(partial);       // fixed order: deterministic
}

at::Tensor gat_node_bwd_input(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& mask,
                              const at::Tensor& dout, const at::Tensor& W, const at::Tensor& as, const at::Tensor& an,
                              const at::Tensor& bias, const at::Tensor& alpha, int64_t act) {
  const GatNodeDims d = gat_node_check(x, bits, mask, W, as, an, bias, alpha, act);
  gat_node_check_dout(dout, d);
  c10::DeviceGuard guard(x.device());
  at::Tensor dx = at::empty_like(x);
  const long rows = (long)d.B * d.T;
  if (rows == 0) return dx;
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  const gat_bits_t* bp = gat_node_bits_ptr(bits);
  GQ_GAT_DISPATCH(d.Cin, d.C, d.H,
      hipLaunchKernelGGL((gat_node_bwd_input_kernel<CIN, C, H>), dim3(gat_node_grid(rows, d.rpw, GATN_BWD_IN_WGS)), dim3(256),
                         0, stream(), x.data_ptr<float>(), bp, bp + (long)d.B * d.N * d.NWD, mask.data_ptr<float>(),
                         dout.data_ptr<float>(), W.data_ptr<float>(), as.data_ptr<float>(), an.data_ptr<float>(),
                         bias.data_ptr<float>(), al_p, dx.data_ptr<float>(), d.B, d.T, d.N, d.NP, d.NWD, (int)act,
                         (int)dout.size(1), (int)dout.size(2)));
  GQ_LAUNCH_CHECK();
  return dx;
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("gat_node_adj_bits", &gq::gat_node_adj_bits);
  m.impl("gat_node_fwd", &gq::gat_node_fwd);
  m.impl("gat_node_bwd", &gq::gat_node_bwd);
  m.impl("gat_node_bwd_input", &gq::gat_node_bwd_input);
}
