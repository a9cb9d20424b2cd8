// Fused EdgeConv + node pooling + concat for the CML front end.
//
// spektral EdgeConv(channels, mlp_hidden=None, aggregate in {sum, mean}) on a dense per-sample
// graph, followed by `timeseries_pooling` and Concatenate([flagged series, pooled])
// (gnnqc/models/graphconv.py EdgeConv is the eager form). With W [2 Cin, C] = [Wa ; Wb] the edge
// message splits in the input space:
//
//   z_ij = [x_i | x_j - x_i] W + b = p_i + q_j     p_i = x_i (Wa - Wb) + b,   q_j = x_j Wb
//   o_i  = mask_i s_i sum_{j: adj_ij > 0} act(z_ij)     s_i = 1 (sum) or 1 / max(deg_i, 1) (mean)
//   out  = [anom | sum_i pw_i o_i]                      pw: node pool weights (mask included)
//
// so an edge costs one add and one activation per channel, and neither z nor act(z) is stored:
// the backward recomputes them. No self loop is added, and the mask is not folded into the
// neighbour words (an edge towards a masked node counts, as in the eager layer). Mapping (all three
// kernels, as in gat.hip): one lane per (row = (b, t), node i); a row's NP = pow2 >= N lanes are
// adjacent lanes of one wave, so the node pool is a shuffle reduction; a lane walks the set bits
// of its node's 64-bit neighbour word (edge_adj_bits, once per batch). Hence N <= 64. Channels are
// staged through LDS in chunks of EDGE_CH: q (and in the backward p) of the row's nodes, one
// 16-byte-aligned slab of EDGE_PITCH floats per node, read as two b128 loads per edge; the pitch of
// 12 floats spreads consecutive nodes over all sixteen 16-byte slots of a bank row.
//
// The backward needs, per node, dp_i = sum_j e_ij and dq_i = sum_{k: adj_ki > 0} e_ki with
// e_ij = act'(z_ij) g_i and g_i = pw_i s_i dout: the second sum is a gather over the transposed
// neighbour word, so every value is written by exactly one lane. edge_pool_bwd runs one channel
// chunk per workgroup (grid.y), keeps [d(Wa - Wb) | dWb-direct | db | dalpha] of the chunk in
// registers over its passes and writes ONE record per workgroup; a fixed-order column sum and
// edge_bwd_finalize (dWa = d(Wa - Wb), dWb = direct - d(Wa - Wb)) follow. No float atomics
// anywhere: results are bitwise reproducible.
#include "gat_common.h"

namespace gq {

constexpr int EDGE_MAX_N = 64;
constexpr int EDGE_GRID_CAP = 256;       // workgroups per launch: more rows take several passes
constexpr int EDGE_CH = 8;               // channels per LDS stage (and per workgroup of edge_pool_bwd)
constexpr int EDGE_PITCH = 12;           // floats per node slab in LDS (16-byte aligned)

// Parameters in LDS (wave-uniform broadcast reads): Wd = Wa - Wb [Cin][C], Wb [Cin][C], bias [C],
// slope [C]. The three activations are one expression, act(z) = z > 0 ? z : slope z, with slope =
// alpha (PReLU), 0 (ReLU) or 1 (linear), so the per-edge loops carry no switch on the activation;
// act'(z) = z > 0 ? 1 : slope takes the slope AT zero, as the eager layer's where(z > 0, ..) and
// relu do.
template <int CIN, int C>
struct EdgeParams {
  static constexpr int NW = CIN * C;
  static constexpr int SIZE = 2 * NW + 2 * C;
  float* p;
  __device__ float wd(int f, int c) const { return p[f * C + c]; }
  __device__ float wb(int f, int c) const { return p[NW + f * C + c]; }
  __device__ float bias(int c) const { return p[2 * NW + c]; }
  __device__ float slope(int c) const { return p[2 * NW + C + c]; }
  __device__ void load(const float* __restrict__ Wg, const float* __restrict__ bg, const float* __restrict__ alg,
                       int act) {
    const int tid = threadIdx.x;
    for (int i = tid; i < NW; i += blockDim.x) {
      const float b = Wg[NW + i];
      p[i] = Wg[i] - b;
      p[NW + i] = b;
    }
    for (int i = tid; i < C; i += blockDim.x) {
      p[2 * NW + i] = bg[i];
      p[2 * NW + C + i] = act == GAT_ACT_PRELU ? alg[i] : (act == GAT_ACT_RELU ? 0.f : 1.f);
    }
    __syncthreads();
  }
};

// bits[0][b][i]: neighbours j of node i (adj_ij > 0, nothing else); bits[1][b][i]: nodes that have
// i as a neighbour (the transposed word, for dq). The degree is the popcount of bits[0].
__global__ void edge_adj_bits_kernel(const float* __restrict__ adj, gat_bits_t* __restrict__ bits, int B, int N) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= (long)B * N) return;
  const int b = (int)(e / N), i = (int)(e % N);
  const float* a = adj + (long)b * N * N;
  gat_bits_t r = 0, c = 0;
  for (int j = 0; j < N; ++j) {
    if (a[i * N + j] > 0.f) r |= 1ull << j;
    if (a[j * N + i] > 0.f) c |= 1ull << j;
  }
  bits[e] = r;
  bits[(long)B * N + e] = c;
}

// p_i and q_i of one node for the channels c0 .. c0 + EDGE_CH
template <int CIN, int C>
__device__ __forceinline__ void edge_pq(const EdgeParams<CIN, C>& prm, int c0, const float (&xi)[CIN],
                                        float (&pi)[EDGE_CH], float (&qi)[EDGE_CH]) {
#pragma unroll
  for (int k = 0; k < EDGE_CH; ++k) {
    float p = prm.bias(c0 + k), q = 0.f;
#pragma unroll
    for (int f = 0; f < CIN; ++f) {
      p += xi[f] * prm.wd(f, c0 + k);
      q += xi[f] * prm.wb(f, c0 + k);
    }
    pi[k] = p;
    qi[k] = q;
  }
}

__device__ __forceinline__ void edge_put(float* s, const float (&v)[EDGE_CH]) {
  reinterpret_cast<float4*>(s)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(s)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

__device__ __forceinline__ void edge_get(const float* s, float (&v)[EDGE_CH]) {
  const float4 a = reinterpret_cast<const float4*>(s)[0], b = reinterpret_cast<const float4*>(s)[1];
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
  v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}

// The lane's node of its row: x_i, the neighbour words, and kc = pw_i s_i (0: the node adds nothing
// to the pooled output). Lanes past the row's nodes or past the last row hold zeros.
template <int CIN>
struct EdgeNode {
  float xi[CIN];
  float kc;
  gat_bits_t nb, nbT;
  bool real;
};

template <int CIN>
__device__ __forceinline__ EdgeNode<CIN> edge_node(const float* __restrict__ x, const gat_bits_t* __restrict__ bits,
                                                   const gat_bits_t* __restrict__ bitsT,
                                                   const float* __restrict__ pw, long row, long rows, int i, int T,
                                                   int N, int mean) {
  EdgeNode<CIN> n;
  n.real = row < rows && i < N;
  n.kc = 0.f;
  n.nb = n.nbT = 0;
#pragma unroll
  for (int f = 0; f < CIN; ++f) n.xi[f] = 0.f;
  if (n.real) {
    const long bn = (row / T) * N + i;
    n.nb = bits[bn];
    if (bitsT != nullptr) n.nbT = bitsT[bn];
    const float p = pw[bn];
    n.kc = mean ? p / (float)max(__popcll(n.nb), 1) : p;
#pragma unroll
    for (int f = 0; f < CIN; ++f) n.xi[f] = x[(row * N + i) * CIN + f];
  }
  return n;
}

// ------------------------------------------------------------------ forward
// out: Mp > 0: time-major LSTM input [T][Mp][Cp] (rows b >= B and channels >= Ca + C zero), else
// [B][T][Ca + C] (the host passes Cp = Ca + C then). pw [B][N]: node pool weights (mask included:
// a masked node has weight 0).
template <int CIN, int C>
__global__ __launch_bounds__(256) void edge_pool_fwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const float* __restrict__ pw,
    const float* __restrict__ anom, const float* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ alpha, float* __restrict__ out, int B, int T, int N, int NP, int Ca, int act,
    int mean, int Mp, int Cp) {
  using P = EdgeParams<CIN, C>;
  __shared__ float sprm[P::SIZE];
  __shared__ __align__(16) float sq[256 * EDGE_PITCH];
  P prm{sprm};
  prm.load(W, bias, alpha, act);
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const int Fo = Ca + C;
  const long rows = (long)B * T;
  const long vrows = Mp > 0 ? (long)Mp * T : rows;        // virtual rows incl. zero padding rows
  const float* qr = sq + rl * NP * EDGE_PITCH;
  for (long row0 = (long)blockIdx.x * rpw; row0 < vrows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const EdgeNode<CIN> n = edge_node<CIN>(x, bits, nullptr, pw, row, rows, i, T, N, mean);
    float acc[C];
#pragma unroll
    for (int c0 = 0; c0 < C; c0 += EDGE_CH) {
      float pi[EDGE_CH], qi[EDGE_CH], al[EDGE_CH], a[EDGE_CH];
      edge_pq<CIN, C>(prm, c0, n.xi, pi, qi);
      __syncthreads();                            // the previous stage's readers are done
      edge_put(sq + tid * EDGE_PITCH, qi);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < EDGE_CH; ++k) {
        a[k] = 0.f;
        al[k] = prm.slope(c0 + k);
      }
      if (n.kc != 0.f) {
        for (gat_bits_t w = n.nb; w; w &= w - 1) {
          const int j = __ffsll((long long)w) - 1;
          float q[EDGE_CH];
          edge_get(qr + j * EDGE_PITCH, q);
#pragma unroll
          for (int k = 0; k < EDGE_CH; ++k) {
            const float z = pi[k] + q[k];
            a[k] += z > 0.f ? z : al[k] * z;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < EDGE_CH; ++k) acc[c0 + k] = n.kc * a[k];
    }
    // node pool: sum over the row's NP lanes (every lane of the wave takes part)
    for (int o = NP >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < C; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    if (row >= vrows) continue;
    float* op = Mp > 0 ? out + ((row % T) * (long)Mp + row / T) * Cp : out + row * (long)Fo;
    if (row >= rows) {                            // (time-major only) padding row
      for (int c = i; c < Cp; c += NP) op[c] = 0.f;
      continue;
    }
    for (int c = i; c < Ca; c += NP) op[c] = anom[row * Ca + c];
    if (i == 0) {                                 // (every lane of the row holds the sums)
#pragma unroll
      for (int k = 0; k < C; ++k) op[Ca + k] = acc[k];
    }
    for (int c = Fo + i; c < Cp; c += NP) op[c] = 0.f;
  }
}

// ------------------------------------------------------------------ backward, shared part
// One node and channel chunk of the backward. pi / qi: the node's own p and q; pr / qr / kr: the
// row's p, q slabs and kc in LDS; al: the activation's slopes; G: the row's upstream gradient on
// the chunk. Gives dp[k] = dL/dp_i, dq[k] = dL/dq_i and dal[k] = the node's share of dalpha (PReLU;
// otherwise nobody asks for it).
__device__ __forceinline__ void edge_chunk_bwd(gat_bits_t nb, gat_bits_t nbT, float kc, const float (&pi)[EDGE_CH],
                                               const float (&qi)[EDGE_CH], const float (&al)[EDGE_CH],
                                               const float (&G)[EDGE_CH], const float* pr, const float* qr,
                                               const float* kr, float (&dp)[EDGE_CH], float (&dq)[EDGE_CH],
                                               float (&dal)[EDGE_CH]) {
#pragma unroll
  for (int k = 0; k < EDGE_CH; ++k) dp[k] = dq[k] = dal[k] = 0.f;
  if (kc != 0.f) {
    for (gat_bits_t w = nb; w; w &= w - 1) {
      const int j = __ffsll((long long)w) - 1;
      float q[EDGE_CH];
      edge_get(qr + j * EDGE_PITCH, q);
#pragma unroll
      for (int k = 0; k < EDGE_CH; ++k) {
        const float z = pi[k] + q[k];
        dp[k] += z > 0.f ? 1.f : al[k];
        dal[k] += z > 0.f ? 0.f : z;
      }
    }
  }
  for (gat_bits_t w = nbT; w; w &= w - 1) {
    const int s = __ffsll((long long)w) - 1;      // node s has this lane's node as a neighbour
    const float ks = kr[s];
    if (ks == 0.f) continue;
    float p[EDGE_CH];
    edge_get(pr + s * EDGE_PITCH, p);
#pragma unroll
    for (int k = 0; k < EDGE_CH; ++k) dq[k] += p[k] + qi[k] > 0.f ? ks : ks * al[k];
  }
#pragma unroll
  for (int k = 0; k < EDGE_CH; ++k) {
    dp[k] *= kc * G[k];
    dal[k] *= kc * G[k];
    dq[k] *= G[k];
  }
}

// ------------------------------------------------------------------ backward (parameters)
// grid (workgroups, C / EDGE_CH): workgroup (k, y) handles the channels y EDGE_CH .. of its rows.
// partial [gridDim.x][C / EDGE_CH][R], R = (2 CIN + 2) EDGE_CH:
// dWd[f][k] | dWq[f][k] | dbias[k] | dalpha[k]  (Wd = Wa - Wb; Wq: Wb through q alone).
// dout: [B][T][dstride], or time-major [T][dmp][dstride] when dmp > 0; the layer's channels
// start at c_off.
template <int CIN, int C>
__global__ __launch_bounds__(256) void edge_pool_bwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const gat_bits_t* __restrict__ bitsT,
    const float* __restrict__ pw, const float* __restrict__ dout, const float* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ alpha, float* __restrict__ partial, int B, int T,
    int N, int NP, int act, int mean, int c_off, int dstride, int dmp) {
  using P = EdgeParams<CIN, C>;
  constexpr int R = (2 * CIN + 2) * EDGE_CH;
  __shared__ float sprm[P::SIZE];
  __shared__ __align__(16) float sp[256 * EDGE_PITCH];
  __shared__ __align__(16) float sq[256 * EDGE_PITCH];
  __shared__ float sk[256];
  __shared__ float red[4][R];
  P prm{sprm};
  prm.load(W, bias, alpha, act);
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const int c0 = blockIdx.y * EDGE_CH;
  const long rows = (long)B * T;
  float aWd[CIN][EDGE_CH], aWq[CIN][EDGE_CH], ab[EDGE_CH], aal[EDGE_CH], al[EDGE_CH];
#pragma unroll
  for (int k = 0; k < EDGE_CH; ++k) {
    ab[k] = aal[k] = 0.f;
    al[k] = prm.slope(c0 + k);
#pragma unroll
    for (int f = 0; f < CIN; ++f) aWd[f][k] = aWq[f][k] = 0.f;
  }
  for (long row0 = (long)blockIdx.x * rpw; row0 < rows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const EdgeNode<CIN> n = edge_node<CIN>(x, bits, bitsT, pw, row, rows, i, T, N, mean);
    float pi[EDGE_CH], qi[EDGE_CH];
    edge_pq<CIN, C>(prm, c0, n.xi, pi, qi);
    __syncthreads();                              // the previous pass's readers are done
    edge_put(sp + tid * EDGE_PITCH, pi);
    edge_put(sq + tid * EDGE_PITCH, qi);
    sk[tid] = n.kc;
    __syncthreads();
    if (!n.real) continue;                        // (no barrier or shuffle below in the loop)
    const long dro = dmp > 0 ? ((row % T) * (long)dmp + row / T) * dstride : row * (long)dstride;
    float G[EDGE_CH], dp[EDGE_CH], dq[EDGE_CH], dal[EDGE_CH];
#pragma unroll
    for (int k = 0; k < EDGE_CH; ++k) G[k] = dout[dro + c_off + c0 + k];
    edge_chunk_bwd(n.nb, n.nbT, n.kc, pi, qi, al, G, sp + rl * NP * EDGE_PITCH, sq + rl * NP * EDGE_PITCH,
                   sk + rl * NP, dp, dq, dal);
#pragma unroll
    for (int k = 0; k < EDGE_CH; ++k) {
      ab[k] += dp[k];
      aal[k] += dal[k];
#pragma unroll
      for (int f = 0; f < CIN; ++f) {
        aWd[f][k] += n.xi[f] * dp[k];
        aWq[f][k] += n.xi[f] * dq[k];
      }
    }
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
    for (int k = 0; k < EDGE_CH; ++k) {
      put(f * EDGE_CH + k, aWd[f][k]);
      put((CIN + f) * EDGE_CH + k, aWq[f][k]);
    }
  }
#pragma unroll
  for (int k = 0; k < EDGE_CH; ++k) {
    put(2 * CIN * EDGE_CH + k, ab[k]);
    put((2 * CIN + 1) * EDGE_CH + k, aal[k]);
  }
  __syncthreads();
  for (int e = tid; e < R; e += blockDim.x)
    partial[((long)blockIdx.x * gridDim.y + blockIdx.y) * R + e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

// tot [C / EDGE_CH][R]: the summed records. Adds dW[f][c] = dWd, dW[Cin + f][c] = dWq - dWd, dbias
// and dalpha into the gradient buffers (nullptr: not needed).
__global__ __launch_bounds__(256) void edge_bwd_finalize_kernel(const float* __restrict__ tot, int CIN, int C,
                                                                float* __restrict__ dW, float* __restrict__ dbias,
                                                                float* __restrict__ dalpha) {
  const int R = (2 * CIN + 2) * EDGE_CH;
  for (int e = threadIdx.x; e < CIN * C; e += blockDim.x) {
    const int c = e % C, f = e / C;
    const float* t = tot + (c / EDGE_CH) * R;
    const float wd = t[f * EDGE_CH + c % EDGE_CH], wq = t[(CIN + f) * EDGE_CH + c % EDGE_CH];
    if (dW) {
      dW[e] += wd;
      dW[CIN * C + e] += wq - wd;
    }
  }
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float* t = tot + (c / EDGE_CH) * R;
    if (dbias) dbias[c] += t[2 * CIN * EDGE_CH + c % EDGE_CH];
    if (dalpha) dalpha[c] += t[(2 * CIN + 1) * EDGE_CH + c % EDGE_CH];
  }
}

// ------------------------------------------------------------------ backward (input)
// dx_i = (Wa - Wb) dp_i + Wb dq_i, the channel chunks staged one after the other. Every dx element
// is written by exactly one lane: no atomics. Masked nodes that are someone's neighbour receive
// their gradient through dq, as in the eager layer.
template <int CIN, int C>
__global__ __launch_bounds__(256) void edge_pool_bwd_input_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const gat_bits_t* __restrict__ bitsT,
    const float* __restrict__ pw, const float* __restrict__ dout, const float* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ alpha, float* __restrict__ dx, int B, int T, int N,
    int NP, int act, int mean, int c_off, int dstride, int dmp) {
  using P = EdgeParams<CIN, C>;
  __shared__ float sprm[P::SIZE];
  __shared__ __align__(16) float sp[256 * EDGE_PITCH];
  __shared__ __align__(16) float sq[256 * EDGE_PITCH];
  __shared__ float sk[256];
  P prm{sprm};
  prm.load(W, bias, alpha, act);
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const long rows = (long)B * T;
  for (long row0 = (long)blockIdx.x * rpw; row0 < rows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const EdgeNode<CIN> n = edge_node<CIN>(x, bits, bitsT, pw, row, rows, i, T, N, mean);
    const long dro = dmp > 0 ? ((row % T) * (long)dmp + row / T) * dstride : row * (long)dstride;
    float dxi[CIN];
#pragma unroll
    for (int f = 0; f < CIN; ++f) dxi[f] = 0.f;
#pragma unroll
    for (int c0 = 0; c0 < C; c0 += EDGE_CH) {
      float pi[EDGE_CH], qi[EDGE_CH];
      edge_pq<CIN, C>(prm, c0, n.xi, pi, qi);
      __syncthreads();                            // the previous stage's readers are done
      edge_put(sp + tid * EDGE_PITCH, pi);
      edge_put(sq + tid * EDGE_PITCH, qi);
      if (c0 == 0) sk[tid] = n.kc;
      __syncthreads();
      if (n.real) {
        float G[EDGE_CH], al[EDGE_CH], dp[EDGE_CH], dq[EDGE_CH], dal[EDGE_CH];
#pragma unroll
        for (int k = 0; k < EDGE_CH; ++k) {
          G[k] = dout[dro + c_off + c0 + k];
          al[k] = prm.slope(c0 + k);
        }
        edge_chunk_bwd(n.nb, n.nbT, n.kc, pi, qi, al, G, sp + rl * NP * EDGE_PITCH, sq + rl * NP * EDGE_PITCH,
                       sk + rl * NP, dp, dq, dal);
#pragma unroll
        for (int k = 0; k < EDGE_CH; ++k) {
#pragma unroll
          for (int f = 0; f < CIN; ++f) dxi[f] += prm.wd(f, c0 + k) * dp[k] + prm.wb(f, c0 + k) * dq[k];
        }
      }
    }
    if (n.real) {
#pragma unroll
      for (int f = 0; f < CIN; ++f) dx[(row * N + i) * CIN + f] = dxi[f];
    }
  }
}

// ------------------------------------------------------------------ instance table
#define GQ_EDGE_DISPATCH(CIN_RT, C_RT, ...)                                              \
  do {                                                                                   \
    const int key__ = (int)(CIN_RT) * 100 + (int)(C_RT);                                 \
    switch (key__) {                                                                     \
      GQ_EDGE_CASES(1, __VA_ARGS__) GQ_EDGE_CASES(2, __VA_ARGS__)                        \
      GQ_EDGE_CASES(3, __VA_ARGS__) GQ_EDGE_CASES(4, __VA_ARGS__)                        \
      default: TORCH_CHECK(false, "edge: Cin 1..4, C in {8, 16, 32}");                   \
    }                                                                                    \
  } while (0)
#define GQ_EDGE_CASE(CI, CC, ...) \
  case CI * 100 + CC: { constexpr int CIN = CI, C = CC; __VA_ARGS__; } break;
#define GQ_EDGE_CASES(CI, ...) \
  GQ_EDGE_CASE(CI, 8, __VA_ARGS__) GQ_EDGE_CASE(CI, 16, __VA_ARGS__) GQ_EDGE_CASE(CI, 32, __VA_ARGS__)

// ------------------------------------------------------------------ host
struct EdgeDims {
  int B, T, N, Cin, C, NP, rpw;
};

// shapes shared by the three kernels: x [B,T,N,Cin], bits [2,B,N], pw [B,N], W [2 Cin,C],
// bias [C], alpha [C] or empty
static EdgeDims edge_check(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& W,
                           const at::Tensor& bias, const at::Tensor& alpha, int64_t act) {
  for (auto* p : {&x, &pw, &W, &bias}) check_f32_cuda(*p, "edge input");
  TORCH_CHECK(x.dim() == 4 && W.dim() == 2, "edge: x must be [B,T,N,Cin], W [2 Cin,C]");
  EdgeDims d;
  d.B = x.size(0), d.T = x.size(1), d.N = x.size(2), d.Cin = x.size(3), d.C = W.size(1);
  TORCH_CHECK(d.N >= 1 && d.N <= EDGE_MAX_N, "edge: 1..64 nodes");
  TORCH_CHECK(W.size(0) == 2 * d.Cin, "edge: W must be [2 Cin,C]");
  TORCH_CHECK(bits.is_cuda() && bits.scalar_type() == at::kLong && bits.is_contiguous() &&
              bits.numel() == 2L * d.B * d.N, "edge: bits must be int64 [2,B,N]");
  TORCH_CHECK(pw.numel() == (long)d.B * d.N, "edge: pool weights must be [B,N]");
  TORCH_CHECK(bias.numel() == d.C, "edge: bias must be [C]");
  TORCH_CHECK(act >= GAT_ACT_LINEAR && act <= GAT_ACT_RELU, "edge: activation code");
  if (act == GAT_ACT_PRELU) {
    check_f32_cuda(alpha, "alpha");
    TORCH_CHECK(alpha.numel() == d.C, "edge: alpha must be [C]");
  }
  d.NP = gat_pow2(d.N);
  d.rpw = 256 / d.NP;
  return d;
}

static int edge_grid(long rows, int rpw) {
  return (int)std::max<long>(1, std::min<long>((rows + rpw - 1) / rpw, EDGE_GRID_CAP));
}

static const gat_bits_t* edge_bits_ptr(const at::Tensor& bits) {
  return reinterpret_cast<const gat_bits_t*>(bits.data_ptr<int64_t>());
}

at::Tensor edge_adj_bits(const at::Tensor& adj, const at::Tensor& mask) {
  check_f32_cuda(adj, "adj");
  check_f32_cuda(mask, "mask");
  TORCH_CHECK(adj.dim() == 3 && adj.size(1) == adj.size(2), "edge: adj must be [B,N,N]");
  const int B = adj.size(0), N = adj.size(1);
  TORCH_CHECK(N >= 1 && N <= EDGE_MAX_N, "edge: 1..64 nodes");
  TORCH_CHECK(mask.dim() == 2 && mask.size(0) == B && mask.size(1) == N, "edge: mask must be [B,N]");
  c10::DeviceGuard guard(adj.device());
  at::Tensor bits = at::empty({2, B, N}, adj.options().dtype(at::kLong));
  if (B == 0) return bits;
  hipLaunchKernelGGL(edge_adj_bits_kernel, dim3(((long)B * N + 255) / 256), dim3(256), 0, stream(),
                     adj.data_ptr<float>(), reinterpret_cast<gat_bits_t*>(bits.data_ptr<int64_t>()), B, N);
  GQ_LAUNCH_CHECK();
  return bits;
}

at::Tensor edge_pool_fwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& anom,
                         const at::Tensor& W, const at::Tensor& bias, const at::Tensor& alpha, int64_t act,
                         bool mean, int64_t Mp, int64_t Cp) {
  const EdgeDims d = edge_check(x, bits, pw, W, bias, alpha, act);
  int Ca = 0;
  if (anom.numel() > 0) {
    check_f32_cuda(anom, "anom");
    TORCH_CHECK(anom.dim() == 3 && anom.size(0) == d.B && anom.size(1) == d.T, "edge: anom must be [B,T,Ca]");
    Ca = anom.size(2);
  }
  const int Fo = Ca + d.C;
  TORCH_CHECK(Mp == 0 || (Mp >= d.B && Mp % 16 == 0 && Cp >= Fo), "edge_pool_fwd: time-major Mp / Cp");
  c10::DeviceGuard guard(x.device());
  at::Tensor out = Mp > 0 ? at::empty({d.T, Mp, Cp}, x.options()) : at::empty({d.B, d.T, Fo}, x.options());
  const long vrows = Mp > 0 ? (long)Mp * d.T : (long)d.B * d.T;
  if (vrows == 0) return out;
  const float* anom_p = Ca ? anom.data_ptr<float>() : nullptr;
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  GQ_EDGE_DISPATCH(d.Cin, d.C,
      hipLaunchKernelGGL((edge_pool_fwd_kernel<CIN, C>), dim3(edge_grid(vrows, d.rpw)), dim3(256), 0, stream(),
                         x.data_ptr<float>(), edge_bits_ptr(bits), pw.data_ptr<float>(), anom_p, W.data_ptr<float>(),
                         bias.data_ptr<float>(), al_p, out.data_ptr<float>(), d.B, d.T, d.N, d.NP, Ca, (int)act,
                         (int)mean, (int)Mp, Mp > 0 ? (int)Cp : Fo));
  GQ_LAUNCH_CHECK();
  return out;
}

static void edge_check_dout(const at::Tensor& dout, const EdgeDims& d, int64_t c_off, bool time_major) {
  check_f32_cuda(dout, "dout");
  TORCH_CHECK(dout.dim() == 3 && c_off >= 0 &&
              (time_major ? (dout.size(0) == d.T && dout.size(1) >= d.B && dout.size(2) >= c_off + d.C)
                          : (dout.size(0) == d.B && dout.size(1) == d.T && dout.size(2) >= c_off + d.C)),
              "edge: dout shape");
}

// the summed records [C / EDGE_CH, R] of the parameter gradients (see edge_pool_bwd_kernel)
at::Tensor edge_pool_bwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& dout,
                         const at::Tensor& W, const at::Tensor& bias, const at::Tensor& alpha, int64_t act,
                         bool mean, int64_t c_off, bool time_major) {
  const EdgeDims d = edge_check(x, bits, pw, W, bias, alpha, act);
  edge_check_dout(dout, d, c_off, time_major);
  c10::DeviceGuard guard(x.device());
  const int R = (2 * d.Cin + 2) * EDGE_CH, nch = d.C / EDGE_CH;
  const long rows = (long)d.B * d.T;
  if (rows == 0) return at::zeros({nch, R}, x.options());
  const int nblk = edge_grid(rows, d.rpw);
  at::Tensor partial = at::empty({nblk, nch, R}, x.options());
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  const gat_bits_t* bp = edge_bits_ptr(bits);
  GQ_EDGE_DISPATCH(d.Cin, d.C,
      hipLaunchKernelGGL((edge_pool_bwd_kernel<CIN, C>), dim3(nblk, nch), dim3(256), 0, stream(),
                         x.data_ptr<float>(), bp, bp + (long)d.B * d.N, pw.data_ptr<float>(), dout.data_ptr<float>(),
                         W.data_ptr<float>(), bias.data_ptr<float>(), al_p, partial.data_ptr<float>(), d.B, d.T, d.N,
                         d.NP, (int)act, (int)mean, (int)c_off, (int)dout.size(2),
                         time_major ? (int)dout.size(1) : 0));
  GQ_LAUNCH_CHECK();
  return nblk == 1 ? partial.view({nch, R}) : colsum(partial);       // fixed order: deterministic
}

static float* edge_sink(const at::Tensor& t, long n, const char* name) {
  if (t.numel() == 0) return nullptr;
  check_f32_cuda(t, name);
  TORCH_CHECK(t.numel() == n, "edge_bwd_finalize: ", name, " size");
  return t.data_ptr<float>();
}

void edge_bwd_finalize(const at::Tensor& tot, const at::Tensor& W, at::Tensor dW, at::Tensor dbias,
                       at::Tensor dalpha) {
  check_f32_cuda(tot, "tot");
  TORCH_CHECK(W.dim() == 2 && W.size(0) % 2 == 0 && W.size(1) % EDGE_CH == 0, "edge: W must be [2 Cin,C]");
  const int Cin = W.size(0) / 2, C = W.size(1);
  const int R = (2 * Cin + 2) * EDGE_CH;
  TORCH_CHECK(tot.numel() == (long)(C / EDGE_CH) * R, "edge_bwd_finalize: tot must be [C/8,R]");
  c10::DeviceGuard guard(tot.device());
  hipLaunchKernelGGL(edge_bwd_finalize_kernel, dim3(1), dim3(256), 0, stream(), tot.data_ptr<float>(), Cin, C,
                     edge_sink(dW, 2L * Cin * C, "dW"), edge_sink(dbias, C, "dbias"), edge_sink(dalpha, C, "dalpha"));
  GQ_LAUNCH_CHECK();
}

at::Tensor edge_pool_bwd_input(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw,
                               const at::Tensor& dout, const at::Tensor& W, const at::Tensor& bias,
                               const at::Tensor& alpha, int64_t act, bool mean, int64_t c_off, bool time_major) {
  const EdgeDims d = edge_check(x, bits, pw, W, bias, alpha, act);
  edge_check_dout(dout, d, c_off, time_major);
  c10::DeviceGuard guard(x.device());
  at::Tensor dx = at::empty_like(x);
  const long rows = (long)d.B * d.T;
  if (rows == 0) return dx;
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  const gat_bits_t* bp = edge_bits_ptr(bits);
  GQ_EDGE_DISPATCH(d.Cin, d.C,
      hipLaunchKernelGGL((edge_pool_bwd_input_kernel<CIN, C>), dim3(edge_grid(rows, d.rpw)), dim3(256), 0, stream(),
                         x.data_ptr<float>(), bp, bp + (long)d.B * d.N, pw.data_ptr<float>(), dout.data_ptr<float>(),
                         W.data_ptr<float>(), bias.data_ptr<float>(), al_p, dx.data_ptr<float>(), d.B, d.T, d.N, d.NP,
                         (int)act, (int)mean, (int)c_off, (int)dout.size(2), time_major ? (int)dout.size(1) : 0));
  GQ_LAUNCH_CHECK();
  return dx;
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("edge_adj_bits", &gq::edge_adj_bits);
  m.impl("edge_pool_fwd", &gq::edge_pool_fwd);
  m.impl("edge_pool_bwd", &gq::edge_pool_bwd);
  m.impl("edge_bwd_finalize", &gq::edge_bwd_finalize);
  m.impl("edge_pool_bwd_input", &gq::edge_pool_bwd_input);
}
