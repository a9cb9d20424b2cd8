// Fused AGNNConv + node pooling + concat for the CML front end.
//
// spektral AGNNConv(trainable, aggregate in {sum, mean}) on a dense per-sample graph, followed by
// `timeseries_pooling` and Concatenate([flagged series, pooled]) (gnnqc/models/graphconv.py AGNNConv
// is the eager form). For a row (b, t) and node i with nb_i = { j : adj_ij > 0 }:
//
//   xn_i   = x_i / max(||x_i||, 1e-12)
//   att_ij = softmax_j(beta <xn_i, xn_j>) over nb_i            (row maximum subtracted)
//   r_i    = sum_j att_ij x_j                                    (the UN-normalised x_j)
//   o_i    = s_i r_i                                             s_i = 1 (sum) or 1 / max(deg_i, 1) (mean)
//   out    = [anom | sum_i pw_i act(o_i)]                        pw: node pool weights (mask included)
//
// The layer has no weight matrix: the parameters are the scalar beta and, with PReLU, Cin slopes,
// and the output width is the input width. No self loop is added and the mask is not folded into
// the neighbour words (an edge towards a masked node counts, as in the eager layer); the words are
// edge_adj_bits' (edge.hip). Nothing of size [B, T, N, N] is stored: the backward kernels recompute
// xn, the scores and the softmax. Mapping (all three kernels, as in gat.hip / edge.hip): one lane
// per (row = (b, t), node i); a row's NP = pow2 >= N lanes are adjacent lanes of one wave, so the
// node pool is a shuffle reduction; a lane walks the set bits of its node's 64-bit neighbour word.
// Hence N <= 64.
//
// LDS: a row's x_j and xn_j are staged once per row block, one 16-byte-aligned slab per node.
// Cin <= 2 packs [x | xn] into ONE float4 (pitch 4 floats); Cin 3, 4 use [x(4) | xn(4)] at edge.hip's
// pitch of 12 floats. Argued from the ds_read_b128 banking (16 lanes per LDS cycle, 64 dword banks =
// sixteen 16-byte slots): node j sits on slot j mod 16 (pitch 4) or 3 j mod 16 (pitch 12), both
// bijections of j mod 16, so 16 consecutive nodes never share a slot. The reads are gathers by
// neighbour index, so that is the most a pitch can give: two lanes of a group collide only when
// they read different nodes 16 apart (or, for NP <= 16, the same node of different rows).
//
// Backward: u_i = act'(o_i) pw_i s_i dout (a Cin-vector), ds_ij = att_ij (<u_i, x_j> - <u_i, r_i>).
// agnn_pool_bwd keeps [dbeta | dalpha[Cin]] in registers over the workgroup's passes and writes ONE
// record per workgroup; a fixed-order column sum and agnn_bwd_finalize follow. agnn_pool_bwd_input
// needs row i's softmax statistics when node k is visited through the transposed word: phase 1 puts
// every node's (max, 1 / normaliser, <u, r>, u) into LDS, phase 2 gathers over the lane's own word
// and its transposed word, so each dx element is written by exactly one lane. No float atomics
// anywhere: results are bitwise reproducible.
//
// The norm is sqrtf(sum x^2) without scaling: an x whose squares underflow (|x| below about 1e-19)
// takes the clamp branch where the exact norm would not. No test pins that corner.
#include "gat_common.h"

namespace gq {

constexpr int AGNN_MAX_N = 64;
constexpr int AGNN_GRID_CAP = 256;       // workgroups per launch: more rows take several passes
constexpr int AGNN_STAT_PITCH = 12;      // floats per node of the phase-1 statistics (8 used)
constexpr float AGNN_EPS = 1e-12f;       // F.normalize's clamp

// A node's slab in LDS: x and xn, read back as whole float4s
template <int CIN>
struct AgnnSlab {
  static constexpr bool PACKED = CIN <= 2;
  static constexpr int PITCH = PACKED ? 4 : 12;
  static __device__ __forceinline__ void put(float* s, const float (&x)[CIN], const float (&xn)[CIN]) {
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (PACKED) {
#pragma unroll
      for (int f = 0; f < CIN; ++f) a[f] = x[f], a[2 + f] = xn[f];
      reinterpret_cast<float4*>(s)[0] = make_float4(a[0], a[1], a[2], a[3]);
    } else {
#pragma unroll
      for (int f = 0; f < CIN; ++f) a[f] = x[f], b[f] = xn[f];
      reinterpret_cast<float4*>(s)[0] = make_float4(a[0], a[1], a[2], a[3]);
      reinterpret_cast<float4*>(s)[1] = make_float4(b[0], b[1], b[2], b[3]);
    }
  }
  static __device__ __forceinline__ void get_xn(const float* s, float (&xn)[CIN]) {
    const float4 v = reinterpret_cast<const float4*>(s)[PACKED ? 0 : 1];
    const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int f = 0; f < CIN; ++f) xn[f] = a[PACKED ? 2 + f : f];
  }
  static __device__ __forceinline__ void get(const float* s, float (&x)[CIN], float (&xn)[CIN]) {
    const float4 v = reinterpret_cast<const float4*>(s)[0];
    const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int f = 0; f < CIN; ++f) x[f] = a[f];
    if constexpr (PACKED) {
#pragma unroll
      for (int f = 0; f < CIN; ++f) xn[f] = a[2 + f];
    } else {
      get_xn(s, xn);
    }
  }
};

template <int CIN>
__device__ __forceinline__ float agnn_dot(const float (&a)[CIN], const float (&b)[CIN]) {
  float d = a[0] * b[0];
#pragma unroll
  for (int f = 1; f < CIN; ++f) d += a[f] * b[f];
  return d;
}

// The score beta <xn_i, xn_j>, rounded as a product of its own (no contraction into the subtraction
// of the row maximum): every walk gets the same number, so the maximum's term is exp(0) = 1 exactly.
template <int CIN>
__device__ __forceinline__ float agnn_score(float beta, const float (&a)[CIN], const float (&b)[CIN]) {
  return __fmul_rn(beta, agnn_dot<CIN>(a, b));
}

// The lane's node of its row: x_i, xn_i, ||x_i||, the neighbour words, the pool weight pw_i (0: the
// node adds nothing to the pooled output) and sd = s_i. Lanes past the row's nodes or past the last
// row hold zeros.
template <int CIN>
struct AgnnNode {
  float x[CIN], xn[CIN];
  float nrm, pw, sd;
  gat_bits_t nb, nbT;
  bool real;
};

template <int CIN>
__device__ __forceinline__ AgnnNode<CIN> agnn_node(const float* __restrict__ x, const gat_bits_t* __restrict__ bits,
                                                   const gat_bits_t* __restrict__ bitsT,
                                                   const float* __restrict__ pw, long row, long rows, int i, int T,
                                                   int N, int mean) {
  AgnnNode<CIN> n;
  n.real = row < rows && i < N;
  n.nrm = n.pw = 0.f;
  n.sd = 1.f;
  n.nb = n.nbT = 0;
#pragma unroll
  for (int f = 0; f < CIN; ++f) n.x[f] = n.xn[f] = 0.f;
  if (n.real) {
    const long bn = (row / T) * N + i;
    const gat_bits_t valid = N == 64 ? ~0ull : (1ull << N) - 1;      // (a neighbour index stays inside the row's slabs)
    n.nb = bits[bn] & valid;
    if (bitsT != nullptr) n.nbT = bitsT[bn] & valid;
    n.pw = pw[bn];
    if (mean) n.sd = 1.f / (float)max(__popcll(n.nb), 1);
    float ss = 0.f;
#pragma unroll
    for (int f = 0; f < CIN; ++f) {
      n.x[f] = x[(row * N + i) * CIN + f];
      ss += n.x[f] * n.x[f];
    }
    n.nrm = sqrtf(ss);
    const float d = fmaxf(n.nrm, AGNN_EPS);
#pragma unroll
    for (int f = 0; f < CIN; ++f) n.xn[f] = n.x[f] / d;
  }
  return n;
}

// Softmax statistics of node i over its neighbour word: m = max_j beta <xn_i, xn_j>, l = sum_j e_ij,
// r = sum_j e_ij x_j with e_ij = exp(beta <xn_i, xn_j> - m). Two walks: the scores are bounded by
// |beta|, but a constant shift by |beta| would underflow every term for a large beta. An empty word
// gives l = 0.
template <int CIN>
__device__ __forceinline__ void agnn_softmax(gat_bits_t nb, const float (&xni)[CIN], float beta, const float* sr,
                                             float& m, float& l, float (&r)[CIN]) {
  using S = AgnnSlab<CIN>;
  m = -INFINITY;
  for (gat_bits_t w = nb; w; w &= w - 1) {
    const int j = __ffsll((long long)w) - 1;
    float xnj[CIN];
    S::get_xn(sr + j * S::PITCH, xnj);
    m = fmaxf(m, agnn_score<CIN>(beta, xni, xnj));
  }
  l = 0.f;
#pragma unroll
  for (int f = 0; f < CIN; ++f) r[f] = 0.f;
  for (gat_bits_t w = nb; w; w &= w - 1) {
    const int j = __ffsll((long long)w) - 1;
    float xj[CIN], xnj[CIN];
    S::get(sr + j * S::PITCH, xj, xnj);
    const float e = __expf(agnn_score<CIN>(beta, xni, xnj) - m);
    l += e;
#pragma unroll
    for (int f = 0; f < CIN; ++f) r[f] += e * xj[f];
  }
}

// ------------------------------------------------------------------ forward
// out: Mp > 0: time-major LSTM input [T][Mp][Cp] (rows b >= B and channels >= Ca + CIN zero), else
// [B][T][Ca + CIN] (the host passes Cp = Ca + CIN then). pw [B][N]: node pool weights (mask
// included: a masked node has weight 0).
template <int CIN>
__global__ __launch_bounds__(256) void agnn_pool_fwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const float* __restrict__ pw,
    const float* __restrict__ anom, const float* __restrict__ betap, const float* __restrict__ alpha,
    float* __restrict__ out, int B, int T, int N, int NP, int Ca, int act, int mean, int Mp, int Cp) {
  using S = AgnnSlab<CIN>;
  __shared__ __align__(16) float sx[256 * S::PITCH];
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const int Fo = Ca + CIN;
  const long rows = (long)B * T;
  const long vrows = Mp > 0 ? (long)Mp * T : rows;        // virtual rows incl. zero padding rows
  const float beta = betap[0];
  float al[CIN];
#pragma unroll
  for (int f = 0; f < CIN; ++f) al[f] = act == GAT_ACT_PRELU ? alpha[f] : 0.f;
  const float* sr = sx + rl * NP * S::PITCH;
  for (long row0 = (long)blockIdx.x * rpw; row0 < vrows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const AgnnNode<CIN> n = agnn_node<CIN>(x, bits, nullptr, pw, row, rows, i, T, N, mean);
    __syncthreads();                              // the previous pass's readers are done
    S::put(sx + tid * S::PITCH, n.x, n.xn);
    __syncthreads();
    float acc[CIN];
#pragma unroll
    for (int f = 0; f < CIN; ++f) acc[f] = 0.f;
    if (n.pw != 0.f) {
      float m, l, r[CIN];
      agnn_softmax<CIN>(n.nb, n.xn, beta, sr, m, l, r);
      const float il = l > 0.f ? 1.f / l : 0.f;     // (o_i exactly as agnn_node_bwd forms it)
#pragma unroll
      for (int f = 0; f < CIN; ++f) acc[f] = n.pw * gat_act(r[f] * il * n.sd, al[f], act);
    }
    // node pool: sum over the row's NP lanes (every lane of the wave takes part)
    for (int o = NP >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int f = 0; f < CIN; ++f) acc[f] += __shfl_xor(acc[f], o, 64);
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
      for (int f = 0; f < CIN; ++f) op[Ca + f] = acc[f];
    }
    for (int c = Fo + i; c < Cp; c += NP) op[c] = 0.f;
  }
}

// ------------------------------------------------------------------ backward, shared part
// Node i's softmax statistics and upstream gradient: m, il = 1 / l (0: no neighbour, or the node
// adds nothing to the output), u = act'(o_i) pw_i s_i G, cu = <u, r_i> and o = o_i. G: the row's
// upstream gradient on the layer's channels.
template <int CIN>
__device__ __forceinline__ void agnn_node_bwd(const AgnnNode<CIN>& n, float beta, const float (&al)[CIN], int act,
                                              const float (&G)[CIN], const float* sr, float& m, float& il,
                                              float (&u)[CIN], float& cu, float (&o)[CIN]) {
  m = il = cu = 0.f;
#pragma unroll
  for (int f = 0; f < CIN; ++f) u[f] = o[f] = 0.f;
  if (n.pw == 0.f) return;
  float l, r[CIN];
  agnn_softmax<CIN>(n.nb, n.xn, beta, sr, m, l, r);
  if (!(l > 0.f)) {
    m = 0.f;
    return;
  }
  il = 1.f / l;
#pragma unroll
  for (int f = 0; f < CIN; ++f) {
    r[f] *= il;
    o[f] = r[f] * n.sd;
    u[f] = gat_act_grad(o[f], al[f], act) * n.pw * n.sd * G[f];
  }
  cu = agnn_dot<CIN>(u, r);                       // (the form of <u, x_j>: one neighbour gives ds = 0 exactly)
}

// ------------------------------------------------------------------ backward (parameters)
// partial [gridDim.x][R], R = 1 + CIN: dbeta | dalpha[CIN]. dout: [B][T][dstride], or time-major
// [T][dmp][dstride] when dmp > 0; the layer's channels start at c_off.
template <int CIN>
__global__ __launch_bounds__(256) void agnn_pool_bwd_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const float* __restrict__ pw,
    const float* __restrict__ dout, const float* __restrict__ betap, const float* __restrict__ alpha,
    float* __restrict__ partial, int B, int T, int N, int NP, int act, int mean, int c_off, int dstride, int dmp) {
  using S = AgnnSlab<CIN>;
  constexpr int R = 1 + CIN;
  __shared__ __align__(16) float sx[256 * S::PITCH];
  __shared__ float red[4][R];
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const long rows = (long)B * T;
  const float beta = betap[0];
  float al[CIN], aal[CIN], ab = 0.f;
#pragma unroll
  for (int f = 0; f < CIN; ++f) {
    al[f] = act == GAT_ACT_PRELU ? alpha[f] : 0.f;
    aal[f] = 0.f;
  }
  const float* sr = sx + rl * NP * S::PITCH;
  for (long row0 = (long)blockIdx.x * rpw; row0 < rows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const AgnnNode<CIN> n = agnn_node<CIN>(x, bits, nullptr, pw, row, rows, i, T, N, mean);
    __syncthreads();                              // the previous pass's readers are done
    S::put(sx + tid * S::PITCH, n.x, n.xn);
    __syncthreads();
    if (n.pw == 0.f) continue;                    // (no barrier or shuffle below in the loop)
    const long dro = dmp > 0 ? ((row % T) * (long)dmp + row / T) * dstride : row * (long)dstride;
    float G[CIN], u[CIN], o[CIN], m, il, cu;
#pragma unroll
    for (int f = 0; f < CIN; ++f) G[f] = dout[dro + c_off + f];
    agnn_node_bwd<CIN>(n, beta, al, act, G, sr, m, il, u, cu, o);
    if (act == GAT_ACT_PRELU) {
#pragma unroll
      for (int f = 0; f < CIN; ++f) aal[f] += o[f] > 0.f ? 0.f : o[f] * n.pw * G[f];
    }
    if (il == 0.f) continue;
    float db = 0.f;
    for (gat_bits_t w = n.nb; w; w &= w - 1) {
      const int j = __ffsll((long long)w) - 1;
      float xj[CIN], xnj[CIN];
      S::get(sr + j * S::PITCH, xj, xnj);
      const float c = agnn_dot<CIN>(n.xn, xnj);
      const float att = __expf(__fmul_rn(beta, c) - m) * il;
      db += att * (agnn_dot<CIN>(u, xj) - cu) * c;
    }
    ab += db;
  }
  // the workgroup's record: wave sums by shuffles, then the 4 wave partials in order
  const int lane = tid & 63, wv = tid >> 6;
  auto put = [&](int e, float v) {
    v = wave_sum(v);
    if (lane == 0) red[wv][e] = v;
  };
  put(0, ab);
#pragma unroll
  for (int f = 0; f < CIN; ++f) put(1 + f, aal[f]);
  __syncthreads();
  if (tid < R) partial[(long)blockIdx.x * R + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// tot [1 + CIN]: the summed records. Adds dbeta and dalpha into the gradient buffers (nullptr: not
// needed); a non-finite value that goes into one raises the step's non-finite flag (chain control
// word 7), like the other gradient producers.
__global__ __launch_bounds__(64) void agnn_bwd_finalize_kernel(const float* __restrict__ tot, int CIN,
                                                               float* __restrict__ dbeta,
                                                               float* __restrict__ dalpha, int* nf) {
  const int e = threadIdx.x;
  if (e > CIN) return;
  float* dst = e == 0 ? dbeta : (dalpha != nullptr ? dalpha + (e - 1) : nullptr);
  if (dst == nullptr) return;
  const float v = tot[e];
  *dst += v;
  if (!isfinite(v)) __hip_atomic_store(nf, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ backward (input)
// dx_k = sum_{i: k in nb_i} att_ik u_i                                   (aggregate path)
//      + d normalize(x_k) applied to dxn_k,                              (score path)
// dxn_k = beta (sum_{j in nb_k} ds_kj xn_j + sum_{i: k in nb_i} ds_ik xn_i).
// Every dx element is written by exactly one lane: no atomics. Masked nodes that are someone's
// neighbour receive their gradient through the transposed word, as in the eager layer.
template <int CIN>
__global__ __launch_bounds__(256) void agnn_pool_bwd_input_kernel(
    const float* __restrict__ x, const gat_bits_t* __restrict__ bits, const gat_bits_t* __restrict__ bitsT,
    const float* __restrict__ pw, const float* __restrict__ dout, const float* __restrict__ betap,
    const float* __restrict__ alpha, float* __restrict__ dx, int B, int T, int N, int NP, int act, int mean,
    int c_off, int dstride, int dmp) {
  using S = AgnnSlab<CIN>;
  __shared__ __align__(16) float sx[256 * S::PITCH];
  __shared__ __align__(16) float sst[256 * AGNN_STAT_PITCH];      // m, il, cu, - | u[4]
  const int tid = threadIdx.x, i = tid & (NP - 1), rl = tid / NP, rpw = 256 / NP;
  const long rows = (long)B * T;
  const float beta = betap[0];
  float al[CIN];
#pragma unroll
  for (int f = 0; f < CIN; ++f) al[f] = act == GAT_ACT_PRELU ? alpha[f] : 0.f;
  const float* sr = sx + rl * NP * S::PITCH;
  const float* str = sst + rl * NP * AGNN_STAT_PITCH;
  for (long row0 = (long)blockIdx.x * rpw; row0 < rows; row0 += (long)gridDim.x * rpw) {
    const long row = row0 + rl;
    const AgnnNode<CIN> n = agnn_node<CIN>(x, bits, bitsT, pw, row, rows, i, T, N, mean);
    __syncthreads();                              // the previous pass's readers are done
    S::put(sx + tid * S::PITCH, n.x, n.xn);
    __syncthreads();
    // phase 1: this node's softmax statistics and u into LDS
    float G[CIN], u[CIN], o[CIN], m, il, cu;
#pragma unroll
    for (int f = 0; f < CIN; ++f) G[f] = 0.f;
    if (n.pw != 0.f) {
      const long dro = dmp > 0 ? ((row % T) * (long)dmp + row / T) * dstride : row * (long)dstride;
#pragma unroll
      for (int f = 0; f < CIN; ++f) G[f] = dout[dro + c_off + f];
    }
    agnn_node_bwd<CIN>(n, beta, al, act, G, sr, m, il, u, cu, o);
    {
      float uu[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int f = 0; f < CIN; ++f) uu[f] = u[f];
      float4* st = reinterpret_cast<float4*>(sst + tid * AGNN_STAT_PITCH);
      st[0] = make_float4(m, il, cu, 0.f);
      st[1] = make_float4(uu[0], uu[1], uu[2], uu[3]);
    }
    __syncthreads();
    if (!n.real) continue;                        // (no barrier or shuffle below in the loop)
    // phase 2: gather over the own word (this node as i) and the transposed word (this node as k)
    float dxk[CIN], dxn[CIN];
#pragma unroll
    for (int f = 0; f < CIN; ++f) dxk[f] = dxn[f] = 0.f;
    if (il != 0.f) {
      for (gat_bits_t w = n.nb; w; w &= w - 1) {
        const int j = __ffsll((long long)w) - 1;
        float xj[CIN], xnj[CIN];
        S::get(sr + j * S::PITCH, xj, xnj);
        const float att = __expf(agnn_score<CIN>(beta, n.xn, xnj) - m) * il;
        const float ds = att * (agnn_dot<CIN>(u, xj) - cu);
#pragma unroll
        for (int f = 0; f < CIN; ++f) dxn[f] += ds * xnj[f];
      }
    }
    for (gat_bits_t w = n.nbT; w; w &= w - 1) {
      const int s = __ffsll((long long)w) - 1;    // node s has this lane's node as a neighbour
      const float4* st = reinterpret_cast<const float4*>(str + s * AGNN_STAT_PITCH);
      const float4 a = st[0];
      if (a.y == 0.f) continue;
      const float4 b = st[1];
      const float ub[4] = {b.x, b.y, b.z, b.w};
      float us[CIN], xns[CIN];
#pragma unroll
      for (int f = 0; f < CIN; ++f) us[f] = ub[f];
      S::get_xn(sr + s * S::PITCH, xns);
      const float att = __expf(agnn_score<CIN>(beta, xns, n.xn) - a.x) * a.y;
      const float ds = att * (agnn_dot<CIN>(us, n.x) - a.z);
#pragma unroll
      for (int f = 0; f < CIN; ++f) {
        dxk[f] += att * us[f];
        dxn[f] += ds * xns[f];
      }
    }
    // through xn = x / max(||x||, eps): the clamp is a constant below eps
    if (n.nrm >= AGNN_EPS) {
      float p = 0.f;
#pragma unroll
      for (int f = 0; f < CIN; ++f) p += n.xn[f] * dxn[f];
      const float q = beta / n.nrm;
#pragma unroll
      for (int f = 0; f < CIN; ++f) dxk[f] += (dxn[f] - n.xn[f] * p) * q;
    } else {
#pragma unroll
      for (int f = 0; f < CIN; ++f) dxk[f] += beta * dxn[f] / AGNN_EPS;
    }
#pragma unroll
    for (int f = 0; f < CIN; ++f) dx[(row * N + i) * CIN + f] = dxk[f];
  }
}

// ------------------------------------------------------------------ instance table
#define GQ_AGNN_DISPATCH(CIN_RT, ...)                       \
  switch (CIN_RT) {                                         \
    case 1: { constexpr int CIN = 1; __VA_ARGS__; } break;  \
    case 2: { constexpr int CIN = 2; __VA_ARGS__; } break;  \
    case 3: { constexpr int CIN = 3; __VA_ARGS__; } break;  \
    case 4: { constexpr int CIN = 4; __VA_ARGS__; } break;  \
    default: TORCH_CHECK(false, "agnn: Cin 1..4");          \
  }

// ------------------------------------------------------------------ host
struct AgnnDims {
  int B, T, N, Cin, NP, rpw;
};

// shapes shared by the three kernels: x [B,T,N,Cin], bits [2,B,N], pw [B,N], beta [1], alpha [Cin]
// or empty
static AgnnDims agnn_check(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& beta,
                           const at::Tensor& alpha, int64_t act) {
  for (auto* p : {&x, &pw, &beta}) check_f32_cuda(*p, "agnn input");
  TORCH_CHECK(x.dim() == 4, "agnn: x must be [B,T,N,Cin]");
  AgnnDims d;
  d.B = x.size(0), d.T = x.size(1), d.N = x.size(2), d.Cin = x.size(3);
  TORCH_CHECK(d.N >= 1 && d.N <= AGNN_MAX_N, "agnn: 1..64 nodes");
  TORCH_CHECK(d.Cin >= 1 && d.Cin <= 4, "agnn: Cin 1..4");
  TORCH_CHECK(bits.is_cuda() && bits.scalar_type() == at::kLong && bits.is_contiguous() &&
              bits.numel() == 2L * d.B * d.N, "agnn: bits must be int64 [2,B,N]");
  TORCH_CHECK(pw.numel() == (long)d.B * d.N, "agnn: pool weights must be [B,N]");
  TORCH_CHECK(beta.numel() == 1, "agnn: beta must be [1]");
  TORCH_CHECK(act >= GAT_ACT_LINEAR && act <= GAT_ACT_RELU, "agnn: activation code");
  if (act == GAT_ACT_PRELU) {
    check_f32_cuda(alpha, "alpha");
    TORCH_CHECK(alpha.numel() == d.Cin, "agnn: alpha must be [Cin]");
  }
  d.NP = gat_pow2(d.N);
  d.rpw = 256 / d.NP;
  return d;
}

static int agnn_grid(long rows, int rpw) {
  return (int)std::max<long>(1, std::min<long>((rows + rpw - 1) / rpw, AGNN_GRID_CAP));
}

static const gat_bits_t* agnn_bits_ptr(const at::Tensor& bits) {
  return reinterpret_cast<const gat_bits_t*>(bits.data_ptr<int64_t>());
}

at::Tensor agnn_pool_fwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& anom,
                         const at::Tensor& beta, const at::Tensor& alpha, int64_t act, bool mean, int64_t Mp,
                         int64_t Cp) {
  const AgnnDims d = agnn_check(x, bits, pw, beta, alpha, act);
  int Ca = 0;
  if (anom.numel() > 0) {
    check_f32_cuda(anom, "anom");
    TORCH_CHECK(anom.dim() == 3 && anom.size(0) == d.B && anom.size(1) == d.T, "agnn: anom must be [B,T,Ca]");
    Ca = anom.size(2);
  }
  const int Fo = Ca + d.Cin;
  TORCH_CHECK(Mp == 0 || (Mp >= d.B && Mp % 16 == 0 && Cp >= Fo), "agnn_pool_fwd: time-major Mp / Cp");
  c10::DeviceGuard guard(x.device());
  at::Tensor out = Mp > 0 ? at::empty({d.T, Mp, Cp}, x.options()) : at::empty({d.B, d.T, Fo}, x.options());
  const long vrows = Mp > 0 ? (long)Mp * d.T : (long)d.B * d.T;
  if (vrows == 0) return out;
  const float* anom_p = Ca ? anom.data_ptr<float>() : nullptr;
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  GQ_AGNN_DISPATCH(d.Cin,
      hipLaunchKernelGGL((agnn_pool_fwd_kernel<CIN>), dim3(agnn_grid(vrows, d.rpw)), dim3(256), 0, stream(),
                         x.data_ptr<float>(), agnn_bits_ptr(bits), pw.data_ptr<float>(), anom_p,
                         beta.data_ptr<float>(), al_p, out.data_ptr<float>(), d.B, d.T, d.N, d.NP, Ca, (int)act,
                         (int)mean, (int)Mp, Mp > 0 ? (int)Cp : Fo));
  GQ_LAUNCH_CHECK();
  return out;
}

static void agnn_check_dout(const at::Tensor& dout, const AgnnDims& d, int64_t c_off, bool time_major) {
  check_f32_cuda(dout, "dout");
  TORCH_CHECK(dout.dim() == 3 && c_off >= 0 &&
              (time_major ? (dout.size(0) == d.T && dout.size(1) >= d.B && dout.size(2) >= c_off + d.Cin)
                          : (dout.size(0) == d.B && dout.size(1) == d.T && dout.size(2) >= c_off + d.Cin)),
              "agnn: dout shape");
}

// the summed record [1 + Cin] of the parameter gradients (see agnn_pool_bwd_kernel)
at::Tensor agnn_pool_bwd(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw, const at::Tensor& dout,
                         const at::Tensor& beta, const at::Tensor& alpha, int64_t act, bool mean, int64_t c_off,
                         bool time_major) {
  const AgnnDims d = agnn_check(x, bits, pw, beta, alpha, act);
  agnn_check_dout(dout, d, c_off, time_major);
  c10::DeviceGuard guard(x.device());
  const int R = 1 + d.Cin;
  const long rows = (long)d.B * d.T;
  if (rows == 0) return at::zeros({R}, x.options());
  const int nblk = agnn_grid(rows, d.rpw);
  at::Tensor partial = at::empty({nblk, R}, x.options());
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  GQ_AGNN_DISPATCH(d.Cin,
      hipLaunchKernelGGL((agnn_pool_bwd_kernel<CIN>), dim3(nblk), dim3(256), 0, stream(), x.data_ptr<float>(),
                         agnn_bits_ptr(bits), pw.data_ptr<float>(), dout.data_ptr<float>(), beta.data_ptr<float>(),
                         al_p, partial.data_ptr<float>(), d.B, d.T, d.N, d.NP, (int)act, (int)mean, (int)c_off,
                         (int)dout.size(2), time_major ? (int)dout.size(1) : 0));
  GQ_LAUNCH_CHECK();
  return nblk == 1 ? partial.view({R}) : colsum(partial);            // fixed order: deterministic
}

static float* agnn_sink(const at::Tensor& t, long n, const char* name) {
  if (t.numel() == 0) return nullptr;
  check_f32_cuda(t, name);
  TORCH_CHECK(t.numel() == n, "agnn_bwd_finalize: ", name, " size");
  return t.data_ptr<float>();
}

void agnn_bwd_finalize(const at::Tensor& tot, at::Tensor dbeta, at::Tensor dalpha) {
  check_f32_cuda(tot, "tot");
  const int Cin = (int)tot.numel() - 1;
  TORCH_CHECK(tot.dim() == 1 && Cin >= 1 && Cin <= 4, "agnn_bwd_finalize: tot must be [1 + Cin]");
  c10::DeviceGuard guard(tot.device());
  hipLaunchKernelGGL(agnn_bwd_finalize_kernel, dim3(1), dim3(64), 0, stream(), tot.data_ptr<float>(), Cin,
                     agnn_sink(dbeta, 1, "dbeta"), agnn_sink(dalpha, Cin, "dalpha"), chain_ctl(tot.get_device()) + 7);
  GQ_LAUNCH_CHECK();
}

at::Tensor agnn_pool_bwd_input(const at::Tensor& x, const at::Tensor& bits, const at::Tensor& pw,
                               const at::Tensor& dout, const at::Tensor& beta, const at::Tensor& alpha, int64_t act,
                               bool mean, int64_t c_off, bool time_major) {
  const AgnnDims d = agnn_check(x, bits, pw, beta, alpha, act);
  agnn_check_dout(dout, d, c_off, time_major);
  c10::DeviceGuard guard(x.device());
  at::Tensor dx = at::empty_like(x);
  const long rows = (long)d.B * d.T;
  if (rows == 0) return dx;
  const float* al_p = act == GAT_ACT_PRELU ? alpha.data_ptr<float>() : nullptr;
  const gat_bits_t* bp = agnn_bits_ptr(bits);
  GQ_AGNN_DISPATCH(d.Cin,
      hipLaunchKernelGGL((agnn_pool_bwd_input_kernel<CIN>), dim3(agnn_grid(rows, d.rpw)), dim3(256), 0, stream(),
                         x.data_ptr<float>(), bp, bp + (long)d.B * d.N, pw.data_ptr<float>(), dout.data_ptr<float>(),
                         beta.data_ptr<float>(), al_p, dx.data_ptr<float>(), d.B, d.T, d.N, d.NP, (int)act, (int)mean,
                         (int)c_off, (int)dout.size(2), time_major ? (int)dout.size(1) : 0));
  GQ_LAUNCH_CHECK();
  return dx;
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("agnn_pool_fwd", &gq::agnn_pool_fwd);
  m.impl("agnn_pool_bwd", &gq::agnn_pool_bwd);
  m.impl("agnn_bwd_finalize", &gq::agnn_bwd_finalize);
  m.impl("agnn_pool_bwd_input", &gq::agnn_pool_bwd_input);
}
