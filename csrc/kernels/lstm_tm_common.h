// Pieces shared by the time-major LSTM kernels (lstm_tm_fwd.hip, lstm_tm_bwd.hip, lstm_grads_jobs.hip,
// lstm_chain_fwd.hip, lstm_chain_bwd.hip, time4_head.hip): tile constants, streamers, the fused pool, and the host side's shape
// predicates with the dispatcher that turns a launch's run-time shape into template arguments.
#pragma once
#include "common.h"

#include <cstdlib>
#include <type_traits>
#include <utility>

#ifndef TM_RG_BF16H
#define TM_RG_BF16H 1    // recompute-gates pairs save layer A's h in bf16 (its only readers stage it as bf16; A/B: 0)
#endif
#ifndef TM_RG_BF16C
#define TM_RG_BF16C 1    // recompute-gates layers save c_t in bf16 (the forward keeps fp32 in registers; A/B: 0)
#endif

namespace gq {

// ---- host: a run-time value as a compile-time constant. f is a generic lambda called with
// std::integral_constant<int, V> (read it as decltype(v)::value); a value outside Vs... raises `what`.
template <int... Vs, class F>
void dispatch_int(int v, const char* what, F&& f) {
  const bool hit = ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  TORCH_CHECK(hit, what);
}
template <class F>
void dispatch_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
// several flags at once: f(c0, c1, ...) with std::true_type / std::false_type
template <class F>
void dispatch_bools(F&& f) { f(); }
template <class F, class... Bs>
void dispatch_bools(F&& f, bool b, Bs... bs) {
  dispatch_bool(b, [&](auto c) { dispatch_bools([&](auto... cs) { f(c, cs...); }, bs...); });
}

// ---- host: what the time-major kernels take. The TORCH_CHECKs of the entry points and the pruning of
// template instances (tm_combo_ok) are these same functions, so the two cannot drift apart.
inline int tm_granule(int Din, const void* x) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(x);
  if (Din % 4 == 0 && a % 16 == 0) return 4;
  if (Din % 2 == 0 && a % 8 == 0) return 2;
  return 1;
}

// H in {16, 32, 64}: one cell per lane, H / 4 waves. Larger hidden sizes keep the seq-major kernels of
// lstm.hip / lstm_grads.hip. The per-step x tile must fit the loader lanes and Din + 1 (bias row) must fit 128.
constexpr bool tm_supported(int H, int Din, int gr) {
  if (H != 16 && H != 32 && H != 64) return false;
  if (Din < 1 || Din > 127) return false;
  return 16 * Din / gr <= 16 * H;
}

// x channel blocks of 32 (KX); 3 runs as 4
constexpr int tm_kx(int Din) { return (Din + 31) / 32 <= 2 ? (Din + 31) / 32 : 4; }

// recompute-gates backward (lstm_tm_bwd_body RG): one cell per lane with the x / h streams of the
// fused weight-gradient kernel (H <= 32, 16-byte x granules)
constexpr bool tm_rg_ok(int H, int gr) { return (H == 16 || H == 32) && gr == 4; }

// some Din has KX channel blocks and passes tm_supported(H, Din, GR): only those (H, KX, GR) are instantiated
template <int H, int KX, int GR>
constexpr bool tm_combo_ok() {
  for (int Din = 1; Din <= 127; ++Din)
    if (tm_kx(Din) == KX && tm_supported(H, Din, GR)) return true;
  return false;
}

// (H, KX, GR) of a launch as constants: f(h, kx, gr). A triple no supported Din reaches ends in an error.
template <int... Hs, class F>
void tm_dispatch(int H, int Din, int gr, const char* what, F&& f) {
  dispatch_int<Hs...>(H, what, [&](auto h) {
    dispatch_int<1, 2, 4>(tm_kx(Din), "lstm_tm: x channel blocks", [&](auto kx) {
      dispatch_int<1, 2, 4>(gr, "lstm_tm: x granule", [&](auto g) {
        if constexpr (tm_combo_ok<decltype(h)::value, decltype(kx)::value, decltype(g)::value>()) f(h, kx, g);
        else TORCH_CHECK(false, "lstm_tm: no instance for (H, Din, granule) = (", H, ", ", Din, ", ", gr, ")");
      });
    });
  });
}

// GNNQC_TM_RECDX=0: multi-column-block layers take dx from weight-gradient slabs + their sum
// (the earlier layout) instead of from the recurrence
inline bool tm_rec_dx() {       // read per call (host side of a launch; tests toggle it)
  const char* e = std::getenv("GNNQC_TM_RECDX");
  return !(e != nullptr && e[0] == '0');
}

// Weight gradients inside the backward recurrence (lstm_tm_bwd_wg_kernel) for layers of at least
// GNNQC_TM_FUSED_WGRAD_MIN_TILES 16-sequence tiles (default 64: with few tiles the separate pass
// spreads the rows over the whole GPU, the recurrence's workgroups cannot); GNNQC_TM_FUSED_WGRAD=0
// turns it off. Read per call (tests switch them).
inline bool tm_fused_wgrad(int H, int Din, int gr, int ntiles) {
  const char* e = std::getenv("GNNQC_TM_FUSED_WGRAD");
  if (e != nullptr && e[0] == '0') return false;
  const char* m = std::getenv("GNNQC_TM_FUSED_WGRAD_MIN_TILES");
  const int min_tiles = m != nullptr ? std::atoi(m) : 64;
  return tm_rg_ok(H, gr) && Din <= 64 && ntiles >= min_tiles;
}

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

// Saved LSTM gates (i, f, g, o of one cell and step) are stored as 4 x bf16 = 8 bytes: the
// forward's largest stream and the backward's largest read (was 16 bytes of fp32). Gate
// activations lie in (0, 1) / (-1, 1), so bf16 keeps ~3 significant digits, the precision of
// the bf16 MFMA operands they are combined with.
__device__ __forceinline__ uint2 gates_pack(float i, float f, float g, float o) {
  const bf16x4_t v = bf16x4_t{(__bf16)i, (__bf16)f, (__bf16)g, (__bf16)o};
  return *reinterpret_cast<const uint2*>(&v);
}
__device__ __forceinline__ float4 gates_unpack(uint2 u) {
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}

// A wave-uniform predicate the compiler can SEE is uniform (an SGPR): branches on it are
// scalar, so no exec-mask join -> no conservative s_waitcnt vmcnt(0) around the loads
// inside (measured: with threadIdx-derived predicates every step drained the load ring).
__device__ __forceinline__ bool wave_uniform(bool p) { return __builtin_amdgcn_readfirstlane((int)p) != 0; }

template <int H>
struct TMC {
  static constexpr int CPL = H > 64 ? H / 64 : 1;   // cells per lane
  static constexpr int NW = H / (4 * CPL);          // waves per 16-sequence tile (<= 16)
  static constexpr int NT = 64 * NW;
  static constexpr int G4 = 4 * H;
  static constexpr int KPH = ((H + 31) / 32) * 32;
  static constexpr int KSH = KPH / 32;              // K = H steps (forward recurrent part)
  static constexpr int KB = G4 / 32;                // K = 4H steps (backward)
  static constexpr int HP = H + 4;                  // row pitch of fp32 [16][H] LDS tiles: the
                                                    // per-cell accesses (16 rows x 4 units per
                                                    // wave) then hit 64 distinct banks
};

// ---- tile streamer: granules of GR floats of one contiguous tile, wave-uniform loaders
template <int GR>
struct Granule {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    if constexpr (GR == 4) {
      const float4 a = *reinterpret_cast<const float4*>(p);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else if constexpr (GR == 2) {
      const float2 a = *reinterpret_cast<const float2*>(p);
      v[0] = a.x; v[1] = a.y;
    } else {
      v[0] = *p;
    }
  }
  __device__ __forceinline__ void zero() { v[0] = v[1] = v[2] = v[3] = 0.f; }
  __device__ __forceinline__ __bf16 bf(int q) const { return (__bf16)v[q]; }
};

// The same GR-element granule from bf16 data, kept as the raw bits: a ring slot's load is waited for
// where the value is used (staged into LDS as bf16), not at the load
template <int GR>
struct GranuleH {
  using R = std::conditional_t<GR == 4, uint2, std::conditional_t<GR == 2, unsigned, unsigned short>>;
  R r;
  __device__ __forceinline__ void load(const __bf16* p) { r = *reinterpret_cast<const R*>(p); }
  __device__ __forceinline__ __bf16 bf(int q) const {
    unsigned w;
    if constexpr (GR == 4) w = q < 2 ? r.x : r.y;
    else w = (unsigned)r;
    return __builtin_bit_cast(__bf16, (unsigned short)((q & 1) ? (w >> 16) : (w & 0xffffu)));
  }
};

// ---- fused MaxPooling1D(P) (valid, stride P) of a stored h sequence (the chain forward's last
// stage, lstm_chain_fwd.hip, whose pooled output leaves the chain). Each storer lane owns
// one float4 granule of the [16][H] tile for the whole sequence, so the running max and the
// byte argmax (first maximum wins, like TF's MaxPoolGrad) stay in its registers; the pooled
// granule and its 4 argmax bytes are written when a window closes. Layout = maxpool1d_fwd's
// on the time-major tensor: pooled [T/P][Mp][H] fp32, argmax [T/P][Mp][H] uint8.
struct PoolAcc {
  float4 m;
  unsigned idx;
  __device__ __forceinline__ void step(const float4& v, int t, int P, int To, float* __restrict__ pout,
                                       unsigned* __restrict__ iout, size_t off, size_t pstep) {
    const int r = t % P;                            // t, P wave-uniform: scalar branches
    if (r == 0) {
      m = v;
      idx = 0u;
    } else {
      const unsigned rb = (unsigned)r;
      if (v.x > m.x) { m.x = v.x; idx = (idx & 0xffffff00u) | rb; }
      if (v.y > m.y) { m.y = v.y; idx = (idx & 0xffff00ffu) | (rb << 8); }
      if (v.z > m.z) { m.z = v.z; idx = (idx & 0xff00ffffu) | (rb << 16); }
      if (v.w > m.w) { m.w = v.w; idx = (idx & 0x00ffffffu) | (rb << 24); }
    }
    if (r == P - 1 && t / P < To) {
      const size_t k = (size_t)(t / P);
      *reinterpret_cast<float4*>(pout + k * pstep + off) = m;
      iout[(k * pstep + off) / 4] = idx;
    }
  }
};

// fused-pool outputs of the chain forward (host)
struct TmPool {
  int P = 0;
  float* out = nullptr;
  unsigned* idx = nullptr;
};

inline TmPool tm_pool_outputs(int P, int T, int Mp, int H, const at::TensorOptions& opt, at::Tensor& pooled,
                              at::Tensor& pidx) {
  TmPool pl;
  if (P <= 0) {
    pooled = at::empty({0}, opt);
    pidx = at::empty({0}, opt.dtype(at::kByte));
    return pl;
  }
  TORCH_CHECK(P <= 255 && T / P >= 1, "lstm_tm: pool size must be 1..255 and <= T");
  pooled = at::empty({T / P, Mp, H}, opt);
  pidx = at::empty({T / P, Mp, H}, opt.dtype(at::kByte));
  pl.P = P;
  pl.out = pooled.data_ptr<float>();
  pl.idx = reinterpret_cast<unsigned*>(pidx.data_ptr<uint8_t>());
  return pl;
}

// ---- time4 (H = 128, Din <= 64) forward and backward A-fragment images (time4_head.hip's 512-thread layout:
// wave w of 8, cell cc of 4, lane = (quad, col)): U fragments [w][cc][s < 4][lane], then W
// fragments [w][cc][s < 2][lane], each 8 bf16. Gathering them from the [K][4H] weights touches 16
// cache lines per load instruction, so the chain forward's idle workgroups build this image once per
// step and the time4 kernel reads it with lane-contiguous 16-B loads.
constexpr int T4PK_U = 8 * 4 * 4 * 64;
constexpr int T4PK_W = 8 * 4 * 2 * 64;
constexpr int T4PK_N = T4PK_U + T4PK_W;
// backward image (time4_head.hip t4_head_bwd_kernel): U rows [w][s < 16][lane] = U[16w + col][32s + 8quad ..],
// then W rows [w][s < 8][lane] = W[16 (w & 3) + col][256 (w >> 2) + 32s + 8quad ..] (rows >= Dw zero)
constexpr int T4PK_BU = 8 * 16 * 64;
constexpr int T4PK_BW = 8 * 8 * 64;
constexpr int T4PK_ALL = T4PK_N + T4PK_BU + T4PK_BW;

__device__ __forceinline__ void t4_pack_one(int f, const float* __restrict__ U, const float* __restrict__ W, int Dw,
                                            bf16x8_t* __restrict__ out) {
  if (f >= T4PK_N) {                       // backward fragments: 8 contiguous floats per lane
    const int fb = f - T4PK_N;
    const bool isU = fb < T4PK_BU;
    const int f2 = isU ? fb : fb - T4PK_BU;
    const int lane = f2 & 63, col = lane & 15, quad = lane >> 4;
    const int s = isU ? (f2 >> 6) & 15 : (f2 >> 6) & 7;
    const int w = isU ? f2 >> 10 : f2 >> 9;
    const float* src;
    float m = 1.f;
    if (isU) {
      src = U + (size_t)(16 * w + col) * 512 + 32 * s + 8 * quad;
    } else {
      const int din = 16 * (w & 3) + col;
      m = din < Dw ? 1.f : 0.f;
      src = W + (size_t)min(din, Dw - 1) * 512 + 256 * (w >> 2) + 32 * s + 8 * quad;
    }
    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
    out[f] = bf16x8_t{(__bf16)(a.x * m), (__bf16)(a.y * m), (__bf16)(a.z * m), (__bf16)(a.w * m),
                      (__bf16)(b.x * m), (__bf16)(b.y * m), (__bf16)(b.z * m), (__bf16)(b.w * m)};
    return;
  }
  const bool isU = f < T4PK_U;
  const int f2 = isU ? f : f - T4PK_U;
  const int lane = f2 & 63;
  const int s = isU ? (f2 >> 6) & 3 : (f2 >> 6) & 1;
  const int cc = isU ? (f2 >> 8) & 3 : (f2 >> 7) & 3;
  const int w = isU ? f2 >> 10 : f2 >> 9;
  const int col = lane & 15, quad = lane >> 4;
  const int gi = w + 8 * cc, au = 4 * gi + (col >> 2), ag = col & 3;
  bf16x8_t v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 32 * s + 8 * quad + j;
    if (isU) v[j] = (__bf16)U[(size_t)k * 512 + ag * 128 + au];
    else v[j] = (__bf16)(W[(size_t)min(k, Dw - 1) * 512 + ag * 128 + au] * (k < Dw ? 1.f : 0.f));
  }
  out[f] = v;
}

}  // namespace gq
