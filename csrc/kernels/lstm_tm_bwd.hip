// Time-major LSTM backward of one layer for gfx950 (lstm_tm_bwd): the reverse recurrence of
// lstm_tm_bwd_body.h as two kernels, and the host side that picks what the recurrence produces itself and
// what a pass over all T*Mp rows (lstm_grads.hip) produces from its dz.
//
// The paths of lstm_tm_bwd, in the order the host tries them:
//   fused weight gradients   (weight gradients wanted, and recomputed gates or tm_fused_wgrad: H <= 32, Din <= 64,
//                            16-byte granules, enough tiles) lstm_tm_bwd_wg_kernel: dW / dU / db accumulate in
//                            VGPRs over all T steps and leave as one split record per tile, summed by
//                            lstm_grads_reduce_records; dx (if wanted) comes from the same kernel; dz never
//                            reaches HBM.
//   rec-dx + rows pass       (weight gradients and dx wanted, several gate-column blocks: H >= 32, GNNQC_TM_RECDX
//                            not 0) lstm_tm_bwd_kernel<DZ, DX> writes dz and dx; lstm_grads_rows adds dW / dU / db.
//   rows pass with slabs     (any other layer with weight gradients) lstm_tm_bwd_kernel<DZ> writes dz only;
//                            lstm_grads_rows adds dW / dU / db and writes dx as one slab per column block, summed
//                            here. A pooled gradient is un-pooled by maxpool1d_bwd first.
//   frozen, recomputed gates (no weight gradients, empty g) lstm_tm_bwd_kernel<DX, RG> writes dx.
//   frozen, saved gates      (no weight gradients) lstm_tm_bwd_kernel<DX> writes dx.
// Every recurrence but the rows pass with slabs un-pools a pooled gradient on load (UP; 16-byte granules).
//
// The host turns (H, x channel blocks, x granule) and the flags into template arguments with tm_dispatch /
// dispatch_bools (lstm_tm_common.h); a combination the kernels forbid or no supported shape reaches ends in
// an error instead of an instance.
#include "common.h"

#include "lstm_grads_body.h"
#include "lstm_tm_bwd_body.h"
#include "lstm_tm_common.h"

namespace gq {

template <int H, int KX, int GR, int D, bool DZ, bool DX, bool LAST, bool RG = false, bool UP = false,
          bool XB = false, bool HB = false>
__global__ __launch_bounds__(TMC<H>::NT) void lstm_tm_bwd_kernel(
    const float* __restrict__ dhout, const __bf16* __restrict__ gbuf, const float* __restrict__ cbuf,
    const float* __restrict__ W, const float* __restrict__ U, float* __restrict__ dx, __bf16* __restrict__ dz,
    int Mp, int T, int Din, int Dw, const float* __restrict__ x = nullptr, const float* __restrict__ h = nullptr,
    const float* __restrict__ bias = nullptr, const unsigned char* __restrict__ pidx = nullptr, int P = 1) {
  lstm_tm_bwd_body<H, KX, GR, D, DZ, DX, LAST, false, RG, UP, XB, HB>(dhout, gbuf, cbuf, W, U, dx, dz, Mp, T, Din,
                                                                      Dw, blockIdx.x, gridDim.x, x, h, nullptr, bias,
                                                                      pidx, P);
}

template <int H, int KX, int D, bool DX, bool LAST, bool RG = false, bool UP = false, bool XB = false, bool HB = false>
__global__ __launch_bounds__(TMC<H>::NT) void lstm_tm_bwd_wg_kernel(
    const float* __restrict__ dhout, const __bf16* __restrict__ gbuf, const float* __restrict__ cbuf,
    const float* __restrict__ W, const float* __restrict__ U, float* __restrict__ dx, const float* __restrict__ x,
    const float* __restrict__ h, float* __restrict__ ws, int Mp, int T, int Din, int Dw,
    const float* __restrict__ bias = nullptr, const unsigned char* __restrict__ pidx = nullptr, int P = 1) {
  lstm_tm_bwd_body<H, KX, 4, D, false, DX, LAST, true, RG, UP, XB, HB>(dhout, gbuf, cbuf, W, U, dx, nullptr, Mp, T,
                                                                       Din, Dw, blockIdx.x, gridDim.x, x, h, ws, bias,
                                                                       pidx, P);
}

// =====================================================================================
// host side
// ring depth (reverse steps) of a saved-gates recurrence's streams. H = 64: 16 waves x 128 VGPRs, shorter rings
constexpr int tm_bwd_depth(int H) { return H >= 64 ? 2 : 4; }
constexpr int TM_RG_D = 4;       // the frozen recompute-gates recurrence

// dh: [T, Mp, H] (or [Mp, H] when only the last step has a gradient). Returns dx [T, Mp, Din]
// (empty if !need_dx) and accumulates dW, dU, db when they are non-empty. An empty g (the forward ran
// with store_gates = false) selects the recompute-gates backward, which needs the bias b.
// pidx / pool (optional): the layer's output went through MaxPooling1D(pool) and dh is the POOLED
// gradient [T / pool, Mp, H] with the pool's byte argmax pidx (un-pooled on load, lstm_tm_bwd_body UP).
at::Tensor lstm_tm_bwd(const at::Tensor& dh, const at::Tensor& g, const at::Tensor& c, const at::Tensor& x,
                       const at::Tensor& h, const at::Tensor& W, const at::Tensor& U, const at::Tensor& b,
                       at::Tensor dW, at::Tensor dU, at::Tensor db, bool need_dx,
                       const c10::optional<at::Tensor>& pidx_opt, int64_t pool) {
  const at::Tensor* ops[] = {&dh, &W, &U, &b};
  for (const at::Tensor* t : ops) check_f32_cuda(*t, "lstm_tm_bwd operand");
  const bool rg = g.numel() == 0;
  // x / h in bf16: a recompute-gates pair's layer-A output (TM_RG_BF16H) as layer B's x or layer A's h
  const bool xb = x.scalar_type() == at::kBFloat16, hb = h.scalar_type() == at::kBFloat16;
  if (!xb) check_f32_cuda(x, "lstm_tm_bwd x");
  if (!hb) check_f32_cuda(h, "lstm_tm_bwd h");
  TORCH_CHECK(((!xb && !hb) || rg) && !(xb && hb) && x.is_cuda() && h.is_cuda(),
              "lstm_tm_bwd: bf16 x or h only from a recompute-gates pair forward");
  const float* xptr = reinterpret_cast<const float*>(x.data_ptr());
  const auto fopt = x.options().dtype(at::kFloat);   // (fp32 outputs / workspaces whatever x's dtype)
  const float* hptr = reinterpret_cast<const float*>(h.data_ptr());
  if (!rg) check_gates_cuda(g);
  // (recompute gates: c_t saved in bf16 by the forward, TM_RG_BF16C)
  TORCH_CHECK(c.is_cuda() && c.is_contiguous() &&
                  c.scalar_type() == ((rg && TM_RG_BF16C) ? at::kBFloat16 : at::kFloat),
              "lstm_tm_bwd: c must be the forward's saved state (", (rg && TM_RG_BF16C) ? "bf16" : "fp32", ")");
  const float* cptr = reinterpret_cast<const float*>(c.data_ptr());
  const int T = (int)x.size(0), Mp = (int)x.size(1), Din = (int)x.size(2), H = (int)U.size(0);
  const int Dw = (int)W.size(0);
  TORCH_CHECK(Dw >= 1 && Dw <= Din && W.size(1) == 4 * H && b.numel() == 4 * H, "lstm_tm_bwd: W / b shape");
  const bool last = dh.dim() == 2;
  const bool up = pidx_opt.has_value() && pidx_opt->defined() && pidx_opt->numel() > 0;
  const unsigned char* pidx = nullptr;
  const int P = up ? (int)pool : 1;
  if (up) {
    TORCH_CHECK(!last && P >= 1 && P <= 255 && T / P >= 1, "lstm_tm_bwd: pool size 1..255 <= T, per-step gradient");
    TORCH_CHECK(pidx_opt->is_cuda() && pidx_opt->scalar_type() == at::kByte && pidx_opt->is_contiguous() &&
                    pidx_opt->sizes() == dh.sizes(), "lstm_tm_bwd: pidx must be a contiguous uint8 tensor shaped like dh");
    pidx = pidx_opt->data_ptr<uint8_t>();
  }
  TORCH_CHECK(last ? (dh.size(0) == Mp && dh.size(1) == H)
                   : (dh.size(0) == (up ? T / P : T) && dh.size(1) == Mp && dh.size(2) == H), "lstm_tm_bwd: dh shape");
  TORCH_CHECK(dh.is_contiguous(), "lstm_tm_bwd: dh must be contiguous");
  TORCH_CHECK((rg || g.numel() == (long)(T + 1) * Mp * H * 4) && c.numel() == (long)(T + 1) * Mp * H &&
                  h.numel() == (long)T * Mp * H, "lstm_tm_bwd: saved state shapes");
  const bool wg = dW.numel() > 0;
  if (wg) {
    const at::Tensor* gs[] = {&dW, &dU, &db};
    for (const at::Tensor* t : gs) check_f32_cuda(*t, "lstm_tm_bwd grad");
    TORCH_CHECK(dW.numel() == (long)Dw * 4 * H && dU.numel() == (long)H * 4 * H && db.numel() == 4 * H,
                "lstm_tm_bwd: gradient buffer shapes");
  }
  const int gr = tm_granule(Din, x.data_ptr());
  TORCH_CHECK(tm_supported(H, Din, gr), "lstm_tm_bwd: unsupported shape");
  TORCH_CHECK(!rg || (tm_rg_ok(H, gr) && Din <= 64 && h.is_contiguous() && x.is_contiguous()),
              "lstm_tm_bwd: recomputed gates need H <= 32, Din <= 64, contiguous 16-byte aligned x / h");
  c10::DeviceGuard guard(x.device());
  const int ntiles = Mp / 16;
  auto st = stream();
  const int ncb_w = lstm_grads_col_blocks(H);
  const __bf16* gptr = rg ? nullptr : bf16_ptr(g);
  const float* dhp = dh.data_ptr<float>();
  const float* Wp = W.data_ptr<float>();
  const float* Up = U.data_ptr<float>();
  const float* bp = b.data_ptr<float>();
  const long rows = (long)T * Mp;
  constexpr const char* kUnpool = "lstm_tm_bwd: un-pooling takes a per-step gradient and 16-byte granules";
  constexpr const char* kBf16 = "lstm_tm_bwd: bf16 x or h only from a recompute-gates pair forward";
  const int xh = xb ? 1 : (hb ? 2 : 0);            // which of x / h is bf16 (recomputed gates only)

  // a saved-gates recurrence writing dz and / or dx (un-pooling on load: per-step gradient, 16-byte granules)
  auto saved_gates_rec = [&](auto hc, auto kxc, auto grc, auto dzc, auto dxc, const float* dhv, float* dxp, __bf16* dzp,
                             const unsigned char* pi) {
    constexpr int HH = decltype(hc)::value, KX = decltype(kxc)::value, GR = decltype(grc)::value;
    constexpr bool DZ = decltype(dzc)::value, DX = decltype(dxc)::value;
    dispatch_bools([&](auto lastc, auto upc) {
      constexpr bool LAST = decltype(lastc)::value, UP = decltype(upc)::value;
      if constexpr (UP && (LAST || GR != 4)) {
        TORCH_CHECK(false, kUnpool);
      } else
        hipLaunchKernelGGL((lstm_tm_bwd_kernel<HH, KX, GR, tm_bwd_depth(HH), DZ, DX, LAST, false, UP>), dim3(ntiles),
                           dim3(TMC<HH>::NT), 0, st, dhv, gptr, cptr, Wp, Up, dxp, dzp, Mp, T, Din, Dw, nullptr, nullptr,
                           nullptr, pi, UP ? P : 1);
    }, last, pi != nullptr);
    GQ_LAUNCH_CHECK();
  };

  if (wg && (rg || tm_fused_wgrad(H, Din, gr, ntiles))) {
    // weight gradients inside the recurrence: one split record per tile, then the reduction
    at::Tensor ws = at::empty({GradsGeom(H, Dw).ws_floats(ntiles)}, fopt);
    at::Tensor dx = need_dx ? at::empty({T + 1, Mp, Din}, fopt) : at::empty({0}, fopt);
    if (need_dx) TORCH_CHECK(tm_granule(Din, dx.data_ptr()) >= gr, "lstm_tm_bwd: dx alignment");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(h.data_ptr()) % 4 == 0 && h.is_contiguous(), "lstm_tm_bwd: h layout");
    float* dxp = need_dx ? dx.data_ptr<float>() : nullptr;
    dispatch_int<16, 32>(H, "lstm_tm_bwd: fused weight gradients need H = 16 or 32", [&](auto hc) {
      dispatch_int<1, 2>(tm_kx(Din), "lstm_tm_bwd: fused weight gradients need Din <= 64", [&](auto kxc) {
        dispatch_int<0, 1, 2>(xh, kBf16, [&](auto xhc) {
          dispatch_bools([&](auto dxc, auto lastc, auto rgc, auto upc) {
            constexpr int HH = decltype(hc)::value, KX = decltype(kxc)::value, XH = decltype(xhc)::value;
            constexpr bool DX = decltype(dxc)::value, LAST = decltype(lastc)::value, RG = decltype(rgc)::value,
                           UP = decltype(upc)::value;
            if constexpr (UP && LAST) {
              TORCH_CHECK(false, kUnpool);
            } else if constexpr (!RG && XH != 0) {
              TORCH_CHECK(false, kBf16);
            } else
              hipLaunchKernelGGL(
                  (lstm_tm_bwd_wg_kernel<HH, KX, HH == 16 ? TMW_D16 : TMW_D32, DX, LAST, RG, UP, XH == 1, XH == 2>),
                  dim3(ntiles), dim3(TMC<HH>::NT), 0, st, dhp, gptr, cptr, Wp, Up, dxp, xptr, hptr, ws.data_ptr<float>(),
                  Mp, T, Din, Dw, bp, pidx, P);
          }, need_dx, last, rg, up);
        });
      });
    });
    GQ_LAUNCH_CHECK();
    lstm_grads_reduce_records(ws, H, Dw, ntiles, dW.data_ptr<float>(), dU.data_ptr<float>(), db.data_ptr<float>(), st);
    return need_dx ? dx.narrow(0, 0, T) : dx;
  }
  TORCH_CHECK(!rg || !wg, "lstm_tm_bwd: recomputed gates with weight gradients take the fused kernel");
  if (wg && need_dx && ncb_w > 1 && tm_rec_dx()) {
    // several gate-column blocks: the weight-gradient pass could only produce dx as ncb partial
    // slabs plus a slab sum (ncb + 2 dx-sized passes); the recurrence computes dx^T = W dz^T
    // itself instead (its MFMA phase has the whole 4H dz tile in LDS) and writes dx once.
    at::Tensor dz = at::empty({T + 1, Mp, 4 * H}, fopt.dtype(at::kBFloat16));
    at::Tensor dx = at::empty({T + 1, Mp, Din}, fopt);
    TORCH_CHECK(tm_granule(Din, dx.data_ptr()) >= gr, "lstm_tm_bwd: dx alignment");
    tm_dispatch<16, 32, 64>(H, Din, gr, "lstm_tm: hidden size must be 16, 32 or 64", [&](auto hc, auto kxc, auto grc) {
      if constexpr (lstm_grads_col_blocks(decltype(hc)::value) > 1)
        saved_gates_rec(hc, kxc, grc, std::true_type{}, std::true_type{}, dhp, dx.data_ptr<float>(), bf16_ptr(dz), pidx);
      else
        TORCH_CHECK(false, "lstm_tm_bwd: one gate-column block takes dx from the rows pass");
    });
    lstm_grads_rows(dz.data_ptr(), 1, x.data_ptr<float>(), h.data_ptr<float>(), Wp, nullptr, dW.data_ptr<float>(),
                    dU.data_ptr<float>(), db.data_ptr<float>(), rows, rows, Mp, H, Dw, Din, rows * Din, Din, rows * Din,
                    st);
    return dx.narrow(0, 0, T);
  }
  if (wg) {
    // recurrence -> dz (bf16), then dW/dU/db (+ dx) in one pass over T*Mp rows. (A pooled gradient
    // is un-pooled to full resolution first: this path's recurrence is instantiated without UP.)
    const at::Tensor dhf = up ? maxpool1d_bwd(dh.view({1, T / P, (long)Mp * H}), pidx_opt->view({1, T / P, (long)Mp * H}),
                                              T, P).view({T, Mp, H})
                              : dh;
    at::Tensor dz = at::empty({T + 1, Mp, 4 * H}, fopt.dtype(at::kBFloat16));
    dispatch_int<16, 32, 64>(H, "lstm_tm: hidden size must be 16, 32 or 64", [&](auto hc) {
      using One = std::integral_constant<int, 1>;          // (no dx: the x channel blocks and granule are unused)
      saved_gates_rec(hc, One{}, One{}, std::true_type{}, std::false_type{}, dhf.data_ptr<float>(), nullptr, bf16_ptr(dz),
                      nullptr);
    });
    // dx keeps the x layout (Din channels); padding channels (>= Dw) get zero gradient
    at::Tensor dx = need_dx ? at::empty({ncb_w, T, Mp, Din}, fopt) : at::empty({0}, fopt);
    lstm_grads_rows(dz.data_ptr(), 1, x.data_ptr<float>(), h.data_ptr<float>(), Wp, need_dx ? dx.data_ptr<float>() : nullptr,
                    dW.data_ptr<float>(), dU.data_ptr<float>(), db.data_ptr<float>(), rows, rows, Mp, H, Dw, Din,
                    rows * Din, Din, rows * Din, st);
    if (!need_dx) return dx;
    return ncb_w == 1 ? dx[0] : dx.sum(0);
  }
  at::Tensor dx = at::empty({T + 1, Mp, Din}, fopt);
  TORCH_CHECK(tm_granule(Din, dx.data_ptr()) >= gr, "lstm_tm_bwd: dx alignment");
  if (rg) {      // frozen weights (integrated gradients), gates recomputed: H <= 32, GR = 4
    dispatch_int<16, 32>(H, "lstm_tm2: hidden size must be 16 or 32", [&](auto hc) {
      dispatch_int<1, 2>(tm_kx(Din), "lstm_tm_bwd: recomputed gates need Din <= 64", [&](auto kxc) {
        dispatch_int<0, 1, 2>(xh, kBf16, [&](auto xhc) {
          dispatch_bools([&](auto lastc, auto upc) {
            constexpr int HH = decltype(hc)::value, KX = decltype(kxc)::value, XH = decltype(xhc)::value;
            constexpr bool LAST = decltype(lastc)::value, UP = decltype(upc)::value;
            if constexpr (UP && LAST) {
              TORCH_CHECK(false, kUnpool);
            } else
              hipLaunchKernelGGL(
                  (lstm_tm_bwd_kernel<HH, KX, 4, TM_RG_D, false, true, LAST, true, UP, XH == 1, XH == 2>), dim3(ntiles),
                  dim3(TMC<HH>::NT), 0, st, dhp, nullptr, cptr, Wp, Up, dx.data_ptr<float>(), nullptr, Mp, T, Din, Dw,
                  xptr, hptr, bp, pidx, P);
          }, last, up);
        });
      });
    });
    GQ_LAUNCH_CHECK();
    return dx.narrow(0, 0, T);
  }
  tm_dispatch<16, 32, 64>(H, Din, gr, "lstm_tm: hidden size must be 16, 32 or 64", [&](auto hc, auto kxc, auto grc) {
    saved_gates_rec(hc, kxc, grc, std::false_type{}, std::true_type{}, dhp, dx.data_ptr<float>(), nullptr, pidx);
  });
  return dx.narrow(0, 0, T);
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("lstm_tm_bwd", &gq::lstm_tm_bwd);
}
