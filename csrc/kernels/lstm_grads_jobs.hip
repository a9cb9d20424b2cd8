// Weight-gradient passes of LSTM layers as JOBS (lstm_grads_body.h GradJob / RedJob): a layer's pass over its
// dz / x / h rows and the reduction of its split records do not feed any later recurrence, so they are
// batched into launches that have idle CUs instead of running one by one behind their layer:
//   lstm_tm_bwd_pipe      a backward recurrence (lstm_tm_bwd_body.h) whose extra workgroups run the job of the layer
//                         finished before it and the reduction of the one before that (lstm_tm_bwd_dual_kernel);
//                         without a recurrence it flushes a pending job / reduction
//   lstm_grads_multi      up to MULTI_MAX jobs in one launch (and, optionally, the fused GCN backward as extra
//                         workgroups), then up to MULTI_MAX reductions in one more
//   lstm_reduce_flush     every reduction lstm_grads_rows queued under lstm_defer_reduce, MULTI_MAX per launch
//   lstm_grads_job_ws     the workspace of a job; lstm_tm_grads: one time-major layer's pass on its own
// The record geometry and the job records are filled by GradsGeom / make_grad_job / make_red_job.
#include "common.h"

#include <cstdlib>
#include "gcn_fused.h"
#include "lstm_grads_body.h"
#include "lstm_tm_bwd_body.h"
#include "lstm_tm_common.h"

namespace gq {

// =====================================================================================
// Horizontal fusion of the backward: one launch = the reverse recurrence of layer L (the
// serial critical path, workgroups [0, ntiles)) + the weight-gradient pass of the layer
// processed just before it (extra 256-thread workgroups) + the split reduction of the layer
// before that. The weight-gradient work used to run after each recurrence on the same
// stream; here it fills the idle CUs while the next recurrence runs (separate streams were
// measured slower: cross-stream event waits). Extra waves of a recurrence-sized workgroup
// exit at once (s_barrier only counts live waves).
template <int HR, int HG, int DT>
__global__ __launch_bounds__(TMC<HR>::NT) void lstm_tm_bwd_dual_kernel(
    const float* __restrict__ dh, const __bf16* __restrict__ g, const float* __restrict__ c,
    const float* __restrict__ W, const float* __restrict__ U, __bf16* __restrict__ dz, int Mp, int T, int Dw,
    int ntiles, GradJob gj, RedJob rj) {
  constexpr int D = HR >= 64 ? 2 : 4;
  const int b = blockIdx.x;
  if (b < ntiles) {
    lstm_tm_bwd_body<HR, 1, 1, D, true, false, false>(dh, g, c, W, U, nullptr, dz, Mp, T, Dw, Dw, b, ntiles);
    return;
  }
  if (threadIdx.x >= 256) return;
  const int gb = b - ntiles;
  if (gb < gj.nblocks) {
    if constexpr (HG > 0)
      {
      __shared__ __attribute__((aligned(16))) char gsm[GradsLds<HG, DT>::BYTES];
      lstm_grads_body<HG, DT, 4>(gj.dz, gj.x, gj.h, gj.W, nullptr, gj.ws, gj.rows, gj.period, gj.hshift, gj.Din,
                                 gj.ldx, 0, gj.Din, gj.xg, gj.x_elems, gb % gj.ncb, gb / gj.ncb, gj.ncb, gj.splits, gsm);
    }
    return;
  }
  const int rb = gb - gj.nblocks;
  if (rb < rj.nblocks) {
    if (rj.kb > 1)     // many slots: KB slot blocks per workgroup
      lstm_grads_reduce_multi<PIPE_RED_KB>(rj.ws, rj.splits, rj.RC, rj.ncb, rj.DT, rj.HT, rj.Din, rj.H, rj.dW, rj.db,
                                           rj.dU, rb, rj.nf);
    else               // few slots, many splits: one slot block per workgroup, 4 add chains per lane
      lstm_grads_reduce_body(rj.ws, rj.splits, rj.RC, nullptr, rj.ncb, rj.DT, rj.HT, rj.Din, rj.H, rj.dW, rj.db,
                             rj.dU, rb, 0, 1, rj.nf);
  }
}

// ---- all pending weight-gradient jobs in ONE launch, then all reductions in ONE launch
// (after the chain backward, whose recurrences leave no per-layer launch to hide them in)
static constexpr int MULTI_MAX = 12;
struct MultiGrad {
  GradJob j[MULTI_MAX];
  int start[MULTI_MAX + 1];
  int key[MULTI_MAX];              // HG * 8 + DT
  int n;
  int gcn_nb;                      // > 0: blocks [0, gcn_nb) run the fused GCN backward (gcn_fused.h)
  GcnBwdJob gcn;
  int gcn_coef;                    // 1: those blocks run the coefficient form (gcn_coef_bwd_body) instead
  GcnCoefJob gcnc;
};
struct MultiRed {
  RedJob j[MULTI_MAX];
  int start[MULTI_MAX + 1];
  int n;
  int* nf;                         // non-finite gradient flag (chain control word 7)
};

// HMAX: the largest hidden size among the launch's jobs. The kernel is allocated for its largest instance
// (HMAX = 128: 155 VGPRs + 52 AGPRs, 27 KB of LDS, two workgroups per CU), so the tail launch behind a chain
// backward that built the upper layers' records itself (chain_wgrad.h) - H = 16 jobs and the GCN backward
// only - takes the instance that holds nothing else and is resident in one round.
template <int HMAX>
__global__ __launch_bounds__(256) void lstm_grads_multi_kernel(MultiGrad M) {
  constexpr int LDSB = GradsLds<HMAX, 5>::BYTES > GcnBwdLds<2, 16>::BYTES ? GradsLds<HMAX, 5>::BYTES
                                                                          : GcnBwdLds<2, 16>::BYTES;
  __shared__ __attribute__((aligned(16))) char smem[LDSB];   // the largest instance
  if ((int)blockIdx.x < M.gcn_nb) {                      // the GCN backward's workgroups
    const int gb = blockIdx.x;
    if (M.gcn_coef) gcn_coef_bwd_body<2, 16>(M.gcnc, gb);
    else if (M.gcn.key == 2 * 64 + 16)                     // (the CML configuration)
      gcn_fused_bwd_body<2, 16>(M.gcn, gb % M.gcn.B, gb / M.gcn.B, smem);
    return;
  }
  const int b = blockIdx.x - M.gcn_nb;
  int k = 0;
  while (k + 1 < M.n && b >= M.start[k + 1]) ++k;        // uniform
  const GradJob gj = M.j[k];                              // by value: scalar loads, no scratch copy
  const int gb = b - M.start[k];
#define GQ_MG(HG, DT)                                                                                    \
  case HG * 8 + DT:                                                                                      \
    if constexpr (HG <= HMAX)                                                                            \
      lstm_grads_body<HG, DT, 4>(gj.dz, gj.x, gj.h, gj.W, nullptr, gj.ws, gj.rows, gj.period, gj.hshift, gj.Din, \
                                 gj.ldx, 0, gj.Din, gj.xg, gj.x_elems, gb % gj.ncb, gb / gj.ncb, gj.ncb, gj.splits, \
                                 smem);                                                                  \
    break;
#define GQ_MG_H(HG) GQ_MG(HG, 1) GQ_MG(HG, 2) GQ_MG(HG, 3) GQ_MG(HG, 4) GQ_MG(HG, 5)
  switch (M.key[k]) {
    GQ_MG_H(16) GQ_MG_H(32) GQ_MG_H(64) GQ_MG_H(128)
    default: break;
  }
#undef GQ_MG_H
#undef GQ_MG
}

__global__ __launch_bounds__(256) void lstm_grads_reduce_multi_kernel(MultiRed M) {
  const int b = blockIdx.x;
  int k = 0;
  while (k + 1 < M.n && b >= M.start[k + 1]) ++k;
  const RedJob rj = M.j[k];
  if (rj.kb > 1)
    lstm_grads_reduce_multi<PIPE_RED_KB>(rj.ws, rj.splits, rj.RC, rj.ncb, rj.DT, rj.HT, rj.Din, rj.H, rj.dW, rj.db,
                                         rj.dU, b - M.start[k], M.nf);
  else
    lstm_grads_reduce_body(rj.ws, rj.splits, rj.RC, nullptr, rj.ncb, rj.DT, rj.HT, rj.Din, rj.H, rj.dW, rj.db,
                           rj.dU, b - M.start[k], 0, 1, M.nf);
}

// =====================================================================================
// host side
// workspace of a pending weight-gradient job: [splits][ncb][(DT + HT) fragments][1024] fp32
at::Tensor lstm_grads_job_ws(const at::Tensor& dz, const at::Tensor& x, const at::Tensor& W, int64_t H) {
  check_f32_cuda(W, "W");
  const GradsGeom geo((int)H, (int)W.size(0));
  const long rows = x.numel() / x.size(-1);
  const long ntiles = (rows + 31) / 32;
  // row tiles per split: each split writes a whole record (all column blocks) once, so few tiles
  // per split multiply the record traffic (written here, re-read by the reduction)
  static const int tps = [] {
    const char* e = std::getenv("GNNQC_GRADS_TPS");
    return e != nullptr ? std::max(1, std::atoi(e)) : 4;   // 4: best of 2 / 4 / 8 / 16 on the CML step
  }();
  const int splits = (int)std::max<long>(1, std::min<long>({(ntiles + tps - 1) / tps, (long)std::max(64, 2048 / geo.ncb),
                                                            (long)PIPE_MAX_SPLITS}));
  c10::DeviceGuard guard(x.device());
  return at::empty({(long)splits * geo.RC}, x.options());
}

// workspace of exactly `splits` records of the layer with input weights W [Din, 4H]: the backward chain's
// weight-gradient epilogues write one per 16-sequence tile (chain_wgrad.h)
at::Tensor lstm_grads_record_ws(const at::Tensor& W, int64_t splits) {
  check_f32_cuda(W, "W");
  TORCH_CHECK(W.dim() == 2 && W.size(1) % 64 == 0 && splits >= 1 && splits <= PIPE_MAX_SPLITS,
              "lstm_grads_record_ws: W [Din, 4H] and 1 .. ", PIPE_MAX_SPLITS, " records");
  const GradsGeom geo((int)W.size(1) / 4, (int)W.size(0));
  c10::DeviceGuard guard(W.device());
  return at::empty({splits * (long)geo.RC}, W.options());
}

static bool grads_job_ok(const at::Tensor& x, int Dw) {
  const int ldx = (int)x.stride(-2);
  return ldx % 4 == 0 && ldx >= Dw && ldx <= 144 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
         GradsGeom::din_tiles(Dw) <= 5 && x.stride(-1) == 1;
}

// rec: dh [T, Mp, H] (empty: no recurrence); job (gz empty: none): dz / x / h / W of the layer
// whose weight gradients to compute, with its row mapping (period, hshift) and workspace;
// reduce (rws empty: none): a job whose gradient pass already ran. Returns the rec's dz.
at::Tensor lstm_tm_bwd_pipe(const at::Tensor& dh, const at::Tensor& g, const at::Tensor& c, const at::Tensor& W,
                            const at::Tensor& U, int64_t T, const at::Tensor& gz, const at::Tensor& gx,
                            const at::Tensor& gh, const at::Tensor& gW, int64_t g_period, int64_t g_hshift,
                            const at::Tensor& gws, const at::Tensor& rws, const at::Tensor& rW, at::Tensor rdW,
                            at::Tensor rdU, at::Tensor rdb) {
  const bool rec = dh.numel() > 0, job = gz.numel() > 0, red = rws.numel() > 0;
  const at::Tensor& ref = rec ? dh : (job ? gz : rws);
  c10::DeviceGuard guard(ref.device());
  int HR = 16, Mp = 0, ntiles = 0, Dw = 1;
  at::Tensor dz = at::empty({0}, ref.options());
  if (rec) {
    for (const at::Tensor* t : {&dh, &c, &W, &U}) check_f32_cuda(*t, "lstm_tm_bwd_pipe operand");
    check_gates_cuda(g);
    HR = (int)U.size(0);
    Mp = (int)dh.size(1);
    TORCH_CHECK(dh.dim() == 3 && dh.size(0) == T && dh.size(2) == HR && Mp % 16 == 0, "lstm_tm_bwd_pipe: dh shape");
    TORCH_CHECK(g.numel() == (long)(T + 1) * Mp * HR * 4 && c.numel() == (long)(T + 1) * Mp * HR,
                "lstm_tm_bwd_pipe: saved state shapes");
    TORCH_CHECK(HR == 16 || HR == 32 || HR == 64, "lstm_tm_bwd_pipe: hidden size");
    ntiles = Mp / 16;
    Dw = (int)W.size(0);
    dz = at::empty({T + 1, Mp, 4 * HR}, dh.options().dtype(at::kBFloat16));
  }
  GradJob gj{};
  at::Tensor gz_b;
  int HG = 0, DTG = 1;
  if (job) {
    check_dz_cuda(gz);
    for (const at::Tensor* t : {&gh, &gW, &gws}) check_f32_cuda(*t, "lstm_tm_bwd_pipe job operand");
    gz_b = job_dz(gz);
    TORCH_CHECK(gx.is_cuda() && gx.scalar_type() == at::kFloat, "lstm_tm_bwd_pipe: job x");
    HG = (int)gW.size(1) / 4;
    TORCH_CHECK(grads_job_ok(gx, (int)gW.size(0)), "lstm_tm_bwd_pipe: job x layout");
    DTG = GradsGeom::din_tiles((int)gW.size(0));
    gj = make_grad_job(gz_b, gx, gh, gW, g_period, g_hshift, gws, "lstm_tm_bwd_pipe: job workspace size");
  }
  RedJob rj{};
  if (red) {
    for (const at::Tensor* t : {&rws, &rW}) check_f32_cuda(*t, "lstm_tm_bwd_pipe reduce operand");
    for (at::Tensor* t : {&rdW, &rdU, &rdb}) check_f32_cuda(*t, "lstm_tm_bwd_pipe reduce gradient");
    const int H = (int)rW.size(1) / 4, Din = (int)rW.size(0);
    const int splits = GradsGeom(H, Din).job_splits(rws, "lstm_tm_bwd_pipe: reduce workspace size");
    TORCH_CHECK(rdW.numel() == rW.numel() && rdU.numel() == (long)H * 4 * H && rdb.numel() == 4 * H,
                "lstm_tm_bwd_pipe: reduce gradient buffers");
    rj = make_red_job(rws.data_ptr<float>(), H, Din, splits, rdW.data_ptr<float>(), rdU.data_ptr<float>(),
                      rdb.data_ptr<float>(), chain_ctl(rws.get_device()) + 7);
  }
  const int nblk = ntiles + gj.nblocks + rj.nblocks;
  if (nblk == 0) return dz;
  TORCH_CHECK(!job || HG == HR || HG == 2 * HR || !rec, "lstm_tm_bwd_pipe: job hidden size must be H or 2H of the rec");
  const __bf16* gp = rec ? bf16_ptr(g) : nullptr;
  const float* dhp = rec ? dh.data_ptr<float>() : nullptr;
  const float* cp = rec ? c.data_ptr<float>() : nullptr;
  const float* Wp = rec ? W.data_ptr<float>() : nullptr;
  const float* Up = rec ? U.data_ptr<float>() : nullptr;
  __bf16* dzp = rec ? bf16_ptr(dz) : nullptr;
  auto st = stream();
  // a flush launch (no recurrence) runs 256-thread job workgroups under the smallest recurrence width that
  // carries the job's hidden size: HG = 16, 32 -> 16, 64 -> 32, 128 -> 64
  const int HL = rec ? HR : (HG <= 32 ? 16 : HG / 2);
  dispatch_int<16, 32, 64>(HL, "lstm_tm_bwd_pipe: job hidden size", [&](auto hrc) {
    dispatch_int<0, 1, 2>(job ? HG / HL : 0, "lstm_tm_bwd_pipe: job hidden size", [&](auto kc) {
      dispatch_int<1, 2, 3, 4, 5>(DTG, "lstm_tm_bwd_pipe: job x layout", [&](auto dtc) {
        constexpr int HRV = decltype(hrc)::value, HGV = decltype(kc)::value * HRV, DTV = decltype(dtc)::value;
        if constexpr (HGV == 0 && DTV != 1) {
          TORCH_CHECK(false, "lstm_tm_bwd_pipe: no job, no din tiles");
        } else
          hipLaunchKernelGGL((lstm_tm_bwd_dual_kernel<HRV, HGV, DTV>), dim3(nblk), dim3(TMC<HRV>::NT), 0, st, dhp, gp,
                             cp, Wp, Up, dzp, Mp, (int)T, Dw, ntiles, gj, rj);
      });
    });
  });
  GQ_LAUNCH_CHECK();
  return dz;
}

// grads of jobs (dz, x, h, W, period, hshift, ws) then reductions of rjobs (ws, W, dW, dU, db):
// a reduce job may be one of this call's grads jobs (stream order runs the grads first).
// gcn_t / gcn_i (optional): the arguments of gcn_fused_bwd - [dh, series, shift, scale, win_group,
// win_center, win_valid, group_anom_pos, pw, wids, table, cursor (empty: none), S, st, W, bias,
// alpha, dW, dgamma, dbeta, dalpha] / [c_off, tb, seq_len, time_norm] - run as extra workgroups of
// the gradient launch (both only need the chain backward's results; the CML configuration,
// Cin = 2, F = 16, only: every instantiation would raise the launch's register allocation).
void lstm_grads_multi(at::TensorList gz, at::TensorList gx, at::TensorList gh, at::TensorList gW,
                      at::IntArrayRef period, at::IntArrayRef hshift, at::TensorList gws, at::TensorList rws,
                      at::TensorList rW, at::TensorList rdW, at::TensorList rdU, at::TensorList rdb,
                      at::TensorList gcn_t, at::IntArrayRef gcn_i) {
  const int ng = (int)gz.size(), nr = (int)rws.size();
  TORCH_CHECK(ng <= MULTI_MAX && nr <= MULTI_MAX && (int)gx.size() == ng && (int)gh.size() == ng &&
                  (int)gW.size() == ng && (int)period.size() == ng && (int)hshift.size() == ng &&
                  (int)gws.size() == ng && (int)rW.size() == nr && (int)rdW.size() == nr && (int)rdU.size() == nr &&
                  (int)rdb.size() == nr, "lstm_grads_multi: job lists");
  TORCH_CHECK((gcn_t.size() == 0 && gcn_i.size() == 0) || (gcn_t.size() == 21 && gcn_i.size() == 4) ||
                  (gcn_t.size() == 10 && gcn_i.size() == 1), "lstm_grads_multi: gcn job lists");
  TORCH_CHECK(gcn_t.size() == 0 || ng > 0, "lstm_grads_multi: a GCN job rides on a gradient launch");
  if (ng + nr == 0) return;
  c10::DeviceGuard guard(ng ? gz[0].device() : rws[0].device());
  auto st = stream();
  if (ng) {
    MultiGrad M{};
    M.n = ng;
    if (gcn_t.size() == 10) {        // coefficient form: [dh, coef, S, st, W, b, dW, dgamma, dbeta, dalpha] / [c_off]
      M.gcnc = gcn_coef_job(gcn_t[0], gcn_i[0], gcn_t[1], gcn_t[2], gcn_t[3], gcn_t[4], gcn_t[5], gcn_t[6], gcn_t[7],
                            gcn_t[8], gcn_t[9]);
      M.gcn_coef = 1;
      M.gcn_nb = M.gcnc.nblocks;
    } else if (gcn_t.size() > 0) {
      const c10::optional<at::Tensor> cur = gcn_t[11].numel() > 0 ? c10::optional<at::Tensor>(gcn_t[11]) : c10::nullopt;
      M.gcn = gcn_bwd_job(gcn_t[0], gcn_i[0], gcn_t[1], gcn_t[2], gcn_t[3], gcn_t[4], gcn_t[5], gcn_t[6], gcn_t[7],
                          gcn_t[8], gcn_t[9], gcn_t[10], cur, gcn_i[1], gcn_i[2], gcn_i[3] != 0, gcn_t[12], gcn_t[13],
                          gcn_t[14], gcn_t[15], gcn_t[16], gcn_t[17], gcn_t[18], gcn_t[19], gcn_t[20], M.gcn_nb);
      TORCH_CHECK(M.gcn.key == 2 * 64 + 16, "lstm_grads_multi: the GCN job takes 2 input / 16 output channels");
    }
    int nb = 0, hmax = 16;
    std::vector<at::Tensor> zb(ng);      // rounded dz of fp32 jobs; stream-ordered, so the temporaries may go
    for (int k = 0; k < ng; ++k) {
      check_dz_cuda(gz[k]);
      zb[k] = job_dz(gz[k]);
      for (const at::Tensor* t : {&gh[k], &gW[k], &gws[k]}) check_f32_cuda(*t, "lstm_grads_multi operand");
      TORCH_CHECK(gx[k].is_cuda() && gx[k].scalar_type() == at::kFloat, "lstm_grads_multi: x");
      const int HG = (int)gW[k].size(1) / 4, Dw = (int)gW[k].size(0);
      TORCH_CHECK(HG == 16 || HG == 32 || HG == 64 || HG == 128, "lstm_grads_multi: hidden size");
      TORCH_CHECK(grads_job_ok(gx[k], Dw), "lstm_grads_multi: x layout");
      M.j[k] = make_grad_job(zb[k], gx[k], gh[k], gW[k], period[k], hshift[k], gws[k], "lstm_grads_multi: workspace size");
      M.key[k] = HG * 8 + GradsGeom::din_tiles(Dw);
      M.start[k] = nb;
      nb += M.j[k].nblocks;
      hmax = std::max(hmax, HG);
    }
    M.start[ng] = nb;
    if (hmax == 16) hipLaunchKernelGGL(lstm_grads_multi_kernel<16>, dim3(M.gcn_nb + nb), dim3(256), 0, st, M);
    else hipLaunchKernelGGL(lstm_grads_multi_kernel<128>, dim3(M.gcn_nb + nb), dim3(256), 0, st, M);
    GQ_LAUNCH_CHECK();
  }
  if (nr) {
    MultiRed R{};
    R.n = nr;
    R.nf = chain_ctl(rws[0].get_device()) + 7;
    int nb = 0;
    for (int k = 0; k < nr; ++k) {
      const int H = (int)rW[k].size(1) / 4, Din = (int)rW[k].size(0);
      const int splits = GradsGeom(H, Din).job_splits(rws[k], "lstm_grads_multi: reduce workspace size");
      TORCH_CHECK(rdW[k].numel() == rW[k].numel() && rdU[k].numel() == (long)H * 4 * H && rdb[k].numel() == 4 * H,
                  "lstm_grads_multi: gradient buffers");
      R.j[k] = make_red_job(rws[k].data_ptr<float>(), H, Din, splits, rdW[k].data_ptr<float>(), rdU[k].data_ptr<float>(),
                            rdb[k].data_ptr<float>(), nullptr);      // (the launch's flag: R.nf)
      R.start[k] = nb;
      nb += R.j[k].nblocks;
    }
    R.start[nr] = nb;
    hipLaunchKernelGGL(lstm_grads_reduce_multi_kernel, dim3(nb), dim3(256), 0, st, R);
    GQ_LAUNCH_CHECK();
  }
}

// Switch for the deferred split reductions (common.h defer_reduce_mode); returns the previous value.
bool lstm_defer_reduce(bool flag) {
  const bool old = defer_reduce_mode();
  defer_reduce_mode() = flag;
  return old;
}

// Every queued split reduction (lstm_grads_rows under defer_reduce_mode) in one launch per
// MULTI_MAX jobs: each job's slot blocks are workgroups of lstm_grads_reduce_multi_kernel, so the
// layers' reductions (7 launches of 9-36 us on the SoilNet step, all of them a tail of idle CUs)
// run side by side. Same fixed summation order per slot as the per-layer reduce: deterministic.
// Returns the number of reductions run.
int64_t lstm_reduce_flush() {
  auto& q = deferred_reds();
  const int n = (int)q.size();
  for (int k0 = 0; k0 < n; k0 += MULTI_MAX) {
    const int kn = std::min(MULTI_MAX, n - k0);
    MultiRed R{};
    R.n = kn;
    R.nf = chain_ctl(c10::hip::current_device()) + 7;
    int nb = 0;
    for (int k = 0; k < kn; ++k) {
      const DeferredRed& d = q[k0 + k];
      TORCH_CHECK(d.ws.numel() >= (long)d.splits * GradsGeom(d.H, d.Din).RC, "lstm_reduce_flush: workspace size");
      R.j[k] = make_red_job(d.ws.data_ptr<float>(), d.H, d.Din, d.splits, d.dW, d.dU, d.db, nullptr);
      R.start[k] = nb;
      nb += R.j[k].nblocks;
    }
    R.start[kn] = nb;
    c10::DeviceGuard guard(q[k0].ws.device());
    hipLaunchKernelGGL(lstm_grads_reduce_multi_kernel, dim3(nb), dim3(256), 0, stream(), R);
    GQ_LAUNCH_CHECK();
  }
  q.clear();       // workspaces return to the caching allocator in stream order
  return n;
}

// Weight gradients (+ dx) of one time-major layer from its dz (lstm_grads_rows): accumulates
// dW, dU, db; returns dx [T, Mp, Din] if need_dx.
at::Tensor lstm_tm_grads(const at::Tensor& dz, const at::Tensor& x, const at::Tensor& h, const at::Tensor& W,
                         at::Tensor dW, at::Tensor dU, at::Tensor db, bool need_dx) {
  check_dz_cuda(dz);
  for (const at::Tensor* t : {&x, &h, &W}) check_f32_cuda(*t, "lstm_tm_grads operand");
  for (const at::Tensor* t : {&dW, &dU, &db}) check_f32_cuda(*t, "lstm_tm_grads gradient");
  const int T = (int)x.size(0), Mp = (int)x.size(1), Din = (int)x.size(2), H = (int)h.size(2);
  const int Dw = (int)W.size(0);
  TORCH_CHECK(dz.size(0) >= T && dz.size(1) == Mp && dz.size(2) == 4 * H && h.size(0) == T && h.size(1) == Mp,
              "lstm_tm_grads: shapes");
  TORCH_CHECK(Dw <= Din && dW.numel() == (long)Dw * 4 * H && dU.numel() == (long)H * 4 * H && db.numel() == 4 * H,
              "lstm_tm_grads: gradient buffer shapes");
  c10::DeviceGuard guard(x.device());
  const long rows = (long)T * Mp;
  const int ncb = lstm_grads_col_blocks(H);
  // padding channels (>= Dw) are written as zeros by the kernel (their W rows are masked)
  at::Tensor dx = need_dx ? at::empty({ncb, T, Mp, Din}, x.options()) : at::empty({0}, x.options());
  lstm_grads_rows(dz.data_ptr(), dz_bf16(dz), x.data_ptr<float>(), h.data_ptr<float>(), W.data_ptr<float>(),
                  need_dx ? dx.data_ptr<float>() : nullptr, dW.data_ptr<float>(), dU.data_ptr<float>(),
                  db.data_ptr<float>(), rows, rows, Mp, H, Dw, Din, rows * Din, Din, rows * Din, stream());
  if (!need_dx) return dx;
  return ncb == 1 ? dx[0] : dx.sum(0);
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("lstm_tm_grads", &gq::lstm_tm_grads);
  m.impl("lstm_tm_bwd_pipe", &gq::lstm_tm_bwd_pipe);
  m.impl("lstm_grads_job_ws", &gq::lstm_grads_job_ws);
  m.impl("lstm_grads_record_ws", &gq::lstm_grads_record_ws);
  m.impl("lstm_grads_multi", &gq::lstm_grads_multi);
}
