// Inference front end and output stage of a scoring step (gnnqc.infer.Predictor).
//
// series_tm_gather: the per-sensor baseline reads ONE node of every window, so its batch is cut
// straight from the resident series as the time-major, padded LSTM input
//   h[t, m, c] = (series[g, c0 - tb + t, n0, c] - shift[g, tc, n0, c]) * scale[g, tc, n0, c] * valid[w, n0]
// (w = ids[m], g = win_group[w], c0 = win_center[w], n0 = max(group_anom_pos[g], 0), tc = c0 or 0;
// batch_gather's arithmetic in batch_gather's order) with zero rows m >= B and zero channels
// c >= C. No [B,T,N,C] window, adjacency or node mask is ever written.
//
// predict_emit: writes one step's probabilities, labels, label mask and window ids into row
// cursor[0] of the pass's output tables and advances the device cursor, so a HIP graph of several
// scoring steps walks the id table and fills the output tables with no host work in between.
#include "common.h"

namespace gq {

// one thread per float4 of h: (t, m, q) with q the fastest index, then m: the [Mp, Cp] slab of a
// time step is written by consecutive lanes as consecutive 16-byte stores
__global__ __launch_bounds__(256) void series_tm_gather_kernel(
    const float* __restrict__ series, const float* __restrict__ shift, const float* __restrict__ scale,
    const long* __restrict__ wg, const long* __restrict__ wc, const uint8_t* __restrict__ wv,
    const float* __restrict__ wlab, const long* __restrict__ gap, const long* __restrict__ wids,
    const long* __restrict__ table, const long* __restrict__ cursor, long nrows, float4* __restrict__ h,
    float* __restrict__ y, float* __restrict__ ym, long* __restrict__ wid_out, int B, int Mp, int Q, int Tw, int Ttot,
    int Tn, int N, int C, int tb, int time_norm) {
  const long* ids = cursor != nullptr ? table + (cursor[0] % nrows) * B : wids;
  const long total = (long)Tw * Mp * Q;
  const int NC = N * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i % Q);
    const long tm = i / Q;
    const int m = (int)(tm % Mp);
    const int t = (int)(tm / Mp);
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m < B) {
      const long wraw = ids[m];
      const long w = wraw < 0 ? 0 : wraw;
      const float live = wraw >= 0 ? 1.f : 0.f;
      const long g = wg[w];
      const long a = gap[g];
      const int n0 = a < 0 ? 0 : (int)a;
      const float v = live * (wv[w * N + n0] ? 1.f : 0.f);
      const long c0 = wc[w];
      const long tn = time_norm ? c0 : 0;
      const float* src = series + (g * Ttot + (c0 - tb) + t) * (long)NC + n0 * C;
      const float* sh = shift + (g * Tn + tn) * (long)NC + n0 * C;
      const float* sc = scale + (g * Tn + tn) * (long)NC + n0 * C;
      float o[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = 4 * q + u;
        // (channels past C read channel C - 1, a valid address, and are dropped)
        const int cc = c < C ? c : C - 1;
        const float val = (src[cc] - sh[cc]) * sc[cc] * v;
        o[u] = c < C ? val : 0.f;
      }
      out = make_float4(o[0], o[1], o[2], o[3]);
      if (t == 0 && q == 0) {
        y[m] = wlab[w] * live;
        ym[m] = live;
        wid_out[m] = wraw;
      }
    }
    h[i] = out;
  }
}

// [h [T, Mp, Cp], y [B], y_mask [B], wid [B]]; ids from wids [B], or (cursor defined) from row
// cursor % table.size(0) of table [rows, B] (batch_gather's convention)
std::vector<at::Tensor> series_tm_gather(const at::Tensor& series, const at::Tensor& shift, const at::Tensor& scale,
                                         const at::Tensor& win_group, const at::Tensor& win_center,
                                         const at::Tensor& win_valid, const at::Tensor& win_label,
                                         const at::Tensor& group_anom_pos, const at::Tensor& wids,
                                         const at::Tensor& table, const c10::optional<at::Tensor>& cursor, int64_t tb,
                                         int64_t seq_len, bool time_norm) {
  check_f32_cuda(series, "series");
  check_f32_cuda(shift, "shift");
  check_f32_cuda(scale, "scale");
  check_f32_cuda(win_label, "win_label");
  TORCH_CHECK(series.dim() == 4, "series_tm_gather: series must be [G,Ttot,N,C]");
  TORCH_CHECK(win_group.scalar_type() == at::kLong && win_center.scalar_type() == at::kLong &&
                  group_anom_pos.scalar_type() == at::kLong && win_group.is_cuda() && win_center.is_cuda() &&
                  group_anom_pos.is_cuda() && win_group.is_contiguous() && win_center.is_contiguous() &&
                  group_anom_pos.is_contiguous(),
              "series_tm_gather: index tensors must be contiguous int64 device tensors");
  TORCH_CHECK(win_valid.scalar_type() == at::kByte && win_valid.is_contiguous() && win_valid.is_cuda(),
              "series_tm_gather: win_valid uint8");
  const int G = series.size(0), Ttot = series.size(1), N = series.size(2), C = series.size(3);
  TORCH_CHECK(shift.dim() == 4 && shift.size(0) == G && shift.size(2) == N && shift.size(3) == C &&
                  scale.sizes() == shift.sizes(),
              "series_tm_gather: shift / scale shape");
  const long W = win_center.size(0);
  TORCH_CHECK(win_valid.dim() == 2 && win_valid.size(0) == W && win_valid.size(1) == N && win_group.size(0) == W,
              "series_tm_gather: per-window tables");
  TORCH_CHECK(win_label.dim() == 1 && win_label.size(0) == W, "series_tm_gather: per-sensor labels [W] only");
  TORCH_CHECK(group_anom_pos.size(0) == G && C >= 1 && seq_len >= 1 && seq_len <= Ttot,
              "series_tm_gather: group / window dimensions");
  const long* wp = nullptr;
  const long* tp = nullptr;
  const long* cp = nullptr;
  long nrows = 1;
  int B;
  if (cursor.has_value() && cursor->defined()) {
    TORCH_CHECK(table.dim() == 2 && table.scalar_type() == at::kLong && table.is_contiguous() && table.is_cuda() &&
                    table.size(0) >= 1,
                "series_tm_gather: table must be a contiguous int64 [rows, B] device tensor");
    TORCH_CHECK(cursor->scalar_type() == at::kLong && cursor->numel() >= 1 && cursor->is_cuda(),
                "series_tm_gather: cursor must be int64[1] on the device");
    B = table.size(1);
    nrows = table.size(0);
    tp = table.data_ptr<long>();
    cp = cursor->data_ptr<long>();
  } else {
    TORCH_CHECK(wids.dim() == 1 && wids.scalar_type() == at::kLong && wids.is_contiguous() && wids.is_cuda(),
                "series_tm_gather: wids int64");
    B = wids.size(0);
    wp = wids.data_ptr<long>();
  }
  TORCH_CHECK(B >= 1, "series_tm_gather: empty batch");
  c10::DeviceGuard guard(series.device());
  auto fo = series.options();
  const int Mp = (B + 15) / 16 * 16, Cp = (C + 3) / 4 * 4, Q = Cp / 4;
  at::Tensor h = at::empty({seq_len, Mp, Cp}, fo);          // (allocations are 16-byte aligned)
  at::Tensor y = at::empty({B}, fo), ym = at::empty({B}, fo);
  at::Tensor wid = at::empty({B}, win_group.options());
  const long total = (long)seq_len * Mp * Q;
  const int grid = (int)std::max<long>(1, std::min<long>((total + 255) / 256, 4096));
  hipLaunchKernelGGL(series_tm_gather_kernel, dim3(grid), dim3(256), 0, stream(), series.data_ptr<float>(),
                     shift.data_ptr<float>(), scale.data_ptr<float>(), win_group.data_ptr<long>(),
                     win_center.data_ptr<long>(), win_valid.data_ptr<uint8_t>(), win_label.data_ptr<float>(),
                     group_anom_pos.data_ptr<long>(), wp, tp, cp, nrows, reinterpret_cast<float4*>(h.data_ptr<float>()),
                     y.data_ptr<float>(), ym.data_ptr<float>(), wid.data_ptr<long>(), B, Mp, Q, (int)seq_len, Ttot,
                     (int)shift.size(1), N, C, (int)tb, time_norm ? 1 : 0);
  GQ_LAUNCH_CHECK();
  return {h, y, ym, wid};
}

// ONE workgroup: every thread reads the cursor, the barrier closes the launch's reads of it, the
// rows are written (a cursor at or past rows_out writes nothing) and thread 0 advances the cursor
// as the last act of the launch (as the optimiser's update advances the training cursor).
__global__ __launch_bounds__(256) void predict_emit_kernel(
    const float* __restrict__ vals, const float* __restrict__ y, const float* __restrict__ mask,
    const long* __restrict__ wid, float* __restrict__ p_out, float* __restrict__ y_out, float* __restrict__ m_out,
    long* __restrict__ wid_out, long* cursor, long rows_out, int R, int B, int logits) {
  const int tid = threadIdx.x;
  const long cur = cursor[0];
  __syncthreads();
  if (cur >= 0 && cur < rows_out) {
    float* po = p_out + cur * R;
    float* yo = y_out + cur * R;
    float* mo = m_out + cur * R;
    for (int i = tid; i < R; i += 256) {
      const float z = vals[i];
      po[i] = logits ? 1.0f / (1.0f + expf(-z)) : z;
      yo[i] = y[i];
      mo[i] = mask[i];
    }
    long* wo = wid_out + cur * B;
    for (int i = tid; i < B; i += 256) wo[i] = wid[i];
  }
  if (tid == 0) cursor[0] = cur + 1;
}

void predict_emit(const at::Tensor& vals, bool logits, const at::Tensor& y, const at::Tensor& mask,
                  const at::Tensor& wid, at::Tensor p_out, at::Tensor y_out, at::Tensor mask_out, at::Tensor wid_out,
                  at::Tensor cursor) {
  check_f32_cuda(vals, "vals");
  check_f32_cuda(y, "y");
  check_f32_cuda(mask, "mask");
  check_f32_cuda(p_out, "p_out");
  check_f32_cuda(y_out, "y_out");
  check_f32_cuda(mask_out, "mask_out");
  const long R = vals.numel(), B = wid.numel();
  TORCH_CHECK(R >= 1 && R < (1L << 31) && B >= 1 && B < (1L << 31), "predict_emit: row sizes");
  TORCH_CHECK(y.numel() == R && mask.numel() == R, "predict_emit: vals, y and mask must have R elements each");
  TORCH_CHECK(wid.scalar_type() == at::kLong && wid.is_contiguous() && wid.is_cuda(), "predict_emit: wid int64");
  TORCH_CHECK(p_out.dim() == 2 && p_out.size(1) == R && y_out.sizes() == p_out.sizes() &&
                  mask_out.sizes() == p_out.sizes(),
              "predict_emit: output tables must be [rows_out, R]");
  const long rows_out = p_out.size(0);
  TORCH_CHECK(wid_out.scalar_type() == at::kLong && wid_out.is_contiguous() && wid_out.is_cuda() &&
                  wid_out.dim() == 2 && wid_out.size(0) == rows_out && wid_out.size(1) == B,
              "predict_emit: wid table must be int64 [rows_out, B]");
  TORCH_CHECK(cursor.scalar_type() == at::kLong && cursor.numel() >= 1 && cursor.is_cuda(),
              "predict_emit: cursor must be int64[1] on the device");
  c10::DeviceGuard guard(vals.device());
  hipLaunchKernelGGL(predict_emit_kernel, dim3(1), dim3(256), 0, stream(), vals.data_ptr<float>(),
                     y.data_ptr<float>(), mask.data_ptr<float>(), wid.data_ptr<long>(), p_out.data_ptr<float>(),
                     y_out.data_ptr<float>(), mask_out.data_ptr<float>(), wid_out.data_ptr<long>(),
                     cursor.data_ptr<long>(), rows_out, (int)R, (int)B, logits ? 1 : 0);
  GQ_LAUNCH_CHECK();
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("series_tm_gather", &gq::series_tm_gather);
  m.impl("predict_emit", &gq::predict_emit);
}
