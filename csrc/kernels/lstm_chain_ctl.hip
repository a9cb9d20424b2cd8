// Host side that the forward and the backward LSTM chain share (no kernels): the per-device control
// words, trace and phase-clock buffers, the co-residency capacity, and the ops that read them.
#include "lstm_chain_common.h"

namespace gq {

long long* chain_trace_buf(int dev) {
  static long long* tr[64] = {nullptr};
  // [0, 512): per-workgroup start / end; [512, 768): stage-loop start (backward)
  if (!tr[dev]) TORCH_CHECK(hipMalloc(&tr[dev], 3 * 256 * sizeof(long long)) == hipSuccess, "lstm_chain: trace");
  return tr[dev];
}

// tile 0's per-step phase clocks [CHAIN_MAX stages][CHAIN_PROF_ROWS][8] of the last launch with
// GNNQC_CHAIN_PROF=1 (forward and backward use the same buffer)
static constexpr size_t CHAIN_PROF_BYTES = CHAIN_MAX * CHAIN_PROF_ROWS * 8 * sizeof(long long);
long long* chain_prof_buf(int dev) {
#ifdef GQ_CHAIN_PROF
  static const bool on = [] {
    const char* e = std::getenv("GNNQC_CHAIN_PROF");
    return e != nullptr && e[0] == '1';
  }();
#else
  const bool on = false;
#endif
  if (!on) return nullptr;
  static long long* pb[64] = {nullptr};
  if (!pb[dev]) {
    TORCH_CHECK(hipMalloc(&pb[dev], CHAIN_PROF_BYTES) == hipSuccess && hipMemset(pb[dev], 0, CHAIN_PROF_BYTES) == hipSuccess,
                "chain prof");
  }
  return pb[dev];
}

// zero the phase-clock buffer before a profiled launch: a stage with fewer than CHAIN_PROF_STEPS
// steps (or fewer marks) than the previous launch's would otherwise leave that launch's rows behind
// (the round-4 table's backward rows 0-1 and m6 columns were such leftovers)
void chain_prof_clear(int dev) {
  long long* pb = chain_prof_buf(dev);
  if (pb != nullptr) TORCH_CHECK(hipMemsetAsync(pb, 0, CHAIN_PROF_BYTES, stream()) == hipSuccess, "chain prof clear");
}
long long* chain_prof_rows(int dev, int s) {   // stage s's rows of it (nullptr: off)
  long long* pb = chain_prof_buf(dev);
  return pb != nullptr ? pb + (size_t)s * CHAIN_PROF_ROWS * 8 : nullptr;
}

// a copy of one of the buffers above as a new tensor on like's device
static at::Tensor chain_copy(const at::Tensor& like, const void* p, at::IntArrayRef shape, at::ScalarType dt, const char* what) {
  at::Tensor o = at::empty(shape, like.options().dtype(dt));
  TORCH_CHECK(hipMemcpyAsync(o.data_ptr(), p, o.nbytes(), hipMemcpyDeviceToDevice, stream()) == hipSuccess, what);
  return o;
}

at::Tensor lstm_chain_prof(const at::Tensor& like) {
  c10::DeviceGuard guard(like.device());
  long long* p = chain_prof_buf(like.get_device());
  TORCH_CHECK(p != nullptr, "lstm_chain_prof: build with GNNQC_CHAIN_PROF_BUILD=1 and set GNNQC_CHAIN_PROF=1 "
                            "before the first chain launch");
  return chain_copy(like, p, {CHAIN_MAX, CHAIN_PROF_ROWS, 8}, at::kLong, "lstm_chain_prof");
}

int* chain_ctl(int dev) {
  static int* ctl[64] = {nullptr};
  TORCH_CHECK(dev >= 0 && dev < 64, "lstm_chain: device index");
  if (!ctl[dev]) {
    hipStreamCaptureStatus cs;
    TORCH_CHECK(hipStreamIsCapturing(stream(), &cs) == hipSuccess && cs == hipStreamCaptureStatusNone,
                "lstm_chain: first use must not be inside a graph capture");
    int* p = nullptr;
    TORCH_CHECK(hipMalloc(&p, 16 * sizeof(int)) == hipSuccess, "lstm_chain: control word allocation");
    const int init[16] = {1, 0};     // epoch 1; [4], [5]: head tickets; [8]: head backward reduce arrivals
    TORCH_CHECK(hipMemcpy(p, init, sizeof(init), hipMemcpyHostToDevice) == hipSuccess, "lstm_chain: init");
    ctl[dev] = p;
  }
  return ctl[dev];
}

// Workgroups of the chain kernels that can be resident at once on this device: the CU count
// of the device (a partitioned MI355X exposes fewer) times the occupancy of the 1024-thread
// chain kernels (with their LDS and VGPR use). Every workgroup of a chain launch must be
// resident, or consumers spin on producers that are never scheduled.
int chain_capacity(int dev) {
  static int cap[64] = {0};
  TORCH_CHECK(dev >= 0 && dev < 64, "lstm_chain: device index");
  if (cap[dev] == 0) {
    hipDeviceProp_t prop;
    TORCH_CHECK(hipGetDeviceProperties(&prop, dev) == hipSuccess, "lstm_chain: device properties");
    const int occ = std::min(chain_fwd_occupancy(), chain_bwd_occupancy());
    cap[dev] = std::max(0, occ) * prop.multiProcessorCount;
  }
  return cap[dev];
}

int64_t lstm_chain_capacity(const at::Tensor& like) {
  TORCH_CHECK(like.is_cuda(), "lstm_chain_capacity: a GPU tensor names the device");
  return chain_capacity(like.get_device());
}

// The device's chain control words as an int32[16] view (no copy): [epoch, finished workgroups,
// spin-timeout flag, timeouts consumed by the gradient guard, time4/head kernel tickets (2),
// debug spin limit (0: default), a gradient producer saw a non-finite value, head backward
// reduce arrivals, 0...]. The optimiser's update reads and clears the flags inside the captured
// step (a timed-out or non-finite step is skipped, never applied).
at::Tensor lstm_chain_ctl(const at::Tensor& like) {
  TORCH_CHECK(like.is_cuda(), "lstm_chain_ctl: a GPU tensor names the device");
  c10::DeviceGuard guard(like.device());
  int* p = chain_ctl(like.get_device());
  return at::from_blob(p, {16}, like.options().dtype(at::kInt));
}

// a copy of this device's first 12 chain control words (tests): [0] epoch, [1] finished workgroups,
// [2] spin timeout, [3] rejected steps, .., [9] consumer re-polls
at::Tensor lstm_chain_status(const at::Tensor& like) {
  c10::DeviceGuard guard(like.device());
  return chain_copy(like, chain_ctl(like.get_device()), {12}, at::kInt, "lstm_chain_status");
}

// [blocks, 2] start / end timestamps (s_memrealtime ticks) of the last chain launch (profiling)
at::Tensor lstm_chain_trace(const at::Tensor& like) {
  c10::DeviceGuard guard(like.device());
  return chain_copy(like, chain_trace_buf(like.get_device()), {3 * 256}, at::kLong, "lstm_chain_trace");
}

}  // namespace gq

TORCH_LIBRARY_IMPL(gnnqc, CUDA, m) {
  m.impl("lstm_chain_status", &gq::lstm_chain_status);
  m.impl("lstm_chain_capacity", &gq::lstm_chain_capacity);
  m.impl("lstm_chain_ctl", &gq::lstm_chain_ctl);
  m.impl("lstm_chain_trace", &gq::lstm_chain_trace);
  m.impl("lstm_chain_prof", &gq::lstm_chain_prof);
}
