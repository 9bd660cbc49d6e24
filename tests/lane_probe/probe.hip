// The lane probe on the DEVICE backends: one small kernel per backend that loads in[block][lane][k], calls the primitive an
// integer selects (probe.hpp) and stores out[block][lane][k] - and a C entry point that uploads, launches, waits and
// downloads.  Built with the flags of libmpmpc.so into tests/_build/liblaneprobe.so (__graft_entry__.py: build_lane_probe);
// no inline assembly here, only what lane_gpu.hpp contains.
// SLOTS = 4 on every backend: the cold storage only has to hold the two (pair: 2 x 2) slots of the round trip.  On the
// workgroup backends SLOTS moves nothing but the offsets of xrow / rrow / erow inside the dynamic LDS (lane_gpu.hpp:
// LaneBlock), which so stays at 27 KB for 256 lanes - below the 64 KB a kernel gets without raising a limit.
#include <hip/hip_runtime.h>

#include <cstddef>

#define MPMPC_HD __device__ __forceinline__
#define MPMPC_HOST_DEVICE __host__ __device__
#include "lane_gpu.hpp"
#include "lane_pair.hpp"
#include "mpmpc_core.hpp"
#include "probe.hpp"

namespace lane_probe {

constexpr int SLOTS = 4;

template <class L, int KIND, int T>
__global__ void __launch_bounds__(T) probe_kernel(int op, int arg, const double* in, double* out, double* mem, int* imem, int* status) {
  using R = typename L::real;
  constexpr int NX = KIND == PAIR ? K / 2 : K;
  const size_t base = ((size_t)blockIdx.x * T + threadIdx.x) * K;
  R x[NX], y[NX];
  if constexpr (KIND == PAIR) {
    for (int k = 0; k < NX; ++k) x[k] = R(in[base + k], in[base + NX + k]);
  } else {
    for (int k = 0; k < NX; ++k) x[k] = in[base + k];
  }
  const bool known = run_op<L, KIND>(op, arg, x, y, mem, imem);
  if (!known && threadIdx.x == 0) status[0] = 1;
  if constexpr (KIND == PAIR) {
    for (int k = 0; k < NX; ++k) { out[base + k] = y[k].v[0]; out[base + NX + k] = y[k].v[1]; }
  } else {
    for (int k = 0; k < NX; ++k) out[base + k] = y[k];
  }
}

struct DeviceBuffer {
  void* p = nullptr;
  ~DeviceBuffer() { if (p) (void)hipFree(p); }
};
#define PROBE_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

struct Call {
  int op, arg, blocks;
  const double* in;
  double* out;
  double* mem;
  int mem_n;
  int* imem;
  int imem_n;
};

template <class L, int KIND, int T>
int launch(const Call& c, size_t lds) {
  const size_t n = (size_t)c.blocks * T * K;
  DeviceBuffer din, dout, dmem, dimem, dstatus;
  PROBE_TRY(hipMalloc(&din.p, n * sizeof(double)));
  PROBE_TRY(hipMalloc(&dout.p, n * sizeof(double)));
  PROBE_TRY(hipMalloc(&dmem.p, (size_t)(c.mem_n > 0 ? c.mem_n : 1) * sizeof(double)));
  PROBE_TRY(hipMalloc(&dimem.p, (size_t)(c.imem_n > 0 ? c.imem_n : 1) * sizeof(int)));
  PROBE_TRY(hipMalloc(&dstatus.p, sizeof(int)));
  PROBE_TRY(hipMemcpy(din.p, c.in, n * sizeof(double), hipMemcpyHostToDevice));
  PROBE_TRY(hipMemset(dout.p, 0xff, n * sizeof(double)));
  PROBE_TRY(hipMemset(dstatus.p, 0, sizeof(int)));
  if (c.mem_n > 0) PROBE_TRY(hipMemcpy(dmem.p, c.mem, (size_t)c.mem_n * sizeof(double), hipMemcpyHostToDevice));
  if (c.imem_n > 0) PROBE_TRY(hipMemcpy(dimem.p, c.imem, (size_t)c.imem_n * sizeof(int), hipMemcpyHostToDevice));
  hipLaunchKernelGGL((probe_kernel<L, KIND, T>), dim3(c.blocks), dim3(T), lds, 0, c.op, c.arg, (const double*)din.p, (double*)dout.p,
                     (double*)dmem.p, (int*)dimem.p, (int*)dstatus.p);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  int status = 0;
  PROBE_TRY(hipMemcpy(&status, dstatus.p, sizeof(int), hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(c.out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
  if (c.mem_n > 0) PROBE_TRY(hipMemcpy(c.mem, dmem.p, (size_t)c.mem_n * sizeof(double), hipMemcpyDeviceToHost));
  if (c.imem_n > 0) PROBE_TRY(hipMemcpy(c.imem, dimem.p, (size_t)c.imem_n * sizeof(int), hipMemcpyDeviceToHost));
  return status ? -2 : 0;
}

using Blk128 = LaneBlock<128, SLOTS>;
using Blk256 = LaneBlock<256, SLOTS>;
using Blk128One = LaneBlock<128, SLOTS, 128, 4>;     // (XR = 4: the exchange rows of the pair kernels)

}  // namespace lane_probe

using namespace lane_probe;

extern "C" int lane_probe_op_count() { return N_OPS; }
extern "C" const char* lane_probe_op_name(int op) { return op_name(op); }
// lanes of one block of this backend (0: no such backend in this build)
extern "C" int lane_probe_threads(int backend) {
  switch (backend) {
    case G64C16: case G64C32: case G32C16: case G16C16: case G64C64: case P16: case P64: return 64;
    case B128: case B128CH128: case P128: return 128;
    case B256: return 256;
    default: return 0;
  }
}
// 0: done; -1: bad arguments; -2: the backend has no such primitive; > 0: the hipError_t of the call that failed
extern "C" int lane_probe_run(int backend, int op, int arg, int blocks, const double* in, double* out, double* mem, int mem_n,
                              int* imem, int imem_n) {
  if (blocks < 1 || blocks > 4 || op < 0 || op >= N_OPS || !in || !out || mem_n < 0 || imem_n < 0) return -1;
  const Call c{op, arg, blocks, in, out, mem, mem_n, imem, imem_n};
  switch (backend) {
    case G64C16: return launch<LaneGpu<64, 16, SLOTS>, WAVE, 64>(c, 0);
    case G64C32: return launch<LaneGpu<64, 32, SLOTS>, WAVE, 64>(c, 0);
    case G32C16: return launch<LaneGpu<32, 16, SLOTS>, WAVE, 64>(c, 0);
    case G16C16: return launch<LaneGpu<16, 16, SLOTS>, WAVE, 64>(c, 0);
    case G64C64: return launch<LaneGpu<64, 64, SLOTS>, WAVE, 64>(c, 0);
    case B128: return launch<Blk128, BLOCK, 128>(c, Blk128::lds_bytes);
    case B256: return launch<Blk256, BLOCK, 256>(c, Blk256::lds_bytes);
    case B128CH128: return launch<Blk128One, BLOCK, 128>(c, Blk128One::lds_bytes);
    case P16: return launch<LanePair<LaneGpu<16, 16, SLOTS>>, PAIR, 64>(c, 0);
    case P64: return launch<LanePair<LaneGpu<64, 64, SLOTS>>, PAIR, 64>(c, 0);
    case P128: return launch<LanePair<Blk128One>, PAIR, 128>(c, Blk128One::lds_bytes);
    default: return -1;
  }
}
