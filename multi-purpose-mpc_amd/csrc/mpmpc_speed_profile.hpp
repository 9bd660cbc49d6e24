// The speed profile of libmpmpc.so, part of the one translation unit mpmpc_hip.hip: the two K4 kernels, the per-device scratch
// and the entry point mpmpc_speed_profile (speed_core.hpp is the solver they run).  Needs no handle.
#pragma once

// K4: speed profile.  The kernel of choice is mpmpc_speed_profile_wave_kernel below (one wavefront per path); this
// one runs the same code one thread per path (a serial interior-point / active-set run over a scalar tridiagonal
// system, speed_core.hpp) for paths too long for the LDS: workspace path-minor in HBM, so that the threads of a
// wave touch consecutive addresses.
__global__ __launch_bounds__(64) void mpmpc_speed_profile_kernel(int B, int n, const double* __restrict__ li,
                                                                 const double* __restrict__ kappa,
                                                                 const double* __restrict__ limits, double eps,
                                                                 double* __restrict__ work, double* __restrict__ v,
                                                                 int* __restrict__ status, int* __restrict__ iters) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= B) return;
  SpWork W{work + p, n, B};
  SpLimits lim{limits[5 * p], limits[5 * p + 1], limits[5 * p + 2], limits[5 * p + 3], limits[5 * p + 4]};
  int it = 0;
  status[p] = sp_solve(n, li + (long)p * n, kappa + (long)p * n, 1, lim, eps, W, v + (long)p * n, 1, &it);
  iters[p] = it;
}

// One WAVEFRONT per path: the elementwise loops of sp_solve_t run strided over the 64 lanes, reductions are
// shuffles, and the tridiagonal systems are solved by parallel cyclic reduction in LDS (sp_cr_factor / sp_cr_solve of
// speed_core.hpp, whose rows the lanes share out).  Everything (the SP_ARRAYS work arrays + sp_cr_arrays(n) arrays of
// cyclic-reduction state, n doubles each) lives in LDS.
struct SpWave {
  SpCyclic cr;        // cyclic-reduction state behind the SP_ARRAYS work arrays
  __device__ int first() const { return threadIdx.x; }
  __device__ int step() const { return 64; }
  __device__ void sync() const { __syncthreads(); }
  __device__ double rmax(double v) const {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
  }
  __device__ double rsum(double v) const {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
  }
  __device__ bool any(bool b) const { __syncthreads(); return __ballot(b) != 0ull; }
  __device__ void tri_factor(const SpWork& W, int n) const { sp_cr_factor(*this, cr, W, n); }
  __device__ void tri_solve(const SpWork& W, int n) const { sp_cr_solve(*this, cr, W, n); }
};
__global__ __launch_bounds__(64) void mpmpc_speed_profile_wave_kernel(int B, int n, const double* __restrict__ li,
                                                                      const double* __restrict__ kappa,
                                                                      const double* __restrict__ limits, double eps,
                                                                      double* __restrict__ v, int* __restrict__ status,
                                                                      int* __restrict__ iters) {
  extern __shared__ double sp_lds[];
  const int p = blockIdx.x;
  if (p >= B) return;
  SpWork W{sp_lds, n, 1};
  SpWave pol{{sp_lds + (long)SP_ARRAYS * n, n}};
  SpLimits lim{limits[5 * p], limits[5 * p + 1], limits[5 * p + 2], limits[5 * p + 3], limits[5 * p + 4]};
  int it = 0;
  const int st = sp_solve_t(pol, n, li + (long)p * n, kappa + (long)p * n, 1, lim, eps, W, v + (long)p * n, 1, &it);
  if (threadIdx.x == 0) { status[p] = st; iters[p] = it; }
}

// device scratch of mpmpc_speed_profile (device_scratch.hpp: one per device, kept between calls, never freed)
static SpScratch g_sp_dev[SP_MAX_DEVICES];

extern "C" int mpmpc_speed_profile(int32_t device, int32_t B, int32_t n, const double* li, const double* kappa,
                        const double* limits, double eps, double* v, int32_t* status, int32_t* iters) {
  if (B < 1 || n < 2) return fail(MPMPC_E_ARG, "speed profile needs B >= 1 paths of n >= 2 segments");
  if (!li || !kappa || !limits || !v || !status) return fail(MPMPC_E_ARG, "li, kappa, limits, v, status must not be NULL");
  const size_t nb = (size_t)B, vec = nb * n;
  const size_t lds_wave = sizeof(double) * (SP_ARRAYS + sp_cr_arrays(n)) * (size_t)n;
  // one wavefront per path while its arrays fit 156 KiB of LDS: n <= 384, where 8 (25 + 9 + 2 * 9) 384 = 159 744 B is
  // 156 KiB exactly; beyond that one thread per path.  (A kernel that ran one thread per path out of 64 KiB of LDS,
  // 25 * 8 n <= 65 536: n <= 327, could never be chosen - the wave kernel takes every such n - and is gone.)
  const bool wave = lds_wave <= 156 * 1024;
  Layout L;
  const auto r_li = L.add<double>(vec), r_kappa = L.add<double>(vec), r_v = L.add<double>(vec), r_lim = L.add<double>(5 * nb),
             r_work = L.add<double>(wave ? 0 : vec * SP_ARRAYS);      // (the HBM workspace of the thread-per-path kernel)
  const auto r_status = L.add<int>(nb), r_iters = L.add<int>(nb);
  Scratch sc;
  if (int rc = scratch_acquire(g_sp_dev, device, L.bytes(), "speed-profile", &sc)) return rc;
  hipStream_t stream = sc.stream;
  char* blk = sc.blk;
  HIP_TRY(hipMemcpyAsync(r_li.at(blk), li, r_li.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_kappa.at(blk), kappa, r_kappa.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_lim.at(blk), limits, r_lim.bytes(), hipMemcpyHostToDevice, stream));
  if (wave) {
    // one wavefront per path (any batch size): lane-parallel arithmetic, cyclic reduction for the tridiagonal solves
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&mpmpc_speed_profile_wave_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_wave));
    hipLaunchKernelGGL(mpmpc_speed_profile_wave_kernel, dim3(B), dim3(64), lds_wave, stream, B, n, r_li.at(blk), r_kappa.at(blk),
                       r_lim.at(blk), eps, r_v.at(blk), r_status.at(blk), r_iters.at(blk));
  } else {
    hipLaunchKernelGGL(mpmpc_speed_profile_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, B, n, r_li.at(blk), r_kappa.at(blk),
                       r_lim.at(blk), eps, r_work.at(blk), r_v.at(blk), r_status.at(blk), r_iters.at(blk));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(stream, v, r_v.at(blk), vec));
  HIP_TRY(pull(stream, status, r_status.at(blk), nb));
  HIP_TRY(pull(stream, iters, r_iters.at(blk), nb));
  HIP_TRY(hipStreamSynchronize(stream));
  return MPMPC_OK;
}
