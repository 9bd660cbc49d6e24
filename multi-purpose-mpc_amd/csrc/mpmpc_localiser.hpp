// Lidar localisation of the rollout, part of the one translation unit mpmpc_hip.hip (included behind mpmpc_estimator.hpp and in
// front of mpmpc_closed_loop.hpp; the step loop of mpmpc_rollout_step.hpp launches K3l and, in front of it, K0l): the kernels K0d
// (the distance field of the base map) and K3l (the scan match of every running car), the handle-free entry points
// mpmpc_distance_field / mpmpc_scan_match and the handle's mpmpc_rollout_set_localiser / mpmpc_rollout_localiser.  The law:
// localiser_core.hpp.  The state: the sub-state lc of the handle (mpmpc_handle.hpp).
#pragma once

constexpr int LC_THREADS = 256;

// K0d: one thread per cell of the grid, integers only.  Every read is clipped to the grid (lc_field_cell).
__global__ __launch_bounds__(256) void mpmpc_distance_field_kernel(MapView map, int D, uint8_t* __restrict__ field) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)map.height * map.width) return;
  const int j = (int)(g / map.width), i = (int)(g - (long long)j * map.width);
  field[g] = (uint8_t)lc_field_cell(map, i, j, D);
}

// The match of ONE car by its workgroup of LC_THREADS lanes (steps 3 - the hits - and 4 of the law).  range(b, &hit): the range
// of beam b, already noisy, and whether the beam is a hit.  end: dynamic LDS, (2 T + 1) * n_beams cells of 8 bytes - slot
// (t + T) * n_beams + b holds the endpoint cell of beam b under heading t (x = LC_SKIP: no hit, LC_BAD: a BAD endpoint).
//   1  the lanes stride over the beams; a lane takes its beam's range once and writes the beam's 2 T + 1 cells
//   2  the lanes stride over the candidates idx (a fastest: the lanes of a wave read neighbouring bytes of the field, which is
//      L2-resident and shared by the fleet; the LDS reads of a wave are broadcasts wherever its lanes share t); each sums its
//      hits' field bytes in int32 and keeps the smallest key it saw
//   3  the minimum of the keys through the wave (a butterfly), then through LDS; every lane returns it
// Returns ~0 when there is no match (hits < min_hits or the prior is not finite); *hits: the number of hits.  The minimum of
// 64-bit integers is order-free, so no output bit depends on how candidates fall on lanes.  Every LDS index is below
// (2 T + 1) * n_beams <= LC_MAX_ENDPOINTS (the host refuses more), every field index is checked against the grid (lc_field_at).
template <class Range>
__device__ __forceinline__ unsigned long long lc_block_match(const MapView& map, const uint8_t* __restrict__ F, const LcSet& s, int n_beams,
                                                             const double* __restrict__ angles, const double* prior, Range range,
                                                             int2* end, int* hits) {
  __shared__ int s_hits;
  __shared__ unsigned long long s_key[LC_THREADS / 64];
  const int tid = threadIdx.x;
  const bool prior_ok = lc_pose_finite(prior);
  if (tid == 0) s_hits = 0;
  __syncthreads();
  for (int b = tid; b < n_beams; b += LC_THREADS) {
    bool hit;
    const double r = range(b, &hit);
    if (hit) atomicAdd(&s_hits, 1);
    if (!prior_ok) continue;
    const double ang = angles[b];
    for (int t = -s.T; t <= s.T; ++t) {
      int2 e = make_int2(LC_SKIP, 0);
      if (hit) {
        double qx, qy;
        if (!lc_endpoint(map, prior[0], prior[1], prior[2] + (double)t * s.step_psi, ang, r, &e.x, &e.y, &qx, &qy)) e = make_int2(LC_BAD, 0);
      }
      end[(t + s.T) * n_beams + b] = e;
    }
  }
  __syncthreads();
  *hits = s_hits;
  if (*hits < s.min_hits || !prior_ok) return ~0ull;      // (uniform)
  const int cap = lc_cap(s.D), n_cand = lc_candidates(s.W, s.T);
  unsigned long long best = ~0ull;
  for (int idx = tid; idx < n_cand; idx += LC_THREADS) {
    int a, c, t;
    lc_candidate(idx, s.W, s.T, &a, &c, &t);
    const long long sa = (long long)a * s.m, sc = (long long)c * s.m;
    const int2* row = end + (t + s.T) * n_beams;
    int sum = 0;
    for (int b = 0; b < n_beams; ++b) {
      const int2 e = row[b];
      if (e.x == LC_SKIP) continue;
      sum += e.x == LC_BAD ? cap : lc_field_at(F, map.width, map.height, cap, e.x + sa, e.y + sc);
    }
    const unsigned long long key = lc_key(sum, a, c, t, idx);
    best = key < best ? key : best;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long other = __shfl_xor(best, d, 64);
    best = other < best ? other : best;
  }
  if ((tid & 63) == 0) s_key[tid >> 6] = best;
  __syncthreads();
  best = s_key[0];
  for (int w = 1; w < LC_THREADS / 64; ++w) best = s_key[w] < best ? s_key[w] : best;
  return best;
}

// mpmpc_scan_match: one workgroup per (prior, scan) pair, no noise
__global__ __launch_bounds__(LC_THREADS) void mpmpc_scan_match_kernel(MapView map, const uint8_t* __restrict__ F, LcSet s, int B, int n_beams,
                                                                      const double* __restrict__ angles, double range_m,
                                                                      const double* __restrict__ prior, const double* __restrict__ ranges,
                                                                      double* __restrict__ fix, int* __restrict__ out) {
  extern __shared__ int2 s_lc_end[];
  const int i = blockIdx.x;
  if (i >= B) return;      // (uniform)
  const double pr[3] = {prior[3L * i], prior[3L * i + 1], prior[3L * i + 2]};
  const double* rg = ranges + (long)i * n_beams;
  int hits;
  const unsigned long long key = lc_block_match(map, F, s, n_beams, angles, pr, [&](int b, bool* hit) {
    const double r = rg[b];
    *hit = r < range_m;
    return r;
  }, s_lc_end, &hits);
  if (threadIdx.x != 0) return;
  double fx[3] = {pr[0], pr[1], pr[2]};
  int cand = -1, score = -1;
  if (key != ~0ull) {
    int a, c, t;
    cand = (int)(key & 0x7fffu);
    score = (int)(key >> 32);
    lc_candidate(cand, s.W, s.T, &a, &c, &t);
    lc_fix(pr, s, map.res, a, c, t, fx);
  }
  for (int e = 0; e < 3; ++e) fix[3L * i + e] = fx[e];
  out[i] = score;
  out[B + i] = cand;
  out[2L * B + i] = hits;
}

// what K3l takes of the localiser
struct LocView {
  unsigned long long seed;
  int car0;
  long long j;             // k - step0 of the step
  int scheduled;           // lc_scheduled(j, period): K0l ran in front and `ranges` are the step's
  LcSet set;
  const uint8_t* F;        // [height][width]
  int n_beams;
  const double* angles;    // [n_beams]
  double range_m;
  double* ranges;          // [B][n_beams]
  double *fix, *prior;     // [B][3] each
  int* primed;             // [B]
  int* out;                // [3][ld]: cand, score, hits
  double* stats;           // [LC_STATS][ld]
  int* count;              // [LC_COUNTS][ld]
  long ld;                 // max_batch
};

// K3l: one step of every running car, one WORKGROUP per car, launched behind K3n and K0l and in front of K3e / K3d / K3a.  Lane 0
// takes the car's state and makes the prior (K3e's command rule: u, or entry assumed[i] of the register); on a scheduled step
// of a primed car the workgroup matches (lc_block_match - the hits' ranges are made noisy in place, each by the lane that
// reads it); lane 0 writes the fix, what the step leaves and the statistics.  A car with alive != 1 is not touched.
__global__ __launch_bounds__(LC_THREADS) void mpmpc_scan_localise_kernel(MapView map, int B, double L, double Ts,
                                                                         const double* __restrict__ pose, const int* __restrict__ alive,
                                                                         const double* __restrict__ u, const double* __restrict__ queue,
                                                                         const int* __restrict__ assumed, LocView v) {
  extern __shared__ int2 s_lc_end[];
  __shared__ double s_prior[3];
  __shared__ int s_mode;      // 0 priming, 1 not scheduled, 2 scan
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= B || alive[i] != 1) return;      // (uniform)
  const double pp[3] = {pose[3L * i], pose[3L * i + 1], pose[3L * i + 2]};
  if (tid == 0) {
    double pr[3] = {pp[0], pp[1], pp[2]};
    int mode = 0;
    if (v.primed[i]) {
      const double* cmd = queue ? queue + 2L * DL_MAX * i + 2 * assumed[i] : u + 2L * i;      // (assumed < DL_MAX: plan_step)
      const double zero[3] = {0.0, 0.0, 0.0};
      double sd = 0.0;
      for (int e = 0; e < 3; ++e) pr[e] = v.fix[3L * i + e];
      dl_nominal(L, Ts, cmd[0], cmd[1], zero, 0.0, pr, &sd);
      mode = v.scheduled ? 2 : 1;
    }
    for (int e = 0; e < 3; ++e) s_prior[e] = pr[e];
    s_mode = mode;
  }
  __syncthreads();
  const double pr[3] = {s_prior[0], s_prior[1], s_prior[2]};
  const int mode = s_mode;
  unsigned long long key = ~0ull;
  int hits = -1;
  if (mode == 2) {      // (uniform)
    double* rg = v.ranges + (long)i * v.n_beams;
    key = lc_block_match(map, v.F, v.set, v.n_beams, v.angles, pr, [&](int b, bool* hit) {
      double r = rg[b];
      *hit = r < v.range_m;
      if (*hit) {
        r = lc_noisy(r, v.set.sigma_r, v.seed, (uint32_t)(v.car0 + i), v.j, b);
        rg[b] = r;
      }
      return r;
    }, s_lc_end, &hits);
  }
  if (tid != 0) return;
  double fx[3] = {pr[0], pr[1], pr[2]}, st[LC_STATS];
  int cnt[LC_COUNTS], cand = -1, score = -1;
  for (int e = 0; e < LC_STATS; ++e) st[e] = v.stats[e * v.ld + i];
  for (int e = 0; e < LC_COUNTS; ++e) cnt[e] = v.count[e * v.ld + i];
  if (mode == 2) {
    if (key == ~0ull) {
      cnt[2] += 1;
    } else {
      int a, c, t;
      cand = (int)(key & 0x7fffu);
      score = (int)(key >> 32);
      lc_candidate(cand, v.set.W, v.set.T, &a, &c, &t);
      lc_fix(pr, v.set, map.res, a, c, t, fx);
      cnt[1] += 1;
      if (lc_on_edge(a, c, t, v.set.W, v.set.T)) cnt[3] += 1;
    }
  }
  lc_stats(fx, pr, pp, st, cnt);
  for (int e = 0; e < 3; ++e) {
    v.fix[3L * i + e] = fx[e];
    v.prior[3L * i + e] = pr[e];
  }
  v.primed[i] = 1;
  v.out[i] = cand;
  v.out[v.ld + i] = score;
  v.out[2 * v.ld + i] = hits;
  for (int e = 0; e < LC_STATS; ++e) v.stats[e * v.ld + i] = st[e];
  for (int e = 0; e < LC_COUNTS; ++e) v.count[e * v.ld + i] = cnt[e];
}

static size_t loc_lds(int T, int n_beams) { return sizeof(int2) * (size_t)(2 * T + 1) * (size_t)n_beams; }

// every car un-primed (or primed with fix0) and the statistics zero, on the slot's stream
static int loc_reset(mpmpc_handle h, Slot& sl, int B, const double* fix0) {
  const size_t mb = (size_t)h->cfg.max_batch;
  LocState& lc = h->lc;
  HIP_TRY(hipMemsetAsync(lc.fix, 0, sizeof(double) * 3 * mb, sl.stream));
  HIP_TRY(hipMemsetAsync(lc.prior, 0, sizeof(double) * 3 * mb, sl.stream));
  HIP_TRY(hipMemsetAsync(lc.primed, 0, sizeof(int) * mb, sl.stream));
  if (fix0) {
    const std::vector<int> ones((size_t)B, 1);
    HIP_TRY(hipMemcpyAsync(lc.fix, fix0, sizeof(double) * 3 * B, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemcpyAsync(lc.primed, ones.data(), sizeof(int) * B, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));      // (`ones` has been read)
  }
  HIP_TRY(hipMemsetAsync(lc.out, 0xff, sizeof(int) * 3 * mb, sl.stream));      // cand, score, hits: -1
  HIP_TRY(hipMemsetAsync(lc.ranges, 0, sizeof(double) * mb * (size_t)lc.n_beams, sl.stream));
  HIP_TRY(hipMemsetAsync(lc.stats, 0, sizeof(double) * LC_STATS * mb, sl.stream));
  HIP_TRY(hipMemsetAsync(lc.count, 0, sizeof(int) * LC_COUNTS * mb, sl.stream));
  lc.ran = false;
  return MPMPC_OK;
}

static LocView loc_view(mpmpc_handle h, long long k) {
  const LocState& lc = h->lc;
  const long long j = k - lc.step0;
  return LocView{lc.seed, lc.car0, j, lc_scheduled(j, lc.period) ? 1 : 0, lc.set, lc.field, lc.n_beams, lc.angles, lc.range, lc.ranges,
                 lc.fix, lc.prior, lc.primed, lc.out, lc.stats, lc.count, (long)h->cfg.max_batch};
}

// device scratch of mpmpc_distance_field and mpmpc_scan_match, which share it (device_scratch.hpp)
static SpScratch g_loc_dev[SP_MAX_DEVICES];

static int loc_check_map(int height, int width, const int8_t* data, const char** why) {
  if (height < 1 || width < 1) { *why = "map needs positive size"; return -1; }
  if (height > COR_MAX_SIDE || width > COR_MAX_SIDE) { *why = "map sides are limited to 65534 cells"; return -1; }
  if (!data) { *why = "data must not be NULL"; return -1; }
  return 0;
}

static void loc_enqueue_field(const MapView& mv, int D, uint8_t* field, hipStream_t stream) {
  const long long cells = (long long)mv.height * mv.width;
  hipLaunchKernelGGL(mpmpc_distance_field_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, mv, D, field);
}

extern "C" {

int mpmpc_distance_field(int32_t device, int32_t height, int32_t width, const int8_t* data, int32_t D, uint8_t* field_out) {
  const char* why = "";
  if (loc_check_map(height, width, data, &why)) return fail(MPMPC_E_ARG, why);
  if (!field_out) return fail(MPMPC_E_ARG, "field_out must not be NULL");
  if (D < 1 || D > LC_MAX_D) return fail(MPMPC_E_ARG, "localiser: D must be in [1, 15] cells");
  const size_t cells = (size_t)height * width;
  Layout L;
  const auto r_map = L.add<int8_t>(cells);
  const auto r_f = L.add<uint8_t>(cells);
  Scratch sc;
  if (int rc = scratch_acquire(g_loc_dev, device, L.bytes(), "localiser", &sc)) return rc;
  HIP_TRY(hipMemcpyAsync(r_map.at(sc.blk), data, cells, hipMemcpyHostToDevice, sc.stream));
  loc_enqueue_field(MapView{r_map.at(sc.blk), height, width, 0.0, 0.0, 1.0}, D, r_f.at(sc.blk), sc.stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(sc.stream, field_out, r_f.at(sc.blk), cells));
  HIP_TRY(hipStreamSynchronize(sc.stream));
  return MPMPC_OK;
}

int mpmpc_scan_match(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y, double resolution,
                     int32_t B, const double* prior, const double* ranges, int32_t n_beams, const double* angles, double range_m, int32_t D,
                     int32_t m, int32_t W, int32_t T, double step_psi, int32_t min_hits, double* fix_out, int32_t* score_out,
                     int32_t* cand_out, int32_t* hits_out) {
  const char* why = "";
  if (loc_check_map(height, width, data, &why)) return fail(MPMPC_E_ARG, why);
  if (!(resolution > 0.0) || !mov_finite(resolution)) return fail(MPMPC_E_ARG, "map needs a positive resolution");
  if (!mov_finite(origin_x) || !mov_finite(origin_y)) return fail(MPMPC_E_ARG, "the map's origin is not finite");
  if (B < 1) return fail(MPMPC_E_ARG, "B must be >= 1");
  if (!prior || !ranges || !fix_out || !score_out || !cand_out || !hits_out)
    return fail(MPMPC_E_ARG, "prior, ranges, fix_out, score_out, cand_out and hits_out must not be NULL");
  const LcSet set{D, m, W, T, min_hits, step_psi, 0.0};
  if (lc_check_setting(n_beams, angles, range_m, resolution, set, 1, B, nullptr, &why)) return fail(MPMPC_E_ARG, why);
  const size_t cells = (size_t)height * width, nb = (size_t)B;
  Layout L;
  const auto r_map = L.add<int8_t>(cells);
  const auto r_f = L.add<uint8_t>(cells);
  const auto r_ang = L.add<double>((size_t)n_beams), r_prior = L.add<double>(3 * nb), r_rg = L.add<double>(nb * (size_t)n_beams),
             r_fix = L.add<double>(3 * nb);
  // the kernel's `out` is ONE region [3][B]: score, candidate, hits
  const auto r_out = L.add<int>(3 * nb), r_score = r_out.part(0, nb), r_cand = r_out.part(nb, nb), r_hits = r_out.part(2 * nb, nb);
  Scratch sc;
  if (int rc = scratch_acquire(g_loc_dev, device, L.bytes(), "localiser", &sc)) return rc;
  char* blk = sc.blk;
  hipStream_t stream = sc.stream;
  HIP_TRY(hipMemcpyAsync(r_map.at(blk), data, cells, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_ang.at(blk), angles, r_ang.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_prior.at(blk), prior, r_prior.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_rg.at(blk), ranges, r_rg.bytes(), hipMemcpyHostToDevice, stream));
  const MapView mv{r_map.at(blk), height, width, origin_x, origin_y, resolution};
  loc_enqueue_field(mv, D, r_f.at(blk), stream);
  hipLaunchKernelGGL(mpmpc_scan_match_kernel, dim3(B), dim3(LC_THREADS), loc_lds(T, n_beams), stream, mv, r_f.at(blk), set, (int)B,
                     (int)n_beams, r_ang.at(blk), range_m, r_prior.at(blk), r_rg.at(blk), r_fix.at(blk), r_out.at(blk));
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(stream, fix_out, r_fix.at(blk), 3 * nb));
  HIP_TRY(pull(stream, score_out, r_score.at(blk), nb));
  HIP_TRY(pull(stream, cand_out, r_cand.at(blk), nb));
  HIP_TRY(pull(stream, hits_out, r_hits.at(blk), nb));
  HIP_TRY(hipStreamSynchronize(stream));
  return MPMPC_OK;
}

int mpmpc_rollout_set_localiser(mpmpc_handle h, int32_t B, int32_t n_beams, const double* angles, double range_m, int32_t D, int32_t m,
                                int32_t W, int32_t T, double step_psi, int32_t min_hits, double sigma_r, int32_t period, uint64_t seed,
                                int32_t car0, int64_t step0, const double* fix0) {
  if (int rc = enter(h)) return rc;
  LocState& lc = h->lc;
  if (B == 0) {      // off: the controller localises on the measured pose (plant) or the true one
    lc.B = 0;
    lc.ran = false;
    return MPMPC_OK;
  }
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  if (!h->cor.map) return fail(MPMPC_E_STATE, "the localiser needs mpmpc_set_map first");
  const LcSet set{D, m, W, T, min_hits, step_psi, sigma_r};
  const char* why = "";
  if (lc_check_setting(n_beams, angles, range_m, h->cor.map_res, set, period, B, fix0, &why)) return fail(MPMPC_E_ARG, why);
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t mb = (size_t)h->cfg.max_batch, cells = (size_t)h->cor.map_h * (size_t)h->cor.map_w;
  lc.B = 0;      // (a failure below leaves the localiser off)
  lc.ran = false;
  if (!lc.fix)
    HIP_TRY(alloc_all(Want{lc.fix, 3 * mb}, Want{lc.prior, 3 * mb}, Want{lc.primed, mb}, Want{lc.out, 3 * mb}, Want{lc.stats, LC_STATS * mb},
                      Want{lc.count, LC_COUNTS * mb}, Want{lc.angles, (size_t)LID_MAX_BEAMS}));
  if (lc.field.count() < cells) HIP_TRY(lc.field.alloc(cells));
  if (lc.ranges.count() < mb * (size_t)n_beams) HIP_TRY(lc.ranges.alloc(mb * (size_t)n_beams));
  lc.n_beams = n_beams;
  HIP_TRY(hipMemcpyAsync(lc.angles, angles, sizeof(double) * (size_t)n_beams, hipMemcpyHostToDevice, sl.stream));
  loc_enqueue_field(h->cor.map_view(), D, lc.field.get(), sl.stream);      // K0d: the field of the map of the moment
  HIP_TRY(hipGetLastError());
  if (int rc = loc_reset(h, sl, B, fix0)) return rc;
  HIP_TRY(hipStreamSynchronize(sl.stream));      // the caller's arrays have been read
  lc.set = set;
  lc.range = range_m;
  lc.period = period;
  lc.seed = seed;
  lc.car0 = car0;
  lc.step0 = step0;
  lc.gen = h->cor.base_gen;
  lc.B = B;
  return MPMPC_OK;
}

int mpmpc_rollout_localiser(mpmpc_handle h, int32_t B, double* fix, double* prior, int32_t* cand, int32_t* score, int32_t* hits, double* ranges,
                            double* err2_max, double* err2_sum, double* head2_sum, double* prior2_sum, int32_t* steps, int32_t* matched,
                            int32_t* lost, int32_t* edge) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B)) return rc;
  const LocState& lc = h->lc;
  if (lc.B != B || !lc.ran)
    return fail(MPMPC_E_STATE, "no rollout step of B cars ran under the localiser in force (mpmpc_rollout_set_localiser)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)h->cfg.max_batch, nb = (size_t)B;
  HIP_TRY(pull(sl.stream, fix, lc.fix, 3 * nb));
  HIP_TRY(pull(sl.stream, prior, lc.prior, 3 * nb));
  HIP_TRY(pull(sl.stream, cand, lc.out, nb));
  HIP_TRY(pull(sl.stream, score, lc.out + mb, nb));
  HIP_TRY(pull(sl.stream, hits, lc.out + 2 * mb, nb));
  HIP_TRY(pull(sl.stream, ranges, lc.ranges, nb * (size_t)lc.n_beams));
  HIP_TRY(pull(sl.stream, err2_max, lc.stats, nb));
  HIP_TRY(pull(sl.stream, err2_sum, lc.stats + mb, nb));
  HIP_TRY(pull(sl.stream, head2_sum, lc.stats + 2 * mb, nb));
  HIP_TRY(pull(sl.stream, prior2_sum, lc.stats + 3 * mb, nb));
  HIP_TRY(pull(sl.stream, steps, lc.count, nb));
  HIP_TRY(pull(sl.stream, matched, lc.count + mb, nb));
  HIP_TRY(pull(sl.stream, lost, lc.count + 2 * mb, nb));
  HIP_TRY(pull(sl.stream, edge, lc.count + 3 * mb, nb));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

}  // extern "C"
