// CPU twin of K0d and K3l (mpmpc_localiser.hpp): the same localiser_core.hpp code, one cell and one car at a time.
// Built by tests/emul_localiser/Makefile, loaded by tests/localiser_twin.py.
#include <cstdint>

#include "localiser_core.hpp"

using namespace mpmpc;

extern "C" {

// Validation of mpmpc_rollout_set_localiser (the library calls the same function): 0 or -1 (E_ARG); *why: the reason
int lc_emu_check(int n_beams, const double* angles, double range_m, double res, int D, int m, int W, int T, double step_psi, int min_hits,
                 double sigma_r, long long period, int B, const double* fix0, const char** why) {
  *why = "";
  return lc_check_setting(n_beams, angles, range_m, res, LcSet{D, m, W, T, min_hits, step_psi, sigma_r}, period, B, fix0, why);
}

// K0d: field [height][width]
void lc_emu_field(int height, int width, const int8_t* data, int D, uint8_t* field) {
  const MapView map{data, height, width, 0.0, 0.0, 1.0};
  for (int j = 0; j < height; ++j)
    for (int i = 0; i < width; ++i) field[(long)j * width + i] = (uint8_t)lc_field_cell(map, i, j, D);
}

// a look-up of the field, outside the grid too
int lc_emu_field_at(const uint8_t* field, int width, int height, int D, long long i, long long j) {
  return lc_field_at(field, width, height, lc_cap(D), i, j);
}

// the noisy ranges of car `car` (car0 already added) at j: hits (ranges[b] < range_m) in place, hit [n_beams] out
void lc_emu_noise(double sigma_r, uint64_t seed, uint32_t car, int64_t j, int n_beams, double range_m, double* ranges, unsigned char* hit) {
  for (int b = 0; b < n_beams; ++b) {
    hit[b] = ranges[b] < range_m ? 1 : 0;
    if (hit[b]) ranges[b] = lc_noisy(ranges[b], sigma_r, seed, car, j, b);
  }
}

// steps 3 (the hits) and 4 for B (prior, scan) pairs: mpmpc_scan_match.  hit may be NULL (ranges < range_m).  min_edge [B]
void lc_emu_match(int height, int width, const int8_t* data, const uint8_t* field, double ox, double oy, double res, int B, const double* prior,
                  const double* ranges, const unsigned char* hit, int n_beams, const double* angles, double range_m, int D, int m, int W, int T,
                  double step_psi, int min_hits, double* fix, int* score, int* cand, int* hits, double* min_edge) {
  const MapView map{data, height, width, ox, oy, res};
  const LcSet s{D, m, W, T, min_hits, step_psi, 0.0};
  for (long i = 0; i < B; ++i)
    hits[i] = lc_match(map, field, s, n_beams, angles, range_m, ranges + i * n_beams, hit ? hit + i * n_beams : nullptr, prior + 3 * i,
                       fix + 3 * i, cand + i, score + i, min_edge + i);
}

// K3l for one car (car0 already added).  st [4] = err2_max, err2_sum, head2_sum, prior2_sum; cnt [4] = steps, matched, lost, edge
void lc_emu_step(int height, int width, const int8_t* data, const uint8_t* field, double ox, double oy, double res, int D, int m, int W, int T,
                 double step_psi, int min_hits, double sigma_r, long long period, uint64_t seed, uint32_t car, int64_t j, double L, double Ts,
                 int n_beams, const double* angles, double range_m, double* ranges, const double* pose, const double* cmd, double* fix,
                 double* prior, int* primed, int* cand, int* score, int* hits, double* st, int* cnt) {
  const MapView map{data, height, width, ox, oy, res};
  lc_step(map, field, LcSet{D, m, W, T, min_hits, step_psi, sigma_r}, period, seed, car, j, L, Ts, n_beams, angles, range_m, ranges, pose, cmd,
          fix, prior, primed, cand, score, hits, st, cnt);
}

}  // extern "C"
