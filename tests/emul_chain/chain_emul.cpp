// CPU twin of the recorder's third kernel (mpmpc_record_chain_kernel): the same rollout_core.hpp code, one car and one entry
// after the other, into a chain laid out by ro_chain_layout.  Built by tests/emul_chain/Makefile, loaded by tests/chain_twin.py.
#include <cstdint>
#include <cstring>
#include <vector>

#include "rollout_core.hpp"

using namespace mpmpc;

extern "C" {

// out [18]: the 15 offsets in RoChainLayout's order (act, meas, queue, pred_pose, pred_s, now, est, cov, used, fix, prior, cand,
// score, hits, ranges; from the chain's start, -1: not recorded), bytes, entries, n_beams
void chain_emu_layout(int B, int fields, int n_beams, long long* out) {
  const RoChainLayout l = ro_chain_layout(B, fields, n_beams);
  const long long v[18] = {l.act, l.meas, l.queue, l.pred_pose, l.pred_s, l.now, l.est, l.cov, l.used, l.fix, l.prior, l.cand, l.score, l.hits,
                           l.ranges, l.bytes, l.entries, l.n_beams};
  std::memcpy(out, v, sizeof(v));
}

// The chain of one recorded step of B cars.  a_in [B]; the sources as the step leaves them, a group's first pointer NULL when
// its feature is not in force (act / queue / est / fix).  Outputs as mpmpc_rollout_trace_chain lays one record out ([B][...]);
// those of bits not selected are left alone (may be NULL).  The chain's memory starts as 0x5a bytes: an entry the code does not
// write shows.
int chain_emu_record(int B, int fields, int n_beams, const int32_t* a_in, const double* act, const double* meas, const double* queue,
                     const double* pred_pose, const double* pred_s, const double* now, const double* est, const double* cov,
                     const int32_t* used, const double* fix, const double* prior, const int32_t* cand, const int32_t* score,
                     const int32_t* hits, const double* ranges, double* o_act, double* o_meas, double* o_queue, double* o_pred_pose,
                     double* o_pred_s, double* o_now, double* o_est, double* o_cov, int32_t* o_used, double* o_fix, double* o_prior,
                     int32_t* o_cand, int32_t* o_score, int32_t* o_hits, double* o_ranges) {
  if (fields & ~RO_REC_EVERY) return -1;
  const RoChainLayout l = ro_chain_layout(B, fields, n_beams);
  std::vector<char> rec((size_t)l.bytes, (char)0x5a);
  const RoChainSrc src{a_in, act, meas, queue, pred_pose, pred_s, now, est, cov, used, fix, prior, cand, score, hits, ranges};
  for (int i = 0; i < B; ++i)
    for (int e = 0; e < l.entries; ++e) ro_record_chain(src, rec.data(), l, i, e);
  auto out = [&](void* dst, long long off, size_t per_car_bytes) {
    if (dst && off >= 0) std::memcpy(dst, rec.data() + off, per_car_bytes * (size_t)B);
  };
  out(o_act, l.act, 16); out(o_meas, l.meas, 24);
  out(o_queue, l.queue, 16 * (size_t)RO_CHAIN_QUEUE); out(o_pred_pose, l.pred_pose, 24); out(o_pred_s, l.pred_s, 8); out(o_now, l.now, 24);
  out(o_est, l.est, 24); out(o_cov, l.cov, 8 * (size_t)RO_CHAIN_COV); out(o_used, l.used, 4);
  out(o_fix, l.fix, 24); out(o_prior, l.prior, 24); out(o_cand, l.cand, 4); out(o_score, l.score, 4); out(o_hits, l.hits, 4);
  out(o_ranges, l.ranges, 8 * (size_t)l.n_beams);
  return 0;
}
}
