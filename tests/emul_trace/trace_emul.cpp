// CPU twin of the rollout's recorder (mpmpc_record_snapshot_kernel / mpmpc_record_write_kernel): the same
// rollout_core.hpp code, one car and one entry after the other, into a record laid out by ro_trace_layout.
// Built by tests/emul/Makefile (`make trace`), loaded by tests/twins.py.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rollout_core.hpp"

using namespace mpmpc;

extern "C" {

// bytes of one record of B cars / entries per car of the second launch
long long trace_emu_record_bytes(int N, int B, int fields) { return ro_trace_layout(N, B, fields).bytes; }
int trace_emu_entries(int N, int B, int fields) { return ro_trace_layout(N, B, fields).entries; }

// One recorded step of B cars.
//   before the step: s, pose [B x 3], alive_in          (what the first launch sees)
//   after the step:  alive, wp_id, status, counter, x0 [B x 3], u [B x 2], cc [B x 2N], z [B x (5N+3)]
//   tables:          gx, gy, gpsi [n_wp]; rows row_ub / row_lb with leading dimension row_ld - per_car: row b, else row wp_id
// Outputs as mpmpc_rollout_trace lays one record out ([B][...]); those of fields not selected are left alone (may be NULL).
int trace_emu_record(int N, int B, int fields, int n_wp, int circular, const double* s, const double* pose,
                     const int32_t* alive_in, const int32_t* alive, const int32_t* wp_id, const int32_t* status,
                     const int32_t* counter, const double* x0, const double* u, const double* cc, const double* z,
                     const double* gx, const double* gy, const double* gpsi, const double* row_ub, const double* row_lb,
                     long long row_ld, int per_car, double* o_s, double* o_pose, int32_t* o_wp_id, double* o_x0,
                     double* o_u, int32_t* o_status, int32_t* o_counter, int32_t* o_alive, double* o_plan, double* o_pred_x,
                     double* o_pred_y, double* o_ub, double* o_lb) {
  if (fields & ~RO_REC_ALL) return -1;
  const RoTraceLayout l = ro_trace_layout(N, B, fields);
  std::vector<char> rec((size_t)l.bytes, (char)0x5a);
  std::vector<int> a_in(B, 12345);
  std::vector<double> trig((size_t)n_wp * 2);
  for (int i = 0; i < n_wp; ++i) { trig[2 * i] = std::cos(gpsi[i]); trig[2 * i + 1] = std::sin(gpsi[i]); }
  for (int i = 0; i < B; ++i)
    for (int c = 0; c < RO_REC_BEGIN_ENTRIES; ++c) ro_record_begin(s, pose, alive_in, a_in.data(), rec.data(), l, i, c);
  const RoRecSrc src{alive, a_in.data(), wp_id, status, counter, x0, u, cc, z, gx, gy, trig.data(), row_ub, row_lb,
                     row_ld, per_car, 2, N, n_wp, circular};
  for (int i = 0; i < B; ++i)
    for (int e = 0; e < l.entries; ++e) ro_record_finish(src, rec.data(), l, i, e);
  auto out = [&](void* dst, long long off, size_t per_car_bytes) {
    if (dst && off >= 0) std::memcpy(dst, rec.data() + off, per_car_bytes * (size_t)B);
  };
  out(o_s, l.s, 8); out(o_pose, l.pose, 24); out(o_wp_id, l.wp_id, 4); out(o_x0, l.x0, 24); out(o_u, l.u, 16);
  out(o_status, l.status, 4); out(o_counter, l.counter, 4); out(o_alive, l.alive, 4);
  out(o_plan, l.plan, 16 * (size_t)N); out(o_pred_x, l.pred_x, 8 * (size_t)(N - 2)); out(o_pred_y, l.pred_y, 8 * (size_t)(N - 2));
  out(o_ub, l.ub, 8 * (size_t)N); out(o_lb, l.lb, 8 * (size_t)N);
  return 0;
}
}
