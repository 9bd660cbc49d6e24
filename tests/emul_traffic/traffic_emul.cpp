// CPU twin of K0t (mpmpc_traffic_kernel): the same traffic_core.hpp code, one car after the other.
// Built by tests/emul/Makefile (`make traffic`), loaded by tests/twins.py.
#include <cstdint>
#include <vector>

#include "traffic_core.hpp"

using namespace mpmpc;

extern "C" {

// Validation of mpmpc_rollout_set_traffic (the library calls the same function): 0, -1 (E_ARG) or -3 (E_STATE).
// static_B / static_off, movers_B / movers_off: the other two settings in force (B = 0: off).
int tr_emu_check(int B, int max_batch, const int32_t* group, const int32_t* radius, int slots, int built, int static_B,
                 const int32_t* static_off, int movers_B, const int32_t* movers_off) {
  const char* why = "";
  return tr_check_traffic(B, max_batch, group, radius, slots, built != 0, static_B, static_off, movers_B, movers_off, &why);
}

// what the other two setters check against the traffic in force
int tr_emu_check_combined(int static_B, const int32_t* static_off, int movers_B, const int32_t* movers_off, int traffic_B,
                          int slots) {
  const char* why = "";
  return mov_check_combined(static_B, static_off, movers_B, movers_off, &why, traffic_B, slots);
}
int tr_emu_check_movers(int B, int max_batch, const int32_t* off, const int32_t* kind, const int32_t* radius,
                        const double* params, int built, int static_B, const int32_t* static_off, int traffic_B, int slots) {
  const char* why = "";
  return mov_check_movers(B, max_batch, off, kind, radius, params, built != 0, static_B, static_off, &why, traffic_B, slots);
}

// the groups as the library lays them out: dense [B], goff [B + 1], members [B]; returns the number of groups or -1
int tr_emu_layout(int B, const int32_t* group, int32_t* dense, int32_t* goff, int32_t* members) {
  return tr_layout(B, group, dense, goff, members);
}

// combined offsets [B + 1] and the movers' slots with `slots` traffic slots per car (0: no traffic)
void tr_emu_combine(int B, const int32_t* static_off, const int32_t* movers_off, int slots, int32_t* off, int32_t* dst) {
  mov_combine(B, static_off, movers_off, off, dst, slots);
}

// out [B][S][3]: the slots of every car for the state (pose, alive) a step finds; returns -1 when a group is too large
int tr_emu_slots(int B, const double* pose, const int32_t* alive, const int32_t* group, const int32_t* radius, int S,
                 int range_cells, int map_h, int map_w, double ox, double oy, double res, int32_t* out) {
  const MapView m{nullptr, map_h, map_w, ox, oy, res};
  std::vector<int32_t> dense((size_t)B), goff((size_t)B + 1), members((size_t)B);
  if (tr_layout(B, group, dense.data(), goff.data(), members.data()) < 0) return -1;
  for (int b = 0; b < B; ++b)
    tr_slots_car(m, pose, alive, dense.data(), radius, goff.data(), members.data(), S, range_cells, b, out + 3L * S * b);
  return 0;
}

}  // extern "C"
