// The lane probe on the TWIN (csrc/lane_emu.hpp): the same primitives (probe.hpp), the same C entry point and array layout
// as probe.hip; one "block" is one emulated execution group of MPMPC_EMU_W lanes.  Built by tests/emul/Makefile with
// MPMPC_EMU_W = 64 (the wavefront backends and the pairs on them), 128 and 256 (the workgroup backends).
#include <cstddef>
#define MPMPC_TICK_BEGIN(i) ((void)0)
#define MPMPC_TICK_END(i) ((void)0)
#define MPMPC_TICK_COUNT(i) ((void)0)
#include "lane_emu.hpp"
#include "lane_pair.hpp"
#include "mpmpc_core.hpp"
#include "probe.hpp"

namespace lane_probe {

constexpr int SLOTS = 4;        // as on the device (probe.hip)

struct Call {
  int op, arg, blocks;
  const double* in;
  double* out;
  double* mem;
  int* imem;
};

template <class L, int KIND>
int run(const Call& c) {
  using R = typename L::real;
  constexpr int NX = KIND == PAIR ? K / 2 : K;
  bool known = true;
  for (int b = 0; b < c.blocks; ++b) {
    const double* in = c.in + (size_t)b * EMU_W * K;
    double* out = c.out + (size_t)b * EMU_W * K;
    R x[NX], y[NX];
    for (int k = 0; k < NX; ++k)
      for (int i = 0; i < EMU_W; ++i) {
        if constexpr (KIND == PAIR) { x[k].v[0].v[i] = in[i * K + k]; x[k].v[1].v[i] = in[i * K + NX + k]; }
        else x[k].v[i] = in[i * K + k];
      }
    known = run_op<L, KIND>(c.op, c.arg, x, y, c.mem, c.imem) && known;
    for (int k = 0; k < NX; ++k)
      for (int i = 0; i < EMU_W; ++i) {
        if constexpr (KIND == PAIR) { out[i * K + k] = y[k].v[0].v[i]; out[i * K + NX + k] = y[k].v[1].v[i]; }
        else out[i * K + k] = y[k].v[i];
      }
  }
  return known ? 0 : -2;
}

}  // namespace lane_probe

using namespace lane_probe;

extern "C" int lane_probe_op_count() { return N_OPS; }
extern "C" const char* lane_probe_op_name(int op) { return op_name(op); }
extern "C" int lane_probe_threads(int backend) {
  switch (backend) {
#if MPMPC_EMU_W == 64
    case G64C16: case G64C32: case G32C16: case G16C16: case G64C64: case P16: case P64: return 64;
#elif MPMPC_EMU_W == 128
    case B128: case B128CH128: case P128: return 128;
#else
    case B256: return 256;
#endif
    default: return 0;
  }
}
extern "C" int lane_probe_run(int backend, int op, int arg, int blocks, const double* in, double* out, double* mem, int mem_n,
                              int* imem, int imem_n) {
  if (blocks < 1 || blocks > 4 || op < 0 || op >= N_OPS || !in || !out || mem_n < 0 || imem_n < 0) return -1;
  const Call c{op, arg, blocks, in, out, mem, imem};
  switch (backend) {
#if MPMPC_EMU_W == 64
    case G64C16: return run<LaneEmu<64, 16, SLOTS>, WAVE>(c);
    case G64C32: return run<LaneEmu<64, 32, SLOTS>, WAVE>(c);
    case G32C16: return run<LaneEmu<32, 16, SLOTS>, WAVE>(c);
    case G16C16: return run<LaneEmu<16, 16, SLOTS>, WAVE>(c);
    case G64C64: return run<LaneEmu<64, 64, SLOTS>, WAVE>(c);
    case P16: return run<LanePair<LaneEmu<16, 16, SLOTS>>, PAIR>(c);
    case P64: return run<LanePair<LaneEmu<64, 64, SLOTS>>, PAIR>(c);
#elif MPMPC_EMU_W == 128
    case B128: return run<LaneEmu<128, 64, SLOTS>, BLOCK>(c);
    case B128CH128: return run<LaneEmu<128, 128, SLOTS>, BLOCK>(c);
    case P128: return run<LanePair<LaneEmu<128, 128, SLOTS>>, PAIR>(c);
#else
    case B256: return run<LaneEmu<256, 128, SLOTS>, BLOCK>(c);
#endif
    default: return -1;
  }
}
