// CPU twin of the route view (tests/test_routes.py): the library's own gather_stage / assemble_fields (mpmpc_assemble.hpp) on
// the emulated lanes - with a route header per instance on the concatenated tables, or without one on a route's own tables - and
// the corridor's horizon walk (corridor_core.hpp) through a route's PathGeom view.  Built by tests/emul/Makefile
// (`make routes`), loaded by tests/twins.py.
#include <cstdint>
#include <vector>

#include "lane_emu.hpp"
#include "lane_pair.hpp"
#include "mpmpc_assemble.hpp"
#include "corridor_core.hpp"
#include "rollout_core.hpp"

using namespace mpmpc;

// out [B][N + 1][MPMPC_NUM_FIELDS]: the fields of stage k of instance i, from assemble_fields on lanes that hold
// (instance, stage) pairs in batch order with `group` lanes per instance - group < EMU_W: an emulated wave holds several
// instances, of different routes.  route: [B][2] headers (PathTables::route) or null.  pair != 0: two stages per lane (LanePair).
extern "C" int routes_emu_fields(const mpmpc_config* cfg, int n_wp, const double* kappa, const double* v_ref, const double* ds_next,
                                 int n_cols, const double* ub_tab, const double* lb_tab, const int* route, int B, int group,
                                 int pair, const int* wp_id, const double* x0, const double* cc, double* out) {
  const int N = cfg->N;
  if (group < 1 || group > EMU_W || EMU_W % group != 0 || (pair ? 2 * group : group) < N + 1) return -1;
  PathTables t{kappa, v_ref, ds_next, n_wp, ub_tab, lb_tab, n_cols};
  t.route = route;
  auto keep = [&](int inst, int k, int f, double v) {
    if (inst < B && k >= 0 && k <= N) out[((size_t)inst * (N + 1) + k) * MPMPC_NUM_FIELDS + f] = v;
  };
  for (int t0 = 0; t0 < B * group; t0 += EMU_W) {
    if (!pair) {
      using L = LaneEmu<64>;
      VI inst, k;
      for (int i = 0; i < EMU_W; ++i) { inst.v[i] = (t0 + i) / group; k.v[i] = (t0 + i) % group; }
      VD f[MPMPC_NUM_FIELDS];
      assemble_fields<L>(*cfg, t, B, inst, k, wp_id, x0, cc, nullptr, nullptr, f);
      for (int i = 0; i < EMU_W; ++i)
        for (int j = 0; j < MPMPC_NUM_FIELDS; ++j) keep(inst.v[i], k.v[i], j, f[j].v[i]);
    } else {
      using L = LanePair<LaneEmu<16, 16>>;      // (only its value types are used here: the lanes are laid out below)
      I2 inst, k;
      for (int i = 0; i < EMU_W; ++i)
        for (int c = 0; c < 2; ++c) { inst.v[c].v[i] = (t0 + i) / group; k.v[c].v[i] = 2 * ((t0 + i) % group) + c; }
      D2 f[MPMPC_NUM_FIELDS];
      assemble_fields<L>(*cfg, t, B, inst, k, wp_id, x0, cc, nullptr, nullptr, f);
      for (int i = 0; i < EMU_W; ++i)
        for (int c = 0; c < 2; ++c)
          for (int j = 0; j < MPMPC_NUM_FIELDS; ++j) keep(inst.v[c].v[i], k.v[c].v[i], j, f[j].v[c].v[i]);
    }
  }
  return 0;
}

// the closed loop's waypoint arithmetic on a route's slice of cum (first row `first`, n waypoints)
extern "C" int routes_emu_current_waypoint(const double* cum, int first, int n, double s) { return ro_current_waypoint(cum + first, n, s); }
extern "C" int routes_emu_past_open_end(int n, int N, int circular, int wp) { return ro_past_open_end(n, N, circular != 0, wp) ? 1 : 0; }

// mpmpc_build_corridor with routes, on the host: the per-waypoint caches (segs / nseg / wpc) are indexed by GLOBAL row, every
// route walks its own rows of them and of the geometry through a PathGeom view (offset base pointers, its length, its circular
// flag) - cor_forced and cor_select as they are - and the table comes out concatenated.  -> start waypoints without a free
// segment, or -3001 (more than COR_MAXSEG free segments on a line)
extern "C" int routes_emu_corridor(int height, int width, const int8_t* data, double ox, double oy, double res, int n_wp,
                                   const double* x, const double* y, const double* psi, const double* ds_next, int P,
                                   const int* first, const int* circular, const double* bub, const double* blb, int n_cols,
                                   double min_width, double safety_margin, double* ub_tab, double* lb_tab) {
  const MapView mv{data, height, width, ox, oy, res};
  std::vector<double> trig((size_t)n_wp * COR_TRIG), segs((size_t)n_wp * 4 * COR_MAXSEG, 0.0), wpc((size_t)n_wp * COR_WPC, 0.0);
  std::vector<int> nseg((size_t)n_wp);
  for (int i = 0; i < n_wp; ++i) {
    cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
    nseg[i] = cor_free_segments(mv, bub[2 * i], bub[2 * i + 1], blb[2 * i], blb[2 * i + 1], min_width, segs.data() + (size_t)i * 4 * COR_MAXSEG);
    if (nseg[i] < 0) return -3001;
  }
  int bad = 0;
  for (int p = 0; p < P; ++p) {
    const size_t f = (size_t)first[p];
    const int n = first[p + 1] - first[p];
    const PathGeom g{x + f, y + f, psi + f, ds_next + f, n, circular[p], trig.data() + f * COR_TRIG};
    const double* sg = segs.data() + f * 4 * COR_MAXSEG;
    const int* ns = nseg.data() + f;
    double* wc = wpc.data() + f * COR_WPC;
    for (int i = 0; i < n; ++i)
      if (ns[i] <= 1) cor_forced(g, sg, ns, i, safety_margin, wc + (size_t)i * COR_WPC);
    for (int w = 0; w < n; ++w) {
      double *ub = ub_tab + (f + w) * n_cols, *lb = lb_tab + (f + w) * n_cols;
      if (!cor_select(g, sg, ns, w + 1, n_cols, safety_margin, ub, lb, wc)) {
        ++bad;
        for (int c = 0; c < n_cols; ++c) ub[c] = lb[c] = __builtin_nan("");
      }
    }
  }
  return bad;
}


// The handle's route state without a handle (route_state.hpp: the object TabState owns): the path's length and flag stand in for
// mpmpc_set_path / mpmpc_config, every call returns the code the library's entry point returns, *why its message.
#include "route_state.hpp"
struct RouteTwin {
  RouteState r;
  int n_wp = 0, N = 30, circular = 1, max_batch = 0;
  const char* why = "";
};
extern "C" RouteTwin* routes_state_new(int N, int circular, int max_batch) {
  RouteTwin* t = new RouteTwin();
  t->N = N; t->circular = circular; t->max_batch = max_batch;
  return t;
}
extern "C" void routes_state_free(RouteTwin* t) { delete t; }
extern "C" const char* routes_state_why(RouteTwin* t) { return t->why; }
extern "C" void routes_state_set_path(RouteTwin* t, int n_wp) { t->n_wp = n_wp; t->r.clear(); }      // (as mpmpc_set_path does)
extern "C" int routes_state_set_routes(RouteTwin* t, int P, const int32_t* first, const int32_t* circular, int* changed) {
  bool ch = false;
  const int rc = t->r.set_routes(t->n_wp, P, first, circular, &ch, &t->why);
  *changed = ch ? 1 : 0;
  return rc;
}
extern "C" int routes_state_set_car_routes(RouteTwin* t, int B, const int32_t* route, int32_t* hdr_out) {
  std::vector<int32_t> hdr;
  if (int rc = t->r.car_headers(t->max_batch, B, route, &hdr, &t->why)) return rc;
  for (size_t i = 0; i < hdr.size(); ++i) hdr_out[i] = hdr[i];
  t->r.keep_car_routes(B, route);
  return MPMPC_OK;
}
extern "C" int routes_state_check_upload(RouteTwin* t, int B, const int32_t* wp_id) {
  return t->r.check_wp_ids(B, wp_id, t->N, t->n_wp, t->circular != 0, &t->why);
}
extern "C" int routes_state_check_batch(RouteTwin* t, int B) { return t->r.check_batch(B, &t->why); }
