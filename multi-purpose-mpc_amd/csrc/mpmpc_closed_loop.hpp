// The closed loop of libmpmpc.so, part of the one translation unit mpmpc_hip.hip (included there behind mpmpc_set_corridor):
// the kernels K0a / K0b (corridor tables from the map), K0c (per-car corridor rows), K0m (movers), K0h (the movers over the
// horizon), K0t / K0ht / K3t (traffic, its horizon, the plan tracks), K3a / K3b (localise, advance) and the two recorder kernels
// K3r, and the entry points that set a rollout up and read it back - mpmpc_set_map, mpmpc_set_path_geometry,
// mpmpc_build_corridor and every mpmpc_rollout_* but the step.  mpmpc_rollout_step itself - its plan, one enqueue function per
// kernel, the loop - is mpmpc_rollout_step.hpp, behind the features a step drives (mpmpc_plant.hpp in front of this header,
// mpmpc_lookahead.hpp, mpmpc_perception.hpp and mpmpc_footprint.hpp behind it).  The state they work on: the sub-states cor,
// obs, ro, rec of the handle (mpmpc_handle.hpp).  The walls of a car's world (mpmpc_rollout_set_walls, below) are rasterised by
// K0w (mpmpc_walls.hpp, in front of this header).
#pragma once

// K0a: free segments of every waypoint's border line, one WAVEFRONT per waypoint.  Lane 0 walks Zingl's anti-aliased
// line (a float32 recurrence in skimage's exact cell order: inherently serial, ~95 cells on Sim_Track) and leaves the
// cells in LDS; all 64 lanes then fetch the occupancies (one memory round trip for the whole line instead of one per
// cell; cells outside the grid count as occupied); lane 0 runs the run-length state machine over the LDS copy and, for
// a waypoint with at most one free segment, computes its bounds once (cor_forced) instead of once per start waypoint
// and column in K0b.  A line longer than COR_CELL_CAP cells or with more than COR_MAXSEG free segments raises *err
// (1 / 2) - mpmpc_build_corridor then fails instead of working with a truncated list.
__global__ __launch_bounds__(64) void mpmpc_free_segments_kernel(MapView map, PathGeom g, const double* __restrict__ bub,
                                                                 const double* __restrict__ blb, double min_width,
                                                                 double safety_margin, double* __restrict__ segs,
                                                                 int* __restrict__ nseg, double* __restrict__ wpc,
                                                                 int* __restrict__ err, int* __restrict__ line_cells,
                                                                 int* __restrict__ line_box) {
  __shared__ int cells[COR_CELL_CAP];
  __shared__ unsigned char occ[COR_CELL_CAP];
  __shared__ int s_n;
  __shared__ double seg[4 * COR_MAXSEG];      // lane 0's segment list (in LDS: a per-lane array would live in scratch)
  const int i = blockIdx.x, lane = threadIdx.x;
  int ux, uy, lx, ly;
  cor_w2m(map, bub[2 * i], bub[2 * i + 1], ux, uy);
  cor_w2m(map, blb[2 * i], blb[2 * i + 1], lx, ly);
  if (lane == 0) s_n = cor_line_cells(ux, uy, lx, ly, cells, COR_CELL_CAP);
  __syncthreads();
  const int n = s_n;
  int cnt;
  if (n > COR_CELL_CAP) {
    cnt = COR_E_CELLS;
  } else {
    for (int k = lane; k < n; k += 64) {
      int x, y;
      cor_unpack_cell(cells[k], x, y);
      occ[k] = cor_cell_free(map, x, y) ? 1 : 0;
      line_cells[(long)i * COR_CELL_CAP + k] = cells[k];      // K0c's cache of the line
    }
    __syncthreads();
    if (lane != 0) return;
    cor_line_box(cells, n, (ux + 1) | ((uy + 1) << 16), (lx + 1) | ((ly + 1) << 16), line_box + (long)i * COR_LINE_BOX);
    cnt = cor_scan_cells(map, ux, uy, lx, ly, min_width, n, [&](int c, int& x, int& y) { cor_unpack_cell(cells[c], x, y); },
                         [&](int c) { return occ[c] != 0; }, seg);
    for (int k = 0; k < 4 * COR_MAXSEG; ++k) segs[(long)i * 4 * COR_MAXSEG + k] = (cnt > 0 && k < 4 * cnt) ? seg[k] : 0.0;
  }
  if (lane != 0) return;
  if (cnt < 0) { atomicMax(err, cnt == COR_E_CELLS ? 1 : 2); cnt = 0; }
  nseg[i] = cnt;
  if (cnt <= 1) cor_forced(g, segs, nseg, i, safety_margin, wpc + (long)i * COR_WPC);
}

// K0b: horizon walk for every start waypoint w (table row w = update_path_constraints(w + 1, ...)).
// K0b: one thread per (start waypoint, column): cor_select_one replays only the short run of multi-segment waypoints
// right before its column, everything else is a row of K0a's per-waypoint table.
__global__ __launch_bounds__(256) void mpmpc_corridor_select_kernel(PathGeom g, const double* __restrict__ segs,
                                                                    const int* __restrict__ nseg, int n_cols,
                                                                    double safety_margin, double* __restrict__ ub_tab,
                                                                    double* __restrict__ lb_tab, int* __restrict__ bad,
                                                                    const double* __restrict__ wpc) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int w = t / n_cols, n = t - w * n_cols;
  if (w >= g.n_wp) return;
  double ub, lb;
  if (!cor_select_one(g, segs, nseg, w + 1, n, safety_margin, wpc, &ub, &lb)) {
    ub = lb = __builtin_nan("");
    if (n == 0) atomicAdd(bad, 1);
  }
  ub_tab[(long)w * n_cols + n] = ub;
  lb_tab[(long)w * n_cols + n] = lb;
}

// K0c: the corridor rows of one rollout step when every car carries its own obstacle discs (mpmpc_rollout_set_obstacles).
// One wavefront per car; lanes loop over the car's N columns (N up to 255).  Column n reads waypoint
// cor_wp(wp_id + 1 + n): if none of the car's discs meets the box of that waypoint's cached border line, it keeps the
// base segments of the last build (nseg / wpc / segs).  The others ("touched") are rescanned in the car's world: the
// wave stages the cached cells of as many touched lines as fit COR_CELL_CAP cells in LDS together with their occupancy
// (base map and discs, every lane fetching cells of its own - one memory round trip per batch of lines instead of one
// per cell), then the lane of each staged column runs the state machine over its cells in LDS (cor_scan_runs) and keeps
// the segment end cells as packed pairs plus the cor_forced row.  After a barrier every lane selects its columns as
// K0b does (cor_select_car_one) and writes lb / ub into the per-instance rows the solve reads.  flag[b] = COR_ROW_*: a
// car still running whose row is blocked / overflowing ends with alive = -3 / -4 (and gets a zero row, so that the
// solve of a stopped car stays an ordinary QP).  Every car gets its row - the solve runs on stopped cars too, and their
// status then matches the shared-table rollout's.
// LDS: 5 KB of staged cells + 0.8 KB of discs + N * (COR_WPC doubles + (2 COR_MAXSEG + 3) ints) = 5.9 KB + 124 B per column
// (+ 384 B of wall headers in the WALLS variant).
// WALLS (mpmpc_rollout_set_walls): the car's wall headers are staged in LDS next to its discs (at most COR_MAX_WALLS x
// WALL_HDR ints = 384 B, behind the staged cells), "touched" also means a wall's box meets the line box, and the staged
// occupancy is !base_free || in a disc || on a wall (wall_core.hpp; one table load per wall whose box holds the cell, through
// L2).  In that variant off may be nullptr (walls only: no discs).  Nothing else differs; without walls the kernel is the
// instantiation <false, false>, the code it always was.
// LEAD (mpmpc_rollout_set_lookahead with movers in the fleet; the law: lookahead_core.hpp): the disc accessor depends on the
// column - for a mover slot whose disc of step k has r > 0 it returns K0h's table entry of (slot, column), else the staged
// entry as without LEAD (look_col_disc) - in the touched test (lane = column) and in the staged occupancy of a column's cells.
// Nothing else differs; <., false> takes an empty LookNone and is instruction for instruction what it was.
// TRAF (mpmpc_rollout_set_lookahead_traffic active; the law: traffic_lookahead_core.hpp): the accessor of the LEAD variant gets a
// second per-column source - for one of the car's last S slots, its traffic slots, whose entry of the list K0c plans from has
// r > 0 it returns K0ht's table entry of (slot, column) (tlk_col_disc) - in the same two places.  A third template parameter
// rather than a null view: the instantiations <., false, false> and the mover-only <., true, false> keep their instructions.
struct LookNone {};
struct LookView {
  const int* car;      // [B + 1][2]: first mover of the car in the fleet's list, first mover slot in the car's own list
  const int* tab;      // [movers][N][3]: K0h's horizon discs (read through L2: staging a car's rows in LDS bought nothing)
};
struct LookTrafficView {
  const int* car;      // as LookView's
  const int* tab;
  const int* tz;       // [B][S][N][3]: K0ht's horizon discs of the cars' traffic slots (through L2, like tab)
  int S;               // traffic slots per car
};
// KEEP (mpmpc_rollout_set_commitment; the law: commitment_core.hpp): the car's memory of the step before - the waypoints of its N
// entries staged in LDS behind everything else (N ints), the entries' rows read from memory where a column has one - decides
// multi-segment columns by rule 1 (cmt_select_car_one in place of cor_select_car_one), and every lane writes the entries of its
// columns into the OTHER buffer of the memory (the host swaps the two per step: no lane reads what another writes) and counts
// kept / switched / moved, reduced over the wave and added to the car's counters by lane 0.  A fourth template parameter and an
// empty view otherwise (KeepNone / KeepView: mpmpc_commitment.hpp): the instantiations <., ., ., false> keep their instructions.
template <bool WALLS, bool LEAD = false, bool TRAF = false, bool KEEP = false>
__global__ __launch_bounds__(64) void mpmpc_car_corridor_kernel(MapView map, PathGeom g, int N, double min_width,
                                                                double safety_margin, const double* __restrict__ segs,
                                                                const int* __restrict__ nseg, const double* __restrict__ wpc,
                                                                const int* __restrict__ line_cells,
                                                                const int* __restrict__ line_box,
                                                                const int* __restrict__ off, const int* __restrict__ discs,
                                                                const int* __restrict__ wp_id, int* __restrict__ alive,
                                                                int* __restrict__ flag, double* __restrict__ lb,
                                                                double* __restrict__ ub, WallView wv,
                                                                const int* __restrict__ route,
                                                                std::conditional_t<TRAF, LookTrafficView, std::conditional_t<LEAD, LookView, LookNone>> lk,
                                                                std::conditional_t<KEEP, KeepView, KeepNone> km) {
  static_assert(LEAD || !TRAF, "the traffic horizon needs the leads");
  static_assert(!KEEP || !LEAD, "commitment under a lookahead is not supported");
  constexpr int PENDING = -1000000;
  // Route fleets: the car's view of the path - the geometry's base pointers and K0a's caches (indexed by GLOBAL row) moved to the
  // first row of its route, n_wp and circular the route's (route_view: corridor_core.hpp); wp_id is local.
  // Everything below, and corridor_core.hpp, works on the view.  (uniform per block; null: one path, nothing moves)
  if (route) {
    const RouteView v = route_header(route, blockIdx.x);
    const long f = v.first;
    g = route_geom(g, v);
    segs += f * 4 * COR_MAXSEG; nseg += f; wpc += f * COR_WPC; line_cells += f * COR_CELL_CAP; line_box += f * COR_LINE_BOX;
  }
  extern __shared__ double lds[];
  double* col_o = lds;                                             // [N][COR_WPC]
  int* col_seg = (int*)(col_o + (long)N * COR_WPC);                // [N][2 * COR_MAXSEG] packed end cells
  int* col_cnt = col_seg + (long)N * 2 * COR_MAXSEG;               // [N]; < 0: COR_E_SEGMENTS; +1000: touched
  int* col_aux = col_cnt + N;                                      // [N] touched: cells of the line
  int* col_off = col_aux + N;                                      // [N] touched and staged: offset in stg_*, else -1
  int* dsc = col_off + N;                                          // [COR_MAX_DISCS][3]
  int* stg_cell = dsc + 3 * COR_MAX_DISCS;                         // [COR_CELL_CAP]
  unsigned char* stg_free = (unsigned char*)(stg_cell + COR_CELL_CAP);   // [COR_CELL_CAP]
  __shared__ int s_over;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int d0 = WALLS && !off ? 0 : off[b], nd = WALLS && !off ? 0 : off[b + 1] - d0;
  for (int k = lane; k < 3 * nd; k += 64) dsc[k] = discs[3L * d0 + k];
  int* whd = (int*)(stg_free + COR_CELL_CAP);                        // [COR_MAX_WALLS][WALL_HDR] (WALLS only)
  int nw = 0;
  if (WALLS && wv.off) {
    const int w0 = wv.off[b];
    nw = wv.off[b + 1] - w0;
    nw = nw > COR_MAX_WALLS ? COR_MAX_WALLS : nw;                    // (the host refuses more)
    for (int k = lane; k < WALL_HDR * nw; k += 64) whd[k] = wv.hdr[(long)WALL_HDR * w0 + k];
  }
  int ns = 0, nm = 0;               // LEAD: the car's mover slots ns .. ns + nm - 1 and their rows of K0h's table
  const int* hz = nullptr;
  if constexpr (LEAD) {
    const int m0 = lk.car[2 * b];
    ns = lk.car[2 * b + 1];
    nm = lk.car[2 * b + 2] - m0;
    hz = lk.tab + (long)m0 * N * 3;
  }
  int ts = 0;                       // TRAF: the car's traffic slots nd - ts .. nd - 1 and its rows of K0ht's table
  const int* tzb = nullptr;
  if constexpr (TRAF) {
    ts = lk.S < nd ? lk.S : nd;     // (the layout gives every car S slots)
    tzb = lk.tz + (long)b * lk.S * N * 3;
  }
  int* mwp = whd + (WALLS ? WALL_HDR * COR_MAX_WALLS : 0);           // [N] the waypoints of the car's memory (KEEP only)
  if constexpr (KEEP)
    for (int k = lane; k < N; k += 64) mwp[k] = km.wp_old[(long)b * N + k];
  if (lane == 0) s_over = 0;
  __syncthreads();
  const int wp = wp_id[b] + 1;
  auto disc = [&](int j) { return (const int*)(dsc + 3 * j); };
  auto whdr = [&](int j) { return (const int*)(whd + WALL_HDR * j); };
  // the disc accessor `d` of column c - the one choice between the three sources - and what is returned with it (a macro, not a
  // function that returns the closure: every such form moved the LEAD instantiations, docs/HISTORY.md)
#define K0C_WITH_COL_DISC(c, EXPR)                                                                                  \
  if constexpr (TRAF) {                                                                                             \
    auto d = [&](int j) { return tlk_col_disc(dsc, j, ns, nm, hz, nd, ts, tzb, N, c); };                            \
    return EXPR;                                                                                                    \
  } else if constexpr (LEAD) {                                                                                      \
    auto d = [&](int j) { return look_col_disc(dsc, j, ns, nm, hz, N, c); };                                        \
    return EXPR;                                                                                                    \
  } else {                                                                                                          \
    auto& d = disc;                                                                                                 \
    return EXPR;                                                                                                    \
  }
  auto touches = [&](const int* box, int c) {
    K0C_WITH_COL_DISC(c, WALLS ? wall_car_touches(box, nd, d, nw, whdr) : (nd > 0 && cor_car_touches(box, nd, d)))
  };
  auto cell_free = [&](int cell, int c) {
    K0C_WITH_COL_DISC(c, WALLS ? wall_car_cell_free(map, cell, nd, d, nw, whdr, wv.tab) : cor_car_cell_free(map, cell, nd, d))
  };
#undef K0C_WITH_COL_DISC
  for (int n = lane; n < N; n += 64) {
    const int i = cor_wp(g, wp + n);
    const int* box = line_box + (long)i * COR_LINE_BOX;
    col_off[n] = -1;
    if (touches(box, n)) {
      col_cnt[n] = PENDING;
      col_aux[n] = box[0];
    } else {
      const int cnt = nseg[i];
      if (cnt <= 1)
        for (int k = 0; k < COR_WPC; ++k) col_o[(long)n * COR_WPC + k] = wpc[(long)i * COR_WPC + k];
      col_cnt[n] = cnt;
    }
  }
  __syncthreads();
  for (int n = 0; n < N;) {            // (uniform: every lane reads the same LDS words)
    int used = 0, e = n;
    for (; e < N; ++e) {
      if (col_cnt[e] != PENDING) continue;
      const int nc = col_aux[e];
      if (used > 0 && used + nc > COR_CELL_CAP) break;
      used += nc;
    }
    used = 0;
    for (int c = n; c < e; ++c) {
      if (col_cnt[c] != PENDING) continue;
      const int nc = col_aux[c];
      if (lane == 0) col_off[c] = used;
      const int* cells = line_cells + (long)cor_wp(g, wp + c) * COR_CELL_CAP;
      for (int k = lane; k < nc; k += 64) {
        const int cell = cells[k];
        stg_cell[used + k] = cell;
        stg_free[used + k] = cell_free(cell, c) ? 1 : 0;
      }
      used += nc;
    }
    __syncthreads();
    for (int c = n + lane; c < e; c += 64) {      // the lane of column c scans it
      const int o0 = col_off[c];
      if (o0 < 0) continue;
      const int nc = col_aux[c];
      const int i = cor_wp(g, wp + c);
      const int* box = line_box + (long)i * COR_LINE_BOX;
      int ux, uy, lx, ly;
      cor_unpack_cell(box[5], ux, uy);
      cor_unpack_cell(box[6], lx, ly);
      int* cs = col_seg + (long)c * 2 * COR_MAXSEG;
      double s0[4] = {0, 0, 0, 0};
      const int cnt = cor_scan_runs(map, ux, uy, lx, ly, min_width, nc,
                                    [&](int k, int& x, int& y) { cor_unpack_cell(stg_cell[o0 + k], x, y); },
                                    [&](int k) { return stg_free[o0 + k] != 0; },
                                    [&](int q, int sx, int sy, int x, int y, double ax, double ay, double bx, double by) {
                                      cs[2 * q] = (sx + 1) | ((sy + 1) << 16);
                                      cs[2 * q + 1] = (x + 1) | ((y + 1) << 16);
                                      if (q == 0) { s0[0] = ax; s0[1] = ay; s0[2] = bx; s0[3] = by; }
                                    });
      if (cnt < 0) s_over = 1;
      else if (cnt <= 1) cor_forced_seg(g, i, cnt, s0, safety_margin, col_o + (long)c * COR_WPC);
      col_cnt[c] = cnt < 0 ? cnt : cnt + 1000;
    }
    __syncthreads();
    n = e;
  }
  auto cnt = [&](int c) { const int v = col_cnt[c]; return v >= 1000 ? v - 1000 : v; };
  auto forced = [&](int c, double* o) { for (int k = 0; k < COR_WPC; ++k) o[k] = col_o[(long)c * COR_WPC + k]; };
  auto seg = [&](int c, int k, double* s) {
    if (col_cnt[c] >= 1000) {
      const int* cs = col_seg + (long)c * 2 * COR_MAXSEG;
      int x, y;
      cor_unpack_cell(cs[2 * k], x, y);
      cor_m2w(map, x, y, s[0], s[1]);
      cor_unpack_cell(cs[2 * k + 1], x, y);
      cor_m2w(map, x, y, s[2], s[3]);
    } else {
      const double* sg = segs + (long)cor_wp(g, wp + c) * 4 * COR_MAXSEG + 4 * k;
      for (int j = 0; j < 4; ++j) s[j] = sg[j];
    }
  };
  const int verdict = cnt(0) == 0 ? COR_ROW_BLOCKED : (s_over ? COR_ROW_OVERFLOW : COR_ROW_OK);   // the reference raises at column 0 first
  if constexpr (KEEP) {
    const double keep = km.keep[b];
    const double* mrow = km.rows_old + (long)b * N * COR_WPC;
    auto mem_wp = [&](int c) { return mwp[c]; };
    auto mem = [&](int i, double* m) {
      const int c = cmt_find(N, mem_wp, i);
      if (c < 0) return false;
      for (int k = 0; k < COR_WPC; ++k) m[k] = mrow[(long)c * COR_WPC + k];
      return true;
    };
    int n_kept = 0, n_switched = 0, n_moved = 0;
    for (int n = lane; n < N; n += 64) {
      double o[COR_WPC] = {0, 0, 0, 0, 0, 0};
      int how = 0;
      if (verdict == COR_ROW_OK) cmt_select_car_one(g, wp, n, safety_margin, keep, cnt, forced, seg, mem, o, &how);
      ub[(long)b * N + n] = o[0];
      lb[(long)b * N + n] = o[1];
      const int i = cor_wp(g, wp + n);
      const bool held = verdict == COR_ROW_OK && cnt(n) >= 1;      // the entry of column n (else: empty)
      km.wp_new[(long)b * N + n] = held ? i : CMT_EMPTY;
      for (int k = 0; k < COR_WPC; ++k) km.rows_new[((long)b * N + n) * COR_WPC + k] = held ? o[k] : 0.0;
      n_kept += how & CMT_KEPT ? 1 : 0;
      n_switched += how & CMT_SWITCHED ? 1 : 0;
      const int c = cmt_find(N, mem_wp, i);
      if (c >= 0 && cmt_moved(o[0], o[1], mrow[(long)c * COR_WPC], mrow[(long)c * COR_WPC + 1])) ++n_moved;
    }
    for (int d = 32; d > 0; d >>= 1) {
      n_kept += __shfl_down(n_kept, d);
      n_switched += __shfl_down(n_switched, d);
      n_moved += __shfl_down(n_moved, d);
    }
    if (lane == 0) {
      km.counts[b] += n_kept;
      km.counts[km.stride + b] += n_switched;
      km.counts[2 * km.stride + b] += n_moved;
    }
  } else {
    for (int n = lane; n < N; n += 64) {
      double u = 0.0, l = 0.0;
      if (verdict == COR_ROW_OK) cor_select_car_one(g, wp, n, safety_margin, cnt, forced, seg, &u, &l);
      ub[(long)b * N + n] = u;
      lb[(long)b * N + n] = l;
    }
  }
  if (lane == 0) {
    flag[b] = verdict;
    if (verdict != COR_ROW_OK && alive[b] == 1) alive[b] = verdict == COR_ROW_BLOCKED ? -3 : -4;
  }
}

// K0m: the movers of one rollout step (mpmpc_rollout_set_movers), launched between K3a and K0c when there are any.  One
// thread per mover of the whole fleet; its parameters are structure-of-arrays ([n] each: a wavefront loads consecutive
// words), its disc of step k (mov_disc: closed form in k; kind 1 searches ro_cum, ~9 probes that stay in L2) goes into
// its slot of its car's disc list - dst[j], laid out on the host when either setting changes - where K0c reads it
// behind the car's static discs.
__global__ __launch_bounds__(256) void mpmpc_obstacle_move_kernel(int n, long long k, long long step0, MapView map,
                                                                  MoverPath path, const int* __restrict__ kind,
                                                                  const int* __restrict__ radius,
                                                                  const double* __restrict__ prm,
                                                                  const int* __restrict__ dst, int* __restrict__ discs,
                                                                  const int* __restrict__ off, int B,
                                                                  const int* __restrict__ route) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  if (route) {      // route fleets: an along-the-path mover follows the route of the car that owns its slot (off: the cars' CSR offsets)
    int lo = 0, hi = B;      // the car b with off[b] <= dst[j] < off[b + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) / 2;
      if (off[mid] <= dst[j]) lo = mid; else hi = mid;
    }
    path = route_path(path, route_header(route, lo));
  }
  int d[3];
  mov_disc(map, path, kind[j], radius[j], prm[j], prm[(long)n + j], prm[2L * n + j], prm[3L * n + j], k, step0, d);
  int* o = discs + 3L * dst[j];
  o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
}

// K0h: the movers' discs over every car's horizon (mpmpc_rollout_set_lookahead; the law: lookahead_core.hpp), launched behind
// K3a - it reads wp_id - when lookahead is set and the fleet has movers.  One 64-lane block per car: the lanes fetch the car's
// N seg_time entries side by side, lane 0 runs the N dependent adds of the lead law over them in LDS (no scan: the rounding
// order is the law's), then the lanes stride over the car's (mover, column) pairs, each one mov_disc at step k + lead_c on the
// route view of the car as K0m forms it.  lead [B][N], tab [movers][N][3]: what the LEAD instantiations of K0c read.
// LDS: 3 KB; no scratch; no device-libm result in any cell (mov_centre's trigonometry is K0's host table).
__global__ __launch_bounds__(64) void mpmpc_mover_horizon_kernel(int N, long long k, long long step0, double Ts, int max_lead,
                                                                 MapView map, PathGeom g, MoverPath path,
                                                                 const double* __restrict__ seg_time,
                                                                 const int* __restrict__ wp_id, int n,
                                                                 const int* __restrict__ kind, const int* __restrict__ radius,
                                                                 const double* __restrict__ prm, const int* __restrict__ car,
                                                                 int* __restrict__ lead, int* __restrict__ tab,
                                                                 const int* __restrict__ route) {
  __shared__ double s_seg[256];      // (N <= 255)
  __shared__ int s_lead[256];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (route) {      // route fleets: the car's view of the path, of seg_time and of what an along-the-path mover follows
    // (written out, not route_view / route_path: every form of them moved this kernel's registers - docs/HISTORY.md)
    const long f = route[2 * b];
    const int nn = route[2 * b + 1];
    g.n_wp = nn > 0 ? nn : -nn;
    g.circular = nn > 0 ? 1 : 0;
    seg_time += f;
    path = MoverPath{path.cum + f, path.x + f, path.y + f, path.trig + f * path.trig_ld, g.n_wp, path.trig_ld, g.circular};
  }
  const int wp = wp_id[b];
  for (int c = lane; c < N; c += 64) s_seg[c] = seg_time[look_seg_row(g, wp, c)];
  __syncthreads();
  if (lane == 0) look_leads(N, Ts, max_lead, [&](int c) { return s_seg[c]; }, s_lead);
  __syncthreads();
  for (int c = lane; c < N; c += 64) lead[(long)b * N + c] = s_lead[c];
  const int m0 = car[2 * b], pairs = (car[2 * b + 2] - m0) * N;
  for (int p = lane; p < pairs; p += 64) {
    const int q = p / N, c = p - q * N;
    const long j = m0 + q;
    int d[3];
    mov_disc(map, path, kind[j], radius[j], prm[j], prm[(long)n + j], prm[2L * n + j], prm[3L * n + j], k + s_lead[c], step0, d);
    int* o = tab + (j * N + c) * 3;
    o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
  }
}

// K0t: the traffic of one rollout step (mpmpc_rollout_set_traffic; the law: traffic_core.hpp), launched in front of K3a -
// it reads pose and alive as the step finds them - when traffic is set.  One WAVEFRONT per car b; the lanes take the
// members of b's group strided by 64 (the host laid the groups out as a CSR list in ascending car index: tr_layout), each
// computes its members' cells and stages their keys in LDS: d2 as b sees the member, or -1 when it is no candidate; the
// position in the list breaks ties, as the car index would.  Then S rounds of "smallest (d2, position) above the last one
// taken": every lane scans the keys it staged, a 64-lane butterfly takes the minimum of the pairs (unique, so every lane
// ends with the same winner), lane t keeps the disc of round t.  The rounds end early when no candidate is left.  At the
// end lanes 0 .. S-1 store the car's S slots - the last S entries of its disc list, where K0c reads them behind the
// static discs and the movers.  LDS: 16 KB (TR_MAX_GROUP keys and cells); no scratch; trip counts depend on the group's
// size and S only.
// WHO (mpmpc_rollout_set_lookahead_traffic active): lane t also keeps the car index of slot t's occupant and stores it in
// who[b][t], -1 for an empty slot - what K0ht reads.  <false> takes an empty LookNone and is the code the kernel always was.
template <bool WHO = false>
__global__ __launch_bounds__(64) void mpmpc_traffic_kernel(int B, int S, int range_cells, MapView map,
                                                           const double* __restrict__ pose, const int* __restrict__ alive,
                                                           const int* __restrict__ dense, const int* __restrict__ radius,
                                                           const int* __restrict__ members, const int* __restrict__ goff,
                                                           const int* __restrict__ off, int* __restrict__ discs,
                                                           std::conditional_t<WHO, int*, LookNone> who) {
  __shared__ long long key[TR_MAX_GROUP];
  __shared__ int cell_x[TR_MAX_GROUP], cell_y[TR_MAX_GROUP];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  int d[3] = {0, 0, 0};                     // lane t: slot t
  [[maybe_unused]] int occupant = -1;       // (WHO) lane t: the car in slot t
  const int g = dense[b];
  int bx = 0, by = 0;
  if (alive[b] == 1 && g >= 0 && tr_cell(map, pose[3L * b], pose[3L * b + 1], &bx, &by)) {      // (uniform)
    const int g0 = goff[g];
    int n = goff[g + 1] - g0;
    n = n > TR_MAX_GROUP ? TR_MAX_GROUP : n;      // (the host refuses larger groups)
    for (int p = lane; p < n; p += 64) {
      const int c = members[g0 + p];
      int cx = 0, cy = 0;
      long long d2 = -1;
      if (c != b && alive[c] == 1 && tr_cell(map, pose[3L * c], pose[3L * c + 1], &cx, &cy) && tr_visible(map, cx, cy, radius[c]))
        d2 = tr_d2(bx, by, cx, cy, range_cells);
      key[p] = d2;
      cell_x[p] = cx;
      cell_y[p] = cy;
    }
    __syncthreads();
    long long last_d2 = -1;
    int last_p = -1;
    for (int t = 0; t < S; ++t) {
      long long best = 0x7fffffffffffffffLL;
      int best_p = 0x7fffffff;
      for (int p = lane; p < n; p += 64) {
        const long long k = key[p];
        if (k >= 0 && tr_less(last_d2, last_p, k, p) && tr_less(k, p, best, best_p)) { best = k; best_p = p; }
      }
      for (int m = 32; m >= 1; m >>= 1) {
        const int lo = __shfl_xor((int)(unsigned)(best & 0xffffffffLL), m, 64), hi = __shfl_xor((int)(best >> 32), m, 64);
        const int op = __shfl_xor(best_p, m, 64);
        const long long o = ((long long)hi << 32) | (unsigned)lo;
        if (tr_less(o, op, best, best_p)) { best = o; best_p = op; }
      }
      if (best_p == 0x7fffffff) break;          // (uniform) no candidate left
      if (lane == t) { d[0] = cell_x[best_p]; d[1] = cell_y[best_p]; d[2] = radius[members[g0 + best_p]]; }
      if constexpr (WHO) {
        if (lane == t) occupant = members[g0 + best_p];
      }
      last_d2 = best;
      last_p = best_p;
    }
  }
  if (lane < S) {
    int* o = discs + 3L * (off[b + 1] - S + lane);
    o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
    if constexpr (WHO) who[(long)b * S + lane] = occupant;
  }
}

// K0ht: the cars' traffic slots over their horizons (mpmpc_rollout_set_lookahead_traffic; the law: traffic_lookahead_core.hpp),
// launched behind K0h - it reads the leads of the step - and in front of K0c.  One 64-lane block per car b; the lanes stride over
// the car's S x N (slot, column) pairs, each one tlk_disc: the slot's disc of step k from the TRUE list, its occupant from
// K0t's who, and - where the column has a lead and the occupant a valid track - a binary search of at most 8 probes in the
// occupant's tm (through L2) for the stage its plan has reached by then.  tz [B][S][N][3].  No LDS, no scratch.
__global__ __launch_bounds__(64) void mpmpc_traffic_horizon_kernel(int N, int S, double Ts, MapView map,
                                                                   const int* __restrict__ off, const int* __restrict__ discs,
                                                                   const int* __restrict__ who, const int* __restrict__ lead,
                                                                   const int* __restrict__ valid, const int* __restrict__ cells,
                                                                   const double* __restrict__ tm, int* __restrict__ tz) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int* slots = discs + 3L * (off[b + 1] - S);
  for (int p = lane; p < S * N; p += 64) {
    const int t = p / N, c = p - t * N;
    int d[3];
    tlk_disc(map, slots + 3 * t, who[(long)b * S + t], lead[(long)b * N + c], Ts, N, valid, cells, tm, d);
    int* o = tz + ((long)b * S * N + p) * 3;
    o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
  }
}

// K3t: the plan tracks a step leaves (mpmpc_rollout_set_lookahead_traffic; the law: traffic_lookahead_core.hpp), launched behind
// K3b while the setting is active.  One WAVEFRONT per car n; the lanes take the N + 1 <= 256 stages of its plan in up to four
// chunks of 64: lane j's cell from z's e_y at the stage's waypoint (K0's host trig table: no device libm), and the running
// maximum of the times as an inclusive max-scan over the chunk (six shuffle steps; a maximum is exact, so the grouping does
// not matter: tlk_time_key / tlk_time_max) with the last lane's value carried into the next chunk.  No LDS, no scratch.
__global__ __launch_bounds__(64) void mpmpc_plan_track_kernel(int B, int N, MapView map, const double* __restrict__ gx,
                                                              const double* __restrict__ gy, const double* __restrict__ trig,
                                                              int n_wp, int circular, const int* __restrict__ wp_id,
                                                              const int* __restrict__ alive, const int* __restrict__ status,
                                                              const double* __restrict__ z, const int* __restrict__ route,
                                                              int* __restrict__ valid, int* __restrict__ cells,
                                                              double* __restrict__ tm) {
  const int n = blockIdx.x, lane = threadIdx.x;
  if (n >= B) return;
  long long first = 0;
  if (route) {      // route fleets: the car's route
    const RouteView v = route_header(route, n);
    first = v.first;
    v.lengths(n_wp, circular);
  }
  if (lane == 0) valid[n] = tlk_valid(alive[n], status[n]) ? 1 : 0;
  const double* zn = z + (long long)(5 * N + 3) * n;
  const int wp = wp_id[n];
  double carry = 0.0;      // tm of the last stage of the chunk before (chunk 0: stage 0's own key)
  for (int j0 = 0; j0 <= N; j0 += 64) {      // (uniform)
    const int j = j0 + lane;
    const bool have = j <= N;
    double v = -HUGE_VAL;      // (past the plan's end: never taken)
    if (have) {
      const long long w = tlk_stage_row(wp, j, n_wp, circular != 0, first);
      int cell[2];
      tlk_stage_cell(map, gx[w], gy[w], trig[w * COR_TRIG], trig[w * COR_TRIG + 1], zn[3 * j], cell);
      int* o = cells + ((long long)n * (N + 1) + j) * 2;
      o[0] = cell[0]; o[1] = cell[1];
      v = tlk_time_key(j, zn[3 * j + 2]);
    }
    for (int m = 1; m < 64; m <<= 1) {      // inclusive scan: lane l ends with the leftmost maximum of lanes 0 .. l
      const double before = __shfl_up(v, m, 64);
      if (lane >= m) v = tlk_time_max(before, v);
    }
    v = tlk_time_max(carry, v);
    if (have) tm[(long long)n * (N + 1) + j] = v;
    carry = __shfl(v, 63, 64);
  }
}

// K3a: where is each car on the path, and what is its path-relative state (one thread per car)
// (alive: 0 = lap finished, s past the path's length; -2 = an open path's end reached, the reference's exit(1) in
//  get_waypoint - wp_id and x0 are still written, they are the state the reference computed before it exited)
__global__ __launch_bounds__(256) void mpmpc_localise_kernel(int B, int n_wp, int N, int circular, const double* __restrict__ cum,
                                                             const double* __restrict__ gx, const double* __restrict__ gy,
                                                             const double* __restrict__ gpsi, const double* __restrict__ s,
                                                             const double* __restrict__ pose, int* __restrict__ alive,
                                                             int* __restrict__ wp_id, double* __restrict__ x0,
                                                             int* __restrict__ shift, const int* __restrict__ route) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B || alive[i] != 1) return;
  if (route) {      // route fleets: the car's slice of cum and of the geometry, its route's length and flag; wp_id stays local
    const RouteView v = route_header(route, i);
    cum += v.first; gx += v.first; gy += v.first; gpsi += v.first;
    v.lengths(n_wp, circular);
  }
  const int wp = ro_current_waypoint(cum, n_wp, s[i]);
  if (wp < 0) { alive[i] = 0; return; }              // lap finished
  if (shift) {                                        // waypoints advanced since the last step (warm start)
    int d = wp - wp_id[i];
    if (d < 0) d += n_wp;
    shift[i] = d;
  }
  wp_id[i] = wp;
  ro_t2s(pose[3 * i], pose[3 * i + 1], pose[3 * i + 2], gx[wp], gy[wp], gpsi[wp], x0 + 3 * i);
  if (ro_past_open_end(n_wp, N, circular != 0, wp)) alive[i] = -2;     // end of an open path
}

// K3b: use the solution (or the fallback plan), drive the plant one step (one thread per car)
__global__ __launch_bounds__(256) void mpmpc_advance_kernel(int B, int N, double L, double Ts, const double* __restrict__ kappa,
                                                            const int* __restrict__ wp_id, const double* __restrict__ x0,
                                                            const int* __restrict__ status, const double* __restrict__ z,
                                                            double* __restrict__ cc, int* __restrict__ counter,
                                                            int* __restrict__ alive, double* __restrict__ pose,
                                                            double* __restrict__ s, double* __restrict__ u_last,
                                                            const int* __restrict__ route) {
  // one thread per (car, plan entry): the N arctangents of a car's new plan are independent; the thread of entry 0
  // then drives the car (it reads only plan entries it wrote itself, or - fallback - entries nobody writes)
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int i = g / N, k = g - i * N;
  if (i >= B || alive[i] != 1) return;
  const int n = 5 * N + 3;
  const int st = status[i];
  if (ro_usable(st)) ro_plan_entry(N, L, z + (long)i * n, cc + (long)i * 2 * N, k);
  if (k == 0 && !ro_drive(N, L, Ts, st, cc + (long)i * 2 * N, counter + i, x0 + 3 * i, kappa[wp_id[i] + (int)route_view(route, i, 0, 0).first], pose + 3 * i,
                          s + i, u_last + 2 * i))
    alive[i] = -1;
}

// K3r: the recorder of a rollout (mpmpc_rollout_record), two launches around a recorded step.  Both give every ENTRY of
// a car's record its own thread, and the record's fields lie car-major ([B][len], the host's layout): consecutive threads
// store consecutive words.  `rec` is the record's base address (64-bit arithmetic on the host).
//   snapshot  before localise: s, pose, alive as the step finds them (4 entries per car)
//   write     after advance: x0, u, wp_id, status, counter, alive, plan, predicted path, corridor row (ro_record_finish)
__global__ __launch_bounds__(256) void mpmpc_record_snapshot_kernel(int B, const double* __restrict__ s,
                                                                    const double* __restrict__ pose,
                                                                    const int* __restrict__ alive, int* __restrict__ a_in,
                                                                    char* __restrict__ rec, RoTraceLayout lay) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(g / RO_REC_BEGIN_ENTRIES), c = (int)(g - (long)i * RO_REC_BEGIN_ENTRIES);
  if (i >= B) return;
  ro_record_begin(s, pose, alive, a_in, rec, lay, i, c);
}
__global__ __launch_bounds__(256) void mpmpc_record_write_kernel(int B, RoRecSrc src, char* __restrict__ rec, RoTraceLayout lay) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(g / lay.entries), e = (int)(g - (long)i * lay.entries);
  if (i >= B) return;
  ro_record_finish(src, rec, lay, i, e);
}
// ... and a third launch behind `write` when a chain bit is selected (MPMPC_REC_PLANT .. MPMPC_REC_SCAN): the pose chain of the step
// from the features' own buffers (ro_record_chain; none of them is written again between its kernel and the end of the step), the
// same thread layout.  `rec` is the address of the record's chain.  No LDS, no scratch.
static_assert(RO_CHAIN_QUEUE == DL_MAX && RO_CHAIN_COV == ES_COV, "rollout_core.hpp disagrees with delay_core.hpp / estimator_core.hpp");
__global__ __launch_bounds__(256) void mpmpc_record_chain_kernel(int B, RoChainSrc src, char* __restrict__ rec, RoChainLayout lay) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(g / lay.entries), e = (int)(g - (long)i * lay.entries);
  if (i >= B) return;
  ro_record_chain(src, rec, lay, i, e);
}

// the footprint audit (mpmpc_footprint.hpp, which follows this header): its accumulators start over with a rollout
static int aud_reset(mpmpc_handle h, int B);
// refusals of the setters below; mpmpc_lookahead.hpp raises the first two as well
static const char* const LOOK_OVER_BUDGET = "the lookahead's disc table (movers x N x 12 bytes) would exceed 256 MiB (LOOK_TABLE_BUDGET)";
static const char* const TLK_OVER_BUDGET = "the traffic lookahead's disc table (B x slots x N x 12 bytes) would exceed 256 MiB (LOOK_TABLE_BUDGET)";
static const char* const WALLS_OTHER_B = "walls are set for another number of cars (mpmpc_rollout_set_walls)";

extern "C" {

int mpmpc_set_map(mpmpc_handle h, int32_t height, int32_t width, const int8_t* data, double origin_x,
                  double origin_y, double resolution) {
  if (int rc = enter(h, data)) return rc;
  if (height < 1 || width < 1 || !(resolution > 0)) return fail(MPMPC_E_ARG, "map needs positive size and resolution");
  if (height > COR_MAX_SIDE || width > COR_MAX_SIDE) return fail(MPMPC_E_ARG, "map sides are limited to 65534 cells");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(h->cor.map.alloc((size_t)height * width));
  HIP_TRY(hipMemcpyAsync(h->cor.map, data, (size_t)height * width, hipMemcpyHostToDevice, h->last().stream));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  h->cor.map_h = height; h->cor.map_w = width; h->cor.map_ox = origin_x; h->cor.map_oy = origin_y; h->cor.map_res = resolution;
  ++h->cor.base_gen;
  return MPMPC_OK;
}

int mpmpc_set_path_geometry(mpmpc_handle h, int32_t n_wp, const double* x, const double* y, const double* psi,
                            const double* border_ub, const double* border_lb) {
  if (int rc = enter(h, x && y && psi && border_ub && border_lb)) return rc;
  if (h->tab.n_wp == 0 || n_wp != h->tab.n_wp) return fail(MPMPC_E_STATE, "set the path first; n_wp must match it");
  HIP_TRY(hipSetDevice(h->cfg.device));
  h->cor.geom_n = 0;      // a failure below leaves "no geometry set"
  if (int rc = upload_table(h, h->cor.gx, x, n_wp)) return rc;
  if (int rc = upload_table(h, h->cor.gy, y, n_wp)) return rc;
  if (int rc = upload_table(h, h->cor.gpsi, psi, n_wp)) return rc;
  if (int rc = upload_table(h, h->cor.bub, border_ub, 2 * (size_t)n_wp)) return rc;
  if (int rc = upload_table(h, h->cor.blb, border_lb, 2 * (size_t)n_wp)) return rc;
  {
    // everything of a waypoint that needs libm, from the HOST's libm: the device tables then hold no device-libm
    // result (bit-exact against the reference's tables, golden G3)
    std::vector<double> trig((size_t)n_wp * COR_TRIG);
    for (int i = 0; i < n_wp; ++i) cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
    if (int rc = upload_table(h, h->cor.gtrig, trig.data(), trig.size())) return rc;
    HIP_TRY(hipStreamSynchronize(h->last().stream));      // `trig` leaves scope
  }
  h->cor.host_bub.assign(border_ub, border_ub + 2 * (size_t)n_wp);
  h->cor.host_blb.assign(border_lb, border_lb + 2 * (size_t)n_wp);
  const size_t nw = (size_t)n_wp;
  if (!h->cor.bad) HIP_TRY(h->cor.bad.alloc(2));
  HIP_TRY(alloc_all(Want{h->cor.segs, (4 * COR_MAXSEG + COR_WPC) * nw} /* + cor_forced rows */, Want{h->cor.nseg, nw},
                    Want{h->cor.line_cells, COR_CELL_CAP * nw}, Want{h->cor.line_box, COR_LINE_BOX * nw}));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  h->cor.geom_n = n_wp;
  ++h->cor.base_gen;
  return MPMPC_OK;
}

int mpmpc_build_corridor(mpmpc_handle h, int32_t n_cols, double min_width, double safety_margin, double* ub_out,
                         double* lb_out, int32_t* bad_rows) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  if (!h->cor.map || h->cor.geom_n == 0 || h->cor.geom_n != h->tab.n_wp)
    return fail(MPMPC_E_STATE, "needs mpmpc_set_path, mpmpc_set_map and mpmpc_set_path_geometry first");
  if (n_cols < h->cfg.N) return fail(MPMPC_E_ARG, "corridor table needs n_cols >= N");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int n = h->tab.n_wp;
  if (h->tab.n_cols != n_cols || !h->tab.ub_tab || !h->tab.lb_tab) {
    h->tab.n_cols = 0;      // a failure here leaves no table and no build
    h->cor.built_gen = 0;
    HIP_TRY(alloc_all(Want{h->tab.ub_tab, (size_t)n * n_cols}, Want{h->tab.lb_tab, (size_t)n * n_cols}));
  }
  const MapView mv = h->cor.map_view();
  const PathGeom pg = h->cor.path_geom(h->tab, h->cfg.circular);
  // the border cells of every waypoint must lie on the map of the moment (numpy indexing in the reference raises
  // IndexError past the upper edges and silently wraps around below zero: here both are an error)
  for (int i = 0; i < n; ++i) {
    int cx[2], cy[2];
    cor_w2m(mv, h->cor.host_bub[2 * i], h->cor.host_bub[2 * i + 1], cx[0], cy[0]);
    cor_w2m(mv, h->cor.host_blb[2 * i], h->cor.host_blb[2 * i + 1], cx[1], cy[1]);
    for (int e = 0; e < 2; ++e)
      if (cx[e] < 0 || cx[e] >= h->cor.map_w || cy[e] < 0 || cy[e] >= h->cor.map_h)
        return fail(MPMPC_E_ARG, "border cell of waypoint " + std::to_string(i) + " lies outside the map");
  }
  HIP_TRY(hipMemsetAsync(h->cor.bad, 0, 2 * sizeof(int), sl.stream));
  double* wpc = h->cor.forced_rows(h->tab);
  // One pair of launches per route (one path: one pair).  A route's view is its rows of every per-waypoint array - the geometry,
  // the border cells, K0a's caches, the table - with its own length and circular flag: the horizon walk of a start waypoint
  // wraps or clamps inside its route, and nothing in the kernels or in corridor_core.hpp knows of routes.
  const int P = h->tab.routes.n_routes ? h->tab.routes.n_routes : 1;
  for (int p = 0; p < P; ++p) {
    const size_t f = h->tab.routes.n_routes ? (size_t)h->tab.routes.first[p] : 0;
    const int np = h->tab.routes.n_routes ? h->tab.routes.first[p + 1] - h->tab.routes.first[p] : n;
    const PathGeom g{pg.x + f, pg.y + f, pg.psi + f, pg.ds_next + f, np, h->tab.routes.n_routes ? (h->tab.routes.circ[p] ? 1 : 0) : pg.circular,
                     pg.trig + f * COR_TRIG};
    double* const segs = h->cor.segs + f * 4 * COR_MAXSEG;
    hipLaunchKernelGGL(mpmpc_free_segments_kernel, dim3(np), dim3(64), 0, sl.stream, mv, g, h->cor.bub + 2 * f, h->cor.blb + 2 * f, min_width,
                       safety_margin, segs, h->cor.nseg + f, wpc + f * COR_WPC, h->cor.bad + 1, h->cor.line_cells + f * COR_CELL_CAP,
                       h->cor.line_box + f * COR_LINE_BOX);
    hipLaunchKernelGGL(mpmpc_corridor_select_kernel, dim3((np * n_cols + 255) / 256), dim3(256), 0, sl.stream, g, segs,
                       h->cor.nseg + f, n_cols, safety_margin, h->tab.ub_tab + f * n_cols, h->tab.lb_tab + f * n_cols, h->cor.bad,
                       wpc + f * COR_WPC);
  }
  HIP_TRY(hipGetLastError());
  int bad2[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(bad2, h->cor.bad, 2 * sizeof(int), hipMemcpyDeviceToHost, sl.stream));
  if (ub_out) HIP_TRY(hipMemcpyAsync(ub_out, h->tab.ub_tab, sizeof(double) * (size_t)n * n_cols, hipMemcpyDeviceToHost, sl.stream));
  if (lb_out) HIP_TRY(hipMemcpyAsync(lb_out, h->tab.lb_tab, sizeof(double) * (size_t)n * n_cols, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  h->cor.built_gen = 0;
  if (bad2[1] != 0) {
    h->tab.n_cols = 0;        // the table is not usable
    return fail(MPMPC_E_ARG, bad2[1] == 1 ? "a waypoint's border line has more than 1024 cells (COR_CELL_CAP)"
                                           : "a waypoint's border line has more than 8 free segments (COR_MAXSEG)");
  }
  const int bad = bad2[0];
  if (bad_rows) *bad_rows = bad;
  h->tab.n_cols = n_cols;
  h->cor.built_gen = h->cor.base_gen;
  h->cor.built_min_width = min_width;
  h->cor.built_sm = safety_margin;
  return MPMPC_OK;
}

int mpmpc_rollout_init(mpmpc_handle h, int32_t B, double Ts, const double* cum_lengths, const double* s,
                       const double* pose, const double* cc0) {
  if (int rc = enter(h, cum_lengths && s && pose)) return rc;
  Slot& sl = h->last();
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  if (!(Ts > 0)) return fail(MPMPC_E_ARG, "Ts must be > 0");
  if (h->tab.n_wp == 0 || h->cor.geom_n != h->tab.n_wp) return fail(MPMPC_E_STATE, "needs mpmpc_set_path and mpmpc_set_path_geometry");
  if (h->tab.n_cols == 0) return fail(MPMPC_E_STATE, "needs a corridor table (mpmpc_set_corridor / mpmpc_build_corridor)");
  if (h->rec.cap > 0 && h->rec.B != B) return fail(MPMPC_E_STATE, "mpmpc_rollout_record was set up for another number of cars");
  if (int rc = check_car_routes(h, B)) return rc;      // (routes: cum_lengths is the routes' own, each from 0, laid end to end)
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)h->cfg.max_batch;
  if (!h->ro.s)      // (all seven or none)
    HIP_TRY(alloc_all(Want{h->ro.s, mb}, Want{h->ro.pose, 3 * mb}, Want{h->ro.u, 2 * mb}, Want{h->ro.counter, mb}, Want{h->ro.alive, mb},
                      Want{h->ro.act, mb * h->ld}, Want{h->ro.shift, mb}));
  if (!h->obs.ro_flag) HIP_TRY(h->obs.ro_flag.alloc(mb));
  if (int rc = upload_table(h, h->ro.cum, cum_lengths, h->tab.n_wp)) return rc;
  const int N = h->cfg.N;
  if (B != h->io.laid_out) lay_out(h, B);
  HIP_TRY(hipMemcpyAsync(h->ro.s, s, sizeof(double) * B, hipMemcpyHostToDevice, sl.stream));
  HIP_TRY(hipMemcpyAsync(h->ro.pose, pose, sizeof(double) * 3 * B, hipMemcpyHostToDevice, sl.stream));
  if (cc0) HIP_TRY(hipMemcpyAsync(h->io.cc, cc0, sizeof(double) * 2 * N * B, hipMemcpyHostToDevice, sl.stream));
  else HIP_TRY(hipMemsetAsync(h->io.cc, 0, sizeof(double) * 2 * N * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->ro.counter, 0, sizeof(int) * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->ro.act, 0, sizeof(int) * (size_t)B * h->ld, sl.stream));     // no guess yet
  HIP_TRY(hipMemsetAsync(h->ro.shift, 0, sizeof(int) * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->ro.u, 0, sizeof(double) * 2 * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->io.wp_id, 0, sizeof(int) * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->io.x0, 0, sizeof(double) * 3 * B, sl.stream));
  HIP_TRY(hipMemsetAsync(sl.status, 0, sizeof(int) * B, sl.stream));
  const std::vector<int> ones((size_t)B, 1);
  HIP_TRY(hipMemcpyAsync(h->ro.alive, ones.data(), sizeof(int) * B, hipMemcpyHostToDevice, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  h->ro.Ts = Ts;
  h->ro.B = B;
  h->ro.valid = true;
  h->io.have_rows = false;       // the corridor comes from the table
  h->obs.car_rows = false;
  h->obs.discs_live = false;
  h->io.uploaded = B;
  h->rec.ro_steps = 0;            // the recorder keeps its configuration and starts over
  h->rec.count = 0;
  h->per.forget();                // what the cars know starts over; the setting stays
  h->look.ran_B = 0;              // (lookahead: the setting stays too, the last step's table is no step's of this rollout)
  h->tlk.forget();                // (... and no plan track is: every car is a frozen disc in the first step)
  if (h->pl.B > 0) {              // a plant in force keeps its parameters; its actuators and accumulators start over
    if (int rc = plant_reset(h, sl, h->pl.B, nullptr)) return rc;
  }
  if (h->dl.B > 0) {              // ... and a delay in force keeps d and c; its registers start over (zeros: the cars stand for d steps)
    if (int rc = delay_reset(h, sl, h->dl.B, nullptr)) return rc;
  }
  if (h->dy.B > 0) {              // ... and dynamics in force keep their parameters; the velocity states and accumulators start over
    if (int rc = dynamics_reset(h, sl, h->dy.B, nullptr)) return rc;
  }
  h->dy.verified = false;         // (Ts may have changed)
  if (h->es.B > 0) {              // ... and an estimator in force keeps its parameters; every car is un-primed, the statistics start over
    if (int rc = est_reset(h, sl, h->es.B, nullptr, nullptr)) return rc;
  }
  if (h->lc.B > 0) {              // ... and so does a localiser in force: its setting and its field stay
    if (int rc = loc_reset(h, sl, h->lc.B, nullptr)) return rc;
  }
  if (h->cm.B > 0) {              // ... and a commitment in force keeps its setting; the memory is emptied, the counters start over
    if (int rc = commitment_reset(h, sl)) return rc;
  }
  return aud_reset(h, B);         // ... and so does the audit (mpmpc_footprint.hpp)
}

int mpmpc_rollout_record(mpmpc_handle h, int32_t B, int32_t capacity, int32_t fields, int32_t stride) {
  if (int rc = enter(h)) return rc;
  if (capacity < 0) return fail(MPMPC_E_ARG, "capacity must be >= 0");
  if (stride < 1) return fail(MPMPC_E_ARG, "stride must be >= 1");
  if (fields & ~RO_REC_EVERY) return fail(MPMPC_E_ARG, "unknown bits in fields");
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  if (capacity > 0 && (fields & RO_REC_SCAN) && h->lc.B == 0)      // (the layout takes the setting's n_beams)
    return fail(MPMPC_E_STATE, "MPMPC_REC_SCAN needs a localiser in force (mpmpc_rollout_set_localiser)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  h->rec.buf.reset();
  h->rec.cap = h->rec.count = 0;
  if (capacity == 0) return MPMPC_OK;
  const RoTraceLayout lay = ro_trace_layout(h->cfg.N, B, fields);
  const RoChainLayout chain = ro_chain_layout(B, fields, h->lc.n_beams);
  const size_t bytes = (size_t)lay.bytes + (size_t)chain.bytes;
  if (!h->rec.ain) HIP_TRY(h->rec.ain.alloc((size_t)h->cfg.max_batch));
  if (h->rec.buf.alloc(bytes * (size_t)capacity)) {
    (void)hipGetLastError();
    return fail(MPMPC_E_HIP, "no device memory for " + std::to_string(capacity) + " records of " + std::to_string(bytes) + " bytes");
  }
  h->rec.lay = lay;
  h->rec.chain = chain;
  h->rec.cap = capacity;
  h->rec.B = B;
  h->rec.fields = fields;
  h->rec.stride = stride;
  return MPMPC_OK;
}

int mpmpc_rollout_recorded(mpmpc_handle h, int32_t* n_records, int32_t* n_steps) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (n_records) *n_records = h->rec.count;
  if (n_steps) *n_steps = (int32_t)h->rec.ro_steps;
  return MPMPC_OK;
}

// field `off` of records first .. first + count - 1 -> host [count][bytes]: one strided copy (dst == nullptr: not asked for)
static int pull_field(mpmpc_handle h, void* dst, long long off, size_t bytes, int first, int count) {
  if (!dst) return MPMPC_OK;
  const char* src = h->rec.buf + h->rec.rec_bytes() * (size_t)first + off;
  if (count == 1) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->last().stream));
  else HIP_TRY(hipMemcpy2DAsync(dst, bytes, src, h->rec.rec_bytes(), bytes, (size_t)count, hipMemcpyDeviceToHost, h->last().stream));
  return MPMPC_OK;
}

int mpmpc_rollout_trace(mpmpc_handle h, int32_t B, int32_t first, int32_t count, double* s, double* pose, int32_t* wp_id,
                        double* x0, double* u, int32_t* status, int32_t* counter, int32_t* alive, double* plan,
                        double* pred_x, double* pred_y, double* ub, double* lb) {
  if (int rc = enter(h)) return rc;
  if (first < 0 || count < 0) return fail(MPMPC_E_ARG, "first and count must be >= 0");
  if (h->rec.cap == 0) return fail(MPMPC_E_STATE, "recording is off (mpmpc_rollout_record)");
  if (B != h->rec.B) return fail(MPMPC_E_STATE, "mpmpc_rollout_record was set up for another number of cars");
  if ((long long)first + count > h->rec.count)
    return fail(MPMPC_E_STATE, "records " + std::to_string(first) + " .. " + std::to_string((long long)first + count - 1) +
                                   " asked for, " + std::to_string(h->rec.count) + " held");
  const RoTraceLayout& l = h->rec.lay;
  if ((plan && l.plan < 0) || ((pred_x || pred_y) && l.pred_x < 0) || ((ub || lb) && l.ub < 0))
    return fail(MPMPC_E_STATE, "a field was asked for that mpmpc_rollout_record did not select");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (count > 0) {
    const size_t N = (size_t)h->cfg.N, nb = (size_t)B;
    int rc = MPMPC_OK;      // (of the first copy that failed: nothing is enqueued behind it)
    auto field = [&](void* dst, long long off, size_t per_car) { if (!rc) rc = pull_field(h, dst, off, per_car * nb, first, count); };
    field(s, l.s, 8); field(pose, l.pose, 24); field(wp_id, l.wp_id, 4); field(x0, l.x0, 24); field(u, l.u, 16);
    field(status, l.status, 4); field(counter, l.counter, 4); field(alive, l.alive, 4);
    field(plan, l.plan, 16 * N); field(pred_x, l.pred_x, 8 * (N - 2)); field(pred_y, l.pred_y, 8 * (N - 2));
    field(ub, l.ub, 8 * N); field(lb, l.lb, 8 * N);
    if (rc) return rc;
  }
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  return MPMPC_OK;
}

int mpmpc_rollout_trace_chain(mpmpc_handle h, int32_t B, int32_t first, int32_t count, double* act, double* meas, double* queue,
                              double* pred_pose, double* pred_s, double* now, double* est, double* cov, int32_t* used, double* fix,
                              double* prior, int32_t* cand, int32_t* score, int32_t* hits, double* ranges) {
  if (int rc = enter(h)) return rc;
  if (first < 0 || count < 0) return fail(MPMPC_E_ARG, "first and count must be >= 0");
  if (h->rec.cap == 0) return fail(MPMPC_E_STATE, "recording is off (mpmpc_rollout_record)");
  if (B != h->rec.B) return fail(MPMPC_E_STATE, "mpmpc_rollout_record was set up for another number of cars");
  if ((long long)first + count > h->rec.count)
    return fail(MPMPC_E_STATE, "records " + std::to_string(first) + " .. " + std::to_string((long long)first + count - 1) +
                                   " asked for, " + std::to_string(h->rec.count) + " held");
  const RoChainLayout& l = h->rec.chain;
  if (((act || meas) && l.act < 0) || ((queue || pred_pose || pred_s || now) && l.queue < 0) || ((est || cov || used) && l.est < 0) ||
      ((fix || prior || cand || score || hits) && l.fix < 0) || (ranges && l.ranges < 0))
    return fail(MPMPC_E_STATE, "a field was asked for that mpmpc_rollout_record did not select");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (count > 0) {
    const size_t nb = (size_t)B;
    const long long at = h->rec.lay.bytes;      // the chain's start in a record
    int rc = MPMPC_OK;      // (of the first copy that failed: nothing is enqueued behind it)
    auto field = [&](void* dst, long long off, size_t per_car) { if (!rc) rc = pull_field(h, dst, at + off, per_car * nb, first, count); };
    field(act, l.act, 16); field(meas, l.meas, 24);
    field(queue, l.queue, 16 * (size_t)RO_CHAIN_QUEUE); field(pred_pose, l.pred_pose, 24); field(pred_s, l.pred_s, 8); field(now, l.now, 24);
    field(est, l.est, 24); field(cov, l.cov, 8 * (size_t)RO_CHAIN_COV); field(used, l.used, 4);
    field(fix, l.fix, 24); field(prior, l.prior, 24); field(cand, l.cand, 4); field(score, l.score, 4); field(hits, l.hits, 4);
    field(ranges, l.ranges, 8 * (size_t)l.n_beams);
    if (rc) return rc;
  }
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  return MPMPC_OK;
}

int mpmpc_rollout_set_counters(mpmpc_handle h, int32_t B, const int32_t* counter) {
  if (int rc = enter(h, counter)) return rc;
  if (int rc = h->ro.check(B)) return rc;
  for (int i = 0; i < B; ++i)
    if (counter[i] < 0 || counter[i] >= h->cfg.N - 1) return fail(MPMPC_E_ARG, "infeasibility counters must be in [0, N - 2]");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(hipMemcpyAsync(h->ro.counter, counter, sizeof(int) * B, hipMemcpyHostToDevice, h->last().stream));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  return MPMPC_OK;
}

// Lays out the device's per-car disc lists from the three host-side settings (st_* / mv_* / tr_*): combined offsets, the
// static discs in place, every mover and traffic slot as the absent disc (K0m and K0t fill the slots in front of every
// K0c), and the movers' slot indices.  new_mv: the movers' block as mpmpc_rollout_set_movers assembled it ([4][n] doubles, [2][n] ints kind / radius,
// the slots follow on the device), or NULL when the movers did not change (only their slot indices are written anew).
static int sync_disc_lists(mpmpc_handle h, std::vector<char>* new_mv) {
  const int B = h->obs.st_B > 0 ? h->obs.st_B : (h->obs.mv_B > 0 ? h->obs.mv_B : h->obs.tr_B);
  h->obs.obst_B = B;
  h->obs.discs_live = false;
  h->look.laid = false;      // (the lookahead's tables follow the lists: look_check_step lays them out anew)
  h->look.ran_B = 0;
  h->tlk.forget();
  if (B == 0) return MPMPC_OK;
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t mb = (size_t)h->cfg.max_batch;
  if (!h->obs.obst_off) HIP_TRY(alloc_all(Want{h->obs.obst_off, mb + 1}, Want{h->obs.obst_discs, 3 * COR_MAX_DISCS * mb}));      // (both or neither)
  if (!h->obs.ro_flag) HIP_TRY(h->obs.ro_flag.alloc(mb));
  const int n = h->obs.mv_B > 0 ? h->obs.mv_n : 0;
  h->obs.comb_off.assign((size_t)B + 1, 0);
  std::vector<int32_t> dst((size_t)n);
  mov_combine(B, h->obs.st_B > 0 ? h->obs.st_off.data() : nullptr, h->obs.mv_B > 0 ? h->obs.mv_off.data() : nullptr, h->obs.comb_off.data(),
              dst.data(), h->obs.tr_B > 0 ? h->obs.tr_S : 0);
  const size_t total = (size_t)h->obs.comb_off[B];
  std::vector<int32_t> discs(3 * total, 0);
  if (h->obs.st_B > 0)
    for (int b = 0; b < B; ++b)
      std::memcpy(discs.data() + 3 * (size_t)h->obs.comb_off[b], h->obs.st_discs.data() + 3 * (size_t)h->obs.st_off[b],
                  sizeof(int32_t) * 3 * (size_t)(h->obs.st_off[b + 1] - h->obs.st_off[b]));
  HIP_TRY(hipMemcpyAsync(h->obs.obst_off, h->obs.comb_off.data(), sizeof(int) * ((size_t)B + 1), hipMemcpyHostToDevice, sl.stream));
  if (total > 0) HIP_TRY(hipMemcpyAsync(h->obs.obst_discs, discs.data(), sizeof(int) * 3 * total, hipMemcpyHostToDevice, sl.stream));
  if (n > 0) {
    const size_t head = (sizeof(double) * MOV_PARAMS + 2 * sizeof(int)) * (size_t)n;      // parameters, kind, radius
    if (new_mv) {
      const size_t bytes = (sizeof(double) * MOV_PARAMS + 3 * sizeof(int)) * (size_t)n;      // + the slots
      if (bytes > h->obs.mv_block.count()) HIP_TRY(h->obs.mv_block.alloc(bytes));             // (only grows)
      HIP_TRY(hipMemcpyAsync(h->obs.mv_block, new_mv->data(), head, hipMemcpyHostToDevice, sl.stream));
    }
    HIP_TRY(hipMemcpyAsync(h->obs.mv_block + head, dst.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, sl.stream));
  }
  HIP_TRY(hipStreamSynchronize(sl.stream));      // the host vectors leave scope
  return MPMPC_OK;
}

int mpmpc_rollout_set_obstacles(mpmpc_handle h, int32_t B, const int32_t* offsets, const int32_t* discs) {
  if (int rc = enter(h)) return rc;
  h->per.forget();      // the worlds change: what the cars know of them starts over
  if (!offsets) {      // no static discs: back to the shared table, unless movers or traffic are set
    h->obs.st_B = 0;
    return sync_disc_lists(h, nullptr);
  }
  const char* why = "";
  if (int rc = cor_check_obstacles(B, h->cfg.max_batch, offsets, discs, h->cor.built(h->tab), h->cor.map_w, h->cor.map_h, &why))
    return fail(rc == -3 ? MPMPC_E_STATE : MPMPC_E_ARG, why);
  if (int rc = mov_check_combined(B, offsets, h->obs.mv_B, h->obs.mv_off.data(), &why, h->obs.tr_B, h->obs.tr_S))
    return fail(rc == -3 ? MPMPC_E_STATE : MPMPC_E_ARG, why);
  if (h->obs.wl_B > 0 && h->obs.wl_B != B) return fail(MPMPC_E_STATE, WALLS_OTHER_B);
  h->obs.st_off.assign(offsets, offsets + (size_t)B + 1);
  h->obs.st_discs.assign(discs, discs + 3 * (size_t)offsets[B]);
  h->obs.st_B = B;
  h->obs.obst_gen = h->cor.base_gen;
  return sync_disc_lists(h, nullptr);
}

int mpmpc_rollout_set_movers(mpmpc_handle h, int32_t B, const int32_t* offsets, const int32_t* kind,
                             const int32_t* radius_cells, const double* params, int64_t step0) {
  if (int rc = enter(h)) return rc;
  h->per.forget();      // the worlds change: what the cars know of them starts over
  if (!offsets) {      // no movers
    h->obs.mv_B = 0;
    h->obs.mv_n = 0;
    return sync_disc_lists(h, nullptr);
  }
  const char* why = "";
  if (int rc = mov_check_movers(B, h->cfg.max_batch, offsets, kind, radius_cells, params, h->cor.built(h->tab), h->obs.st_B, h->obs.st_off.data(), &why,
                                h->obs.tr_B, h->obs.tr_S))
    return fail(rc == -3 ? MPMPC_E_STATE : MPMPC_E_ARG, why);
  if (h->obs.wl_B > 0 && h->obs.wl_B != B) return fail(MPMPC_E_STATE, WALLS_OTHER_B);
  if (h->look.max_lead > 0 && look_table_bytes(offsets[B], h->cfg.N) > LOOK_TABLE_BUDGET) return fail(MPMPC_E_ARG, LOOK_OVER_BUDGET);
  const size_t n = (size_t)offsets[B];
  std::vector<char> blk((sizeof(double) * MOV_PARAMS + 2 * sizeof(int)) * n);
  double* p = (double*)blk.data();
  int32_t* ki = (int32_t*)(p + MOV_PARAMS * n);
  for (size_t j = 0; j < n; ++j) {
    for (int t = 0; t < MOV_PARAMS; ++t) p[(size_t)t * n + j] = params[MOV_PARAMS * j + t];
    ki[j] = kind[j];
    ki[n + j] = radius_cells[j];
  }
  h->obs.mv_off.assign(offsets, offsets + (size_t)B + 1);
  h->obs.mv_B = B;
  h->obs.mv_n = (int)n;
  h->obs.mv_step0 = step0;
  h->obs.mv_gen = h->cor.base_gen;
  return sync_disc_lists(h, &blk);
}

int mpmpc_rollout_set_traffic(mpmpc_handle h, int32_t B, const int32_t* group, const int32_t* radius_cells, int32_t slots,
                              int32_t range_cells) {
  if (int rc = enter(h)) return rc;
  h->per.forget();      // the worlds change: what the cars know of them starts over
  if (!group) {      // no traffic
    h->obs.tr_B = 0;
    return sync_disc_lists(h, nullptr);
  }
  const char* why = "";
  if (int rc = tr_check_traffic(B, h->cfg.max_batch, group, radius_cells, slots, h->cor.built(h->tab), h->obs.st_B, h->obs.st_off.data(),
                                h->obs.mv_B, h->obs.mv_off.data(), &why))
    return fail(rc == -3 ? MPMPC_E_STATE : MPMPC_E_ARG, why);
  if (h->obs.wl_B > 0 && h->obs.wl_B != B) return fail(MPMPC_E_STATE, WALLS_OTHER_B);
  if (h->tlk.on && h->look.max_lead > 0 && tlk_table_bytes(B, slots, h->cfg.N) > LOOK_TABLE_BUDGET) return fail(MPMPC_E_ARG, TLK_OVER_BUDGET);
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t nb = (size_t)B;
  std::vector<int32_t> blk(4 * nb + 1);      // dense group, radius, members, the groups' offsets
  const int G = tr_layout(B, group, blk.data(), blk.data() + 3 * nb, blk.data() + 2 * nb);
  std::memcpy(blk.data() + nb, radius_cells, sizeof(int32_t) * nb);
  if (!h->obs.tr_block) HIP_TRY(h->obs.tr_block.alloc(4 * (size_t)h->cfg.max_batch + 1));
  HIP_TRY(hipMemcpyAsync(h->obs.tr_block, blk.data(), sizeof(int) * (3 * nb + (size_t)G + 1), hipMemcpyHostToDevice, h->last().stream));
  HIP_TRY(hipStreamSynchronize(h->last().stream));      // `blk` leaves scope
  h->obs.tr_B = B;
  h->obs.tr_S = slots;
  h->obs.tr_range = range_cells;
  h->obs.tr_gen = h->cor.base_gen;
  return sync_disc_lists(h, nullptr);
}

int mpmpc_rollout_set_walls(mpmpc_handle h, int32_t B, const int32_t* offsets, const int32_t* walls) {
  if (int rc = enter(h)) return rc;
  h->per.forget();      // the worlds change: what the cars know of them starts over
  if (!offsets) {      // no walls
    if (h->obs.wl_B > 0) h->obs.discs_live = false;      // (the worlds change; without walls in force the call changes nothing)
    h->obs.wl_B = 0;
    h->obs.wl_n = 0;
    return MPMPC_OK;
  }
  const char* why = "";
  if (int rc = wall_check_walls(B, h->cfg.max_batch, offsets, walls, h->cor.built(h->tab), h->cor.map_w, h->cor.map_h, h->obs.obst_B, &why))
    return fail(rc == -3 ? MPMPC_E_STATE : MPMPC_E_ARG, why);
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t n = (size_t)offsets[B];
  std::vector<int32_t> hdr(WALL_HDR * n + 1);
  const size_t total = (size_t)wall_layout((long)n, walls, hdr.data());
  // a refused call leaves the setting as it was: the new table is built in buffers of its own and swapped in at the end
  Buf<int> n_off, n_hdr, n_tab, n_raw, n_ok;
  HIP_TRY(alloc_all(Want{n_off, (size_t)h->cfg.max_batch + 1}, Want{n_hdr, WALL_HDR * n + 1}, Want{n_tab, total + 1}, Want{n_raw, 4 * n + 1},
                    Want{n_ok, n + 1}));
  std::vector<int32_t> ok(n, 1);
  HIP_TRY(hipMemcpyAsync(n_off, offsets, sizeof(int) * ((size_t)B + 1), hipMemcpyHostToDevice, sl.stream));
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(n_hdr, hdr.data(), sizeof(int) * WALL_HDR * n, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemcpyAsync(n_raw, walls, sizeof(int) * 4 * n, hipMemcpyHostToDevice, sl.stream));
    hipLaunchKernelGGL(mpmpc_wall_raster_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, sl.stream, (int)n, n_raw.get(), n_hdr.get(),
                       n_tab.get(), n_ok.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ok.data(), n_ok, sizeof(int) * n, hipMemcpyDeviceToHost, sl.stream));
  }
  HIP_TRY(hipStreamSynchronize(sl.stream));      // the host vectors leave scope
  for (size_t j = 0; j < n; ++j)
    if (ok[j] != 1) return fail(MPMPC_E_ARG, "wall " + std::to_string(j) + " does not fit the wall table (csrc/wall_core.hpp, step 3)");
  h->obs.wl_off = std::move(n_off); h->obs.wl_hdr = std::move(n_hdr); h->obs.wl_tab = std::move(n_tab);
  h->obs.wl_raw = std::move(n_raw); h->obs.wl_ok = std::move(n_ok);
  h->obs.wl_B = B;
  h->obs.wl_n = (int)n;
  h->obs.wl_gen = h->cor.base_gen;
  h->obs.discs_live = false;      // the worlds were set anew: those of the last step are gone
  return MPMPC_OK;
}

int mpmpc_rollout_obstacles(mpmpc_handle h, int32_t B, int32_t* discs_out, int32_t* offsets_out) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B)) return rc;
  if (!h->obs.car_rows || !h->obs.discs_live || B != h->obs.obst_B)      // (a world of walls only has no disc lists)
    return fail(MPMPC_E_STATE, "the last rollout step did not build per-car rows for B cars, or the obstacles / movers / traffic were set "
                               "anew since (mpmpc_rollout_set_obstacles / mpmpc_rollout_set_movers / mpmpc_rollout_set_traffic)");
  if (offsets_out) std::memcpy(offsets_out, h->obs.comb_off.data(), sizeof(int32_t) * ((size_t)B + 1));
  if (discs_out && h->obs.comb_off[B] > 0) {
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipMemcpyAsync(discs_out, h->obs.obst_discs, sizeof(int) * 3 * (size_t)h->obs.comb_off[B], hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
  }
  return MPMPC_OK;
}

int mpmpc_rollout_corridor(mpmpc_handle h, int32_t B, double* ub, double* lb) {
  if (int rc = enter(h, ub && lb)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B)) return rc;
  if (!h->obs.car_rows) return fail(MPMPC_E_STATE, "the last rollout step did not build per-car rows (mpmpc_rollout_set_obstacles)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t nb = (size_t)B * h->cfg.N;
  std::vector<int> flag(B);
  HIP_TRY(hipMemcpyAsync(ub, h->io.ub, sizeof(double) * nb, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipMemcpyAsync(lb, h->io.lb, sizeof(double) * nb, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipMemcpyAsync(flag.data(), h->obs.ro_flag, sizeof(int) * B, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  for (int b = 0; b < B; ++b)
    if (flag[b] != COR_ROW_OK)
      for (int n = 0; n < h->cfg.N; ++n) ub[(size_t)b * h->cfg.N + n] = lb[(size_t)b * h->cfg.N + n] = std::nan("");
  return MPMPC_OK;
}

int mpmpc_rollout_warm_start(mpmpc_handle h, int32_t enable) {
  if (int rc = enter(h)) return rc;
  h->ro.warm = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
  return MPMPC_OK;
}

int mpmpc_rollout_state(mpmpc_handle h, int32_t B, double* s, double* pose, double* cc, int32_t* wp_id, double* x0,
                        double* u_last, int32_t* status, int32_t* counter, int32_t* alive) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B, "the rollout's state was overwritten by an upload / solve / assemble on this handle: "
                              "call mpmpc_rollout_init again")) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t N = (size_t)h->cfg.N, nb = (size_t)B;
  HIP_TRY(pull(sl.stream, s, h->ro.s, nb));
  HIP_TRY(pull(sl.stream, pose, h->ro.pose, 3 * nb));
  HIP_TRY(pull(sl.stream, cc, h->io.cc, 2 * N * nb));
  HIP_TRY(pull(sl.stream, wp_id, h->io.wp_id, nb));
  HIP_TRY(pull(sl.stream, x0, h->io.x0, 3 * nb));
  HIP_TRY(pull(sl.stream, u_last, h->ro.u, 2 * nb));
  HIP_TRY(pull(sl.stream, status, sl.status, nb));
  HIP_TRY(pull(sl.stream, counter, h->ro.counter, nb));
  HIP_TRY(pull(sl.stream, alive, h->ro.alive, nb));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

}  // extern "C"
