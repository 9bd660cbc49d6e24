// The skeleton of an emulated solve launch (TEST INFRASTRUCTURE ONLY), shared by emul.cpp and emul_wide.cpp: the steps of a
// solve kernel under the names they have on the device (mpmpc_hip.hip, "the steps of a solve kernel") - here over the waves of
// a launch in turn, on an assembled QP, with lists that are appended to in order.  Include after lane_emu.hpp, lane_pair.hpp and
// the solver headers.
#pragma once
#include <type_traits>
#include <vector>

struct Problem {          // what a launch solves ...
  const mpmpc_config* cfg;
  const mpmpc_settings* st;
  const double* qp;
  int B;
};
struct Outputs {          // ... and where its results go
  double *z, *u0;
  int *status, *iters;
  double *resid, *y;
};

inline const VI& first(const VI& v) { return v; }          // the first stage of every lane: with two stages per lane, component 0
inline const VI& first(const I2& v) { return v.v[0]; }
template <class I>
inline I both(const VI& v) {                               // one value per lane, for both of its stages
  if constexpr (std::is_same<I, VI>::value) return v; else return I(v, v);
}

// step 2, batch order: wave w carries the instances w * per_wave .. (ids >= B: "none")
struct BatchOrder {
  template <class L> int waves(int B) const { return (B + L::per_wave - 1) / L::per_wave; }
  template <class L> typename L::ival inst(int w, int) const { return L::slot() + w * L::per_wave; }
};
// ... list order: the waves take consecutive entries of a tail list; the last wave of a packed launch may carry B = "none"
struct ListOrder {
  const int* ids;
  int n;
  ListOrder(const int* ids_, int n_) : ids(ids_), n(n_) {}
  ListOrder(const std::vector<int>& v) : ids(v.data()), n((int)v.size()) {}
  template <class L> int waves(int) const { return (n + L::per_wave - 1) / L::per_wave; }
  template <class L> typename L::ival inst(int w, int B) const {
    const VI slot = first(L::slot());
    VI r;
    for (int i = 0; i < EMU_W; ++i) {
      const int e = w * L::per_wave + slot.v[i];
      r.v[i] = e < n ? ids[e] : B;
    }
    return both<typename L::ival>(r);
  }
};
template <class L>
inline typename L::ival stage_of_lane(int N) { return L::stage() - lane_offset(L::group, L::split, N); }

// step 3: the active sets to start from (closed loop; null: none)
inline VI warm_guess(const int* guess, int ld, const VI& inst, const VI& k, int B, int N) {
  VI g(0);
  for (int i = 0; i < EMU_W; ++i)
    if (guess && inst.v[i] < B && k.v[i] >= 0 && k.v[i] <= N) g.v[i] = guess[inst.v[i] * ld + k.v[i]];
  return g;
}
// (an argument of step 5 in the tail kernels: the interior-point iterations an earlier kernel spent on the lane's instance)
template <class I>
inline I spent_ipm(const int* iters, const I& inst, int B) {
  VI r(0);
  for (int i = 0; i < EMU_W; ++i)
    if (first(inst).v[i] < B) r.v[i] = iters[first(inst).v[i] * 2 + 1];
  return both<I>(r);
}

// step 8: stage 0 of an instance left MPMPC_UNSOLVED appends it to the list of the next kernel - in ascending order here
template <class I, class St>
inline void leave_to_tail(std::vector<int>& list, const I& inst, const I& k, int B, const St& status) {
  for (int i = 0; i < EMU_W; ++i)
    if (first(k).v[i] == 0 && first(inst).v[i] < B && first(status).v[i] == MPMPC_UNSOLVED) list.push_back(first(inst).v[i]);
}

// One emulated launch of a kernel whose solver is S on the lanes L: for every wave of the order - ids (2), the fields of the
// assembled QP (4), `solve` = the kernel's own run and store (5, 7), and what it leaves (8; left = null: a kernel without a list)
template <class S, class L, class Order, class Solve>
static void wave_loop(const Problem& p, const Order& order, std::vector<int>* left, Solve&& solve) {
  const int N = p.cfg->N, ld = stage_ld(N);
  for (int w = 0; w < order.template waves<L>(p.B); ++w) {
    const typename L::ival inst = order.template inst<L>(w, p.B);
    const typename L::ival k = stage_of_lane<L>(N);
    S s;
    typename L::real fields[MPMPC_NUM_FIELDS];
    S::fetch_fields(p.qp, p.B, ld, inst, k, N, fields);
    solve(s, fields, inst, k);
    if (left) leave_to_tail(*left, inst, k, p.B, s.status);
  }
}

// mpmpc_reduced_kernel and its forms with two stages per lane / on a workgroup: the reduced-native solver; the instances it
// leaves UNSOLVED are appended to tail.  guess / act (one stage per lane only): the closed loop's active sets, in and out
template <class L, bool CR = true>
static void solve_rn(const Problem& p, const Outputs& o, std::vector<int>& tail, const int* guess = nullptr, int* act = nullptr) {
  using S = ReducedSolver<L, CR>;
  const int N = p.cfg->N, ld = stage_ld(N);
  wave_loop<S, L>(p, BatchOrder{}, &tail, [&](S& s, const typename L::real* fields, const typename L::ival& inst, const typename L::ival& k) {
    if constexpr (L::stages_per_lane == 1) {
      if (guess) s.template run<true>(fields, p.B, inst, k, N, make_params(*p.st), warm_guess(guess, ld, inst, k, p.B, N));
    }
    if (!guess) s.template run<false>(fields, p.B, inst, k, N, make_params(*p.st));
    s.store(inst, k, p.cfg->wheelbase, o.z, o.u0, o.status, o.iters, o.resid, o.y, act, ld);
  });
}
// mpmpc_reduced_t_kernel (and forms): the reduced-native solver of the weightings with a terminal cost on the time state
template <class L, bool CR = true>
static void solve_rnt(const Problem& p, const Outputs& o, std::vector<int>& tail) {
  using S = ReducedTSolver<L, CR>;
  wave_loop<S, L>(p, BatchOrder{}, &tail, [&](S& s, const typename L::real* fields, const typename L::ival& inst, const typename L::ival& k) {
    s.run(fields, p.B, inst, k, p.cfg->N, make_params(*p.st), p.cfg->QN[2]);
    s.store(inst, k, p.cfg->wheelbase, o.z, o.u0, o.status, o.iters, o.resid, o.y);
  });
}
// mpmpc_reduced_tail_kernel (and forms): the reduced-native tail solver on the listed instances; what it leaves goes to tail2
template <class L>
static void solve_rn_tail(const Problem& p, const Outputs& o, const ListOrder& list, std::vector<int>& tail2) {
  using S = ReducedTailSolver<L>;
  wave_loop<S, L>(p, list, &tail2, [&](S& s, const typename L::real* fields, const typename L::ival& inst, const typename L::ival& k) {
    s.run(fields, p.B, inst, k, p.cfg->N, make_params(*p.st), spent_ipm(o.iters, inst, p.B));
    s.store(inst, k, p.cfg->wheelbase, o.z, o.u0, o.status, o.iters, o.resid, o.y);
  });
}
// (an exported entry point hands a list back as ids + count)
inline void list_out(const std::vector<int>& list, int* ids, int* n) {
  *n = (int)list.size();
  for (int i = 0; i < *n; ++i) ids[i] = list[i];
}
