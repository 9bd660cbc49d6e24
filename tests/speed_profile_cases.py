"""Named inputs of the speed profile (K4) and an exact reference for them that shares nothing with any solver in the tree.

The problem (csrc/speed_core.hpp):   min 1/2 |v|^2 - hi' v   s.t.  a_min <= c_i (v[i+1] - v[i]) <= a_max,  v_min <= v <= hi,
c_i = 1 / (2 li_i), hi_i = min(v_max, sqrt(ay_max / (|kappa_i| + eps))) - the Euclidean projection of hi onto a polytope.

reference():  Lawson-Hanson least-distance programming, one scipy.optimize.nnls call.  With the rows G v >= g, G = [D; -D; I; -I],
    h = g - G hi,  E = [G'; h'],  f = e_{n+1},  u = nnls(E, f),  r = E u - f,  v = hi - r[:n] / r[n]
(with two scalings that do not move the minimiser, see reference(), and a textbook Lawson-Hanson iteration in numpy for the few
cases where scipy's nnls stops short of its own optimality conditions), followed by ONE refinement step: the equality-constrained
projection of hi onto the rows that are active at that v (lstsq on those rows: the minimum-norm correction is the projection).
kkt():  plain-numpy optimality check of ANY candidate v: worst constraint violation, and the stationarity residual
    |v - hi - G_A' lam|_inf with lam >= 0 from nnls on the rows within 1e-7 of their bound.  v is the optimum iff both are zero
    (the problem is strictly convex), whatever produced it.

Validation of reference() against the certified fixtures (max |v - x|, asserted by test_reference_against_certified_fixtures):
    g2_speed_profile.npz       (Sim_Track,  n = 199):  nnls alone 1.6e-15,   with the refinement step 8.0e-15
    g2_speed_profile_real.npz  (Real_Track, n = 301):  nnls alone 2.2e-16,   with the refinement step 2.2e-16
Both are a million times below the 1e-8 bar the tests hold the kernels to, so these tracks do not ask for the refinement step.
It stays for the thin polytopes of tiny_li (rows with c = 500): there nnls alone ends at constraint violations of 2e-10, the
refined point at 1.5e-11 (kkt() over all cases: violation <= 1.5e-11, stationarity <= 5e-13).

The references of all cases take two minutes to compute (nnls on a dense (n + 1) x (4 n - 2) matrix: 2 s at n = 384, 30 s where
the numpy iteration has to step in), so their v is recorded in tests/golden/g9_speed_profile_cases.npz
(python tests/speed_profile_cases.py writes it) and the tests load that.  The record is not trusted: tests/test_speed_profile.py
runs kkt() on every recorded v against the inputs generated here, and recomputes reference() for the sizes up to 129.

Families (li, kappa, limits (a_min, a_max, v_min, v_max, ay_max)); random ones are seeded by (family, n):
    hairpin        hairpin - straight - hairpin: li 0.05, kappa 20 on the first and last n // 10 + 1 points, limits (-0.1, 0.05, 0, 5, 1)
    hairpin_loose  the same path, loose acceleration (-10, 10, 0, 1, 4)
    tiny_li        li 1e-3, kappa 30 (u - 0.5) on half the points, (-0.01, 0.01, 0, 2, 1)
    sawtooth       li 0.05, kappa 50 / 0 alternating, (-0.2, 0.2, 0, 1.5, 2)
    li_decades     li 10^U(-3, 1), kappa as tiny_li, (-0.3, 0.3, 0, 1, 4)
    vmin_positive  li 0.05, kappa as tiny_li, (-0.05, 0.05, 0.25, 1, 4)
    constant       li 0.05, kappa 3, (-0.3, 0.3, 0, 1, 4)
    straight       li 0.05, kappa 0 (the cap is sqrt(ay_max / eps)), (-0.3, 0.3, 0, 1, 4)
    iid            the generator of test_speed_profile_path_lengths: li U(0.03, 0.06), kappa N(0, 2) on half the points, random limits

What the iid inputs of the older tests lacked is long runs of consecutive ACTIVE acceleration rows.  Longest run per family,
from the reference (accel_run(); ACCEL_RUNS holds every case):
    n = 200:  hairpin 159, hairpin_loose 0, tiny_li 199, sawtooth 199, li_decades 7, vmin_positive 26, constant 0, straight 0, iid 24
    n = 384:  hairpin 204, hairpin_loose 0, tiny_li 268, sawtooth 383, li_decades 6, vmin_positive 28, constant 0, straight 0, iid 19
    n = 385:  hairpin 205, hairpin_loose 0, tiny_li 133, sawtooth 384, li_decades 8, vmin_positive 29, constant 0, straight 0, iid 28
    n = 420:  hairpin 223, hairpin_loose 0, tiny_li 115, sawtooth 419, li_decades 8, vmin_positive 24, constant 0, straight 0, iid 79
On the hairpin the speed peak falls exactly on a waypoint at n = 64 and n = 200 (rising rows, falling rows and the boxes at both
ends: one active row more than unknowns - a degenerate vertex).  recorded() asserts that some case has a run of at least 150 rows.
"""
from __future__ import annotations

import os

import numpy as np

EPS = 1e-12
FAMILIES = ("hairpin", "hairpin_loose", "tiny_li", "sawtooth", "li_decades", "vmin_positive", "constant", "straight", "iid")
SIZES_WAVE = (2, 3, 63, 64, 65, 128, 129, 200, 256, 257, 384)        # one wavefront per path; 384 fills the LDS
SIZES_THREAD = (385, 420)                                             # the thread-per-path kernel
SIZES = SIZES_WAVE + SIZES_THREAD
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_speed_profile_cases.npz")
ACTIVE_TOL = 1e-7


def make(family, n):
    """-> li [n], kappa [n], limits [5] of the named case."""
    rng = np.random.default_rng([FAMILIES.index(family), n])
    li = np.full(n, 0.05)
    half = lambda: 30.0 * (rng.uniform(0, 1, n) - 0.5) * (rng.uniform(0, 1, n) < 0.5)
    if family in ("hairpin", "hairpin_loose"):
        k = n // 10 + 1
        kappa = np.zeros(n)
        kappa[:k] = kappa[n - k:] = 20.0
        lim = (-0.1, 0.05, 0.0, 5.0, 1.0) if family == "hairpin" else (-10.0, 10.0, 0.0, 1.0, 4.0)
    elif family == "tiny_li":
        li, kappa, lim = np.full(n, 1e-3), half(), (-0.01, 0.01, 0.0, 2.0, 1.0)
    elif family == "sawtooth":
        kappa, lim = 50.0 * (np.arange(n) % 2 == 0), (-0.2, 0.2, 0.0, 1.5, 2.0)
    elif family == "li_decades":
        li, kappa, lim = 10.0 ** rng.uniform(-3, 1, n), half(), (-0.3, 0.3, 0.0, 1.0, 4.0)
    elif family == "vmin_positive":
        kappa, lim = half(), (-0.05, 0.05, 0.25, 1.0, 4.0)
    elif family == "constant":
        kappa, lim = np.full(n, 3.0), (-0.3, 0.3, 0.0, 1.0, 4.0)
    elif family == "straight":
        kappa, lim = np.zeros(n), (-0.3, 0.3, 0.0, 1.0, 4.0)
    elif family == "iid":
        li = rng.uniform(0.03, 0.06, n)
        kappa = rng.normal(0.0, 2.0, n) * (rng.uniform(0, 1, n) < 0.5)
        lim = (-rng.uniform(0.05, 0.5), rng.uniform(0.1, 1.0), 0.0, rng.uniform(0.6, 1.5), rng.uniform(1.0, 5.0))
    else:
        raise KeyError(family)
    return np.ascontiguousarray(li, float), np.ascontiguousarray(kappa, float), np.array(lim, float)


def rows(li, kappa, lim, eps=EPS):
    """-> hi [n], G [4 n - 2, n], g: the constraints as G v >= g, rows [D; -D; I; -I]."""
    n = len(li)
    a_min, a_max, v_min, v_max, ay_max = lim
    hi = np.minimum(v_max, np.sqrt(ay_max / (np.abs(kappa) + eps)))
    D = np.zeros((n - 1, n))
    c = 1.0 / (2.0 * np.asarray(li)[:n - 1])
    D[np.arange(n - 1), np.arange(n - 1)] = -c
    D[np.arange(n - 1), np.arange(1, n)] = c
    G = np.vstack([D, -D, np.eye(n), -np.eye(n)])
    g = np.hstack([np.full(n - 1, a_min), np.full(n - 1, -a_max), np.full(n, v_min), -hi])
    return hi, G, g


def _lawson_hanson(A, b, tol=1e-12):
    """argmin |A x - b|, x >= 0: the textbook active-set iteration with a fresh lstsq per step (slow, and robust)."""
    n = A.shape[1]
    P, x, w = np.zeros(n, bool), np.zeros(n), A.T @ b
    while True:
        wz = np.where(P, -np.inf, w)
        j = int(np.argmax(wz))
        if not wz[j] > tol:
            return x
        P[j] = True
        while True:
            s = np.zeros(n)
            s[P] = np.linalg.lstsq(A[:, P], b, rcond=None)[0]
            if s[P].min() > 0:
                break
            bad = P & (s <= 0)
            x = x + np.min(x[bad] / (x[bad] - s[bad])) * (s - x)
            P &= x > 1e-15
            x[~P] = 0.0
        x, w = s, A.T @ (b - A @ s)


def reference(li, kappa, lim, eps=EPS, refine=True):
    """The optimum v [n] (module docstring).  Two scalings that leave the minimiser where it is keep nnls well-conditioned:
    h is divided by sig, an upper bound of the distance |v - hi| (a constant profile at min(hi) is feasible), so that the last
    component of r is about 1/2 instead of 1 / (1 + |v - hi|^2); and every column of E is normalised."""
    from scipy.optimize import nnls
    hi, G, g = rows(li, kappa, lim, eps)
    n = len(hi)
    sig = np.linalg.norm(hi - hi.min())
    if sig == 0.0:
        return hi                                # a constant cap: hi itself is feasible
    h = (g - G @ hi) / sig
    w = 1.0 / np.sqrt((G * G).sum(axis=1) + h * h)
    E = np.vstack([(G * w[:, None]).T, (h * w)[None, :]])
    f = np.zeros(n + 1)
    f[n] = 1.0
    u, _ = nnls(E, f, maxiter=30 * E.shape[1])
    if np.max(E.T @ (f - E @ u)) > 1e-10:        # nnls gave up short of its own optimality conditions (tiny_li: the rows
        u = _lawson_hanson(E, f)                 # D and -D are parallel to 1e-5 there)
    r = E @ u - f
    v = hi - sig * r[:n] / r[n]
    if refine:
        act = G @ v - g <= ACTIVE_TOL
        if act.any():
            v = hi + np.linalg.lstsq(G[act], g[act] - G[act] @ hi, rcond=None)[0]
    return v


def kkt(li, kappa, lim, v, eps=EPS):
    """-> (worst constraint violation, stationarity residual) of the candidate v, both >= 0 and 0 at the optimum."""
    from scipy.optimize import nnls
    hi, G, g = rows(li, kappa, lim, eps)
    slack = G @ v - g
    act = slack <= ACTIVE_TOL
    d = v - hi                                   # gradient of 1/2 |v - hi|^2: must be G_A' lam, lam >= 0
    stat = np.max(np.abs(d))
    if act.any():
        lam, _ = nnls(G[act].T, d, maxiter=30 * int(act.sum()))
        stat = np.max(np.abs(G[act].T @ lam - d))
    return max(0.0, float(-slack.min())), float(stat)


def accel_run(li, lim, v):
    """Longest run of consecutive acceleration rows at a bound (within ACTIVE_TOL) at v."""
    a = (v[1:] - v[:-1]) / (2.0 * np.asarray(li)[:len(v) - 1])
    on = (a - lim[0] <= ACTIVE_TOL) | (lim[1] - a <= ACTIVE_TOL)
    best = cur = 0
    for b in on:
        cur = cur + 1 if b else 0
        best = max(best, cur)
    return best


def case_id(family, n):
    return "%s-%d" % (family, n)


CASES = [(f, n) for n in SIZES for f in FAMILIES]
_record = None
ACCEL_RUNS = {}


def recorded(family, n):
    """The recorded reference v of a case (read-only array)."""
    global _record
    if _record is None:
        with np.load(RECORD) as z:
            _record = {k: z[k] for k in z.files}
        for k in _record.values():
            k.setflags(write=False)
        for f, m in CASES:
            li, _, lim = make(f, m)
            ACCEL_RUNS[case_id(f, m)] = accel_run(li, lim, _record[case_id(f, m)])
        assert max(ACCEL_RUNS.values()) >= 150, ACCEL_RUNS
    return _record[case_id(family, n)]


def batch(n, families=FAMILIES):
    """One path per family at size n -> LI [B, n], KA [B, n], LIM [B, 5], VREF [B, n]."""
    parts = [make(f, n) for f in families]
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]),
            np.stack([recorded(f, n) for f in families]))


if __name__ == "__main__":
    import time
    out = {}
    for f, n in CASES:
        t0 = time.time()
        li, kappa, lim = make(f, n)
        out[case_id(f, n)] = reference(li, kappa, lim)
        print("%-20s %6.2f s  kkt %.1e %.1e  run %d" % ((case_id(f, n), time.time() - t0) + kkt(li, kappa, lim, out[case_id(f, n)])
                                                       + (accel_run(li, lim, out[case_id(f, n)]),)), flush=True)
    np.savez_compressed(RECORD, **out)
