"""Independent NumPy restatement of the activation map (test infrastructure: the checker of csrc/knp_activation.inc and
cgx_hip/activation.py).  Written from the definitions of include/knpemi_hip.h: the detector as an explicit loop over the records
and the vertices, the velocity as an explicit loop over the facets from the coordinates, the per-group rows with NumPy sums, minima
and maxima.  Plain Python floats: IEEE double, no fused multiply-add.

Bounds the tests use.  An interpolated time t0 + q h is one divide, one multiply and one add after exact-to-one-rounding
differences; with or without contraction of the multiply-add that is a few roundings of a value no larger than max(|t1|, h):
``time_tol`` = 8 * 2^-52 * max(|t1|, h).  The slope (v1 - v0)/h is two roundings: 4 * 2^-52 |s|.  The velocity is compared through
|g|^2 = (c d1^2 - 2 b d1 d2 + a d2^2)/det, whose evaluations differ by the order and contraction of a handful of products: TOL = 1e-12
(the project's summation-order bound, tests/phim_ref.py) of the un-cancelled sum (c d1^2 + 2 |b d1 d2| + a d2^2)/det, and the
components of g likewise against their un-cancelled sums.
"""
import math

import numpy as np

EPS = 2.0 ** -52
TOL = 1e-12
NAN = float("nan")


def time_tol(t1, h):
    return 8.0 * EPS * max(abs(t1), h)


def detector_ref(trace, times, thr_up, thr_down=None):
    """``trace`` [records, n]: phi_m at the listed vertices, record 0 is the state at ``arm()``; ``times`` [records].  Returns the
    dict of ``ActivationMap.result()`` plus ``k_peak`` / ``k_dvdt`` (the record at which the peak was taken / the interval, by its
    end record, of the steepest upstroke; -1 where dvdt_max is still -inf), ``k_act`` / ``k_last`` / ``k_repol`` (the end record of
    the interval of that event, -1 without one) and ``t_cross`` (per vertex the list of (record, time) of every upward crossing)."""
    v = np.asarray(trace, dtype=np.float64)
    t = [float(x) for x in times]
    thr_down = thr_up if thr_down is None else thr_down
    R, n = v.shape
    out = {k: np.full(n, NAN) for k in ("t_act", "t_last", "t_repol", "t_dvdt")}
    out["v_peak"] = v[0].copy()
    out["t_peak"] = np.full(n, t[0])
    out["dvdt_max"] = np.full(n, -np.inf)
    out["count"] = np.zeros(n, dtype=np.int64)
    out["k_peak"] = np.zeros(n, dtype=np.int64)
    for key in ("k_dvdt", "k_act", "k_last", "k_repol"):
        out[key] = np.full(n, -1, dtype=np.int64)
    out["t_cross"] = [[] for _ in range(n)]
    for j in range(n):
        last = float(v[0, j])
        for k in range(1, R):
            t0, t1 = t[k - 1], t[k]
            h = t1 - t0
            v0, v1 = last, float(v[k, j])
            if v0 < thr_up and v1 >= thr_up:
                tx = t0 + (thr_up - v0) / (v1 - v0) * h
                out["count"][j] += 1
                if out["count"][j] == 1:
                    out["t_act"][j], out["k_act"][j] = tx, k
                out["t_last"][j], out["k_last"][j] = tx, k
                out["t_cross"][j].append((k, tx))
            if out["count"][j] > 0 and math.isnan(out["t_repol"][j]) and v0 >= thr_down and v1 < thr_down:
                out["t_repol"][j], out["k_repol"][j] = t0 + (v0 - thr_down) / (v0 - v1) * h, k
            if v1 > out["v_peak"][j]:
                out["v_peak"][j], out["t_peak"][j], out["k_peak"][j] = v1, t1, k
            s = (v1 - v0) / h
            if s > out["dvdt_max"][j]:
                out["dvdt_max"][j], out["t_dvdt"][j], out["k_dvdt"][j] = s, t0 + 0.5 * h, k
            last = v1
    out["apd"] = out["t_repol"] - out["t_act"]
    return out


def velocity_ref(coords, facet_vertices, T):
    """Per facet (rows of ``facet_vertices`` [n, d], d = 2 segments / 3 triangles) from the vertex coordinates and the nodal ``T``:
    ``valid`` [n], ``speed`` [n], ``direction`` [n, dim] (NaN where invalid), ``gg`` = |g|^2 and ``gg_unc`` its un-cancelled sum,
    ``g`` [n, dim] and ``g_unc`` [n, dim] the un-cancelled sums of its components (all NaN where a T is not finite)."""
    X = np.asarray(coords, dtype=np.float64)
    fv = np.asarray(facet_vertices)
    n, d = fv.shape
    dim = X.shape[1]
    valid = np.zeros(n, dtype=bool)
    speed, gg, ggu = np.full(n, NAN), np.full(n, NAN), np.full(n, NAN)
    direction, g, gu = np.full((n, dim), NAN), np.full((n, dim), NAN), np.full((n, dim), NAN)
    for i in range(n):
        x = [[float(c) for c in X[v]] for v in fv[i]]
        tt = [float(T[v]) for v in fv[i]]
        if not all(math.isfinite(q) for q in tt):
            continue
        if d == 2:
            e = [x[1][c] - x[0][c] for c in range(dim)]
            L = math.sqrt(sum(q * q for q in e))
            dT = tt[1] - tt[0]
            if L == 0.0:
                continue
            gg[i] = ggu[i] = dT * dT / (L * L)
            g[i] = [dT * q / (L * L) for q in e]
            gu[i] = [abs(q) for q in g[i]]
            if dT != 0.0 and L > 0.0:
                valid[i] = True
                speed[i] = L / abs(dT)
                direction[i] = [math.copysign(1.0, dT) * q / L for q in e]
            continue
        e1 = [x[1][c] - x[0][c] for c in range(dim)]
        e2 = [x[2][c] - x[0][c] for c in range(dim)]
        a = sum(p * q for p, q in zip(e1, e1))
        b = sum(p * q for p, q in zip(e1, e2))
        c = sum(p * q for p, q in zip(e2, e2))
        det = a * c - b * b
        if det == 0.0:
            continue
        d1, d2 = tt[1] - tt[0], tt[2] - tt[0]
        gg[i] = (c * d1 * d1 - 2.0 * b * d1 * d2 + a * d2 * d2) / det
        ggu[i] = (c * d1 * d1 + 2.0 * abs(b * d1 * d2) + a * d2 * d2) / det
        w1, w2 = (c * d1 - b * d2) / det, (a * d2 - b * d1) / det
        u1, u2 = (c * abs(d1) + abs(b * d2)) / det, (a * abs(d2) + abs(b * d1)) / det
        g[i] = [w1 * p + w2 * q for p, q in zip(e1, e2)]
        gu[i] = [u1 * abs(p) + u2 * abs(q) for p, q in zip(e1, e2)]
        if gg[i] > 0.0 and math.isfinite(gg[i]):
            valid[i] = True
            ln = math.sqrt(gg[i])
            speed[i] = 1.0 / ln
            direction[i] = [q / ln for q in g[i]]
    return {"valid": valid, "speed": speed, "direction": direction, "gg": gg, "gg_unc": ggu, "g": g, "g_unc": gu}


def facet_measures(coords, facet_vertices):
    X = np.asarray(coords, dtype=np.float64)[np.asarray(facet_vertices)]
    if X.shape[1] == 2:
        return np.linalg.norm(X[:, 1] - X[:, 0], axis=1)
    return 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)


def summary_ref(coords, facet_vertices, facet_tags, T, groups):
    """The rows of knp_diag_activation for ``groups`` (lists of membrane tags; a facet goes to the first group that lists its tag) over
    the given facets: [n_groups, 5] = (valid area, sum |F| speed over the valid facets, min T, max T, activated area), the facets
    every group covered, the facet measures, and ``S1`` [n_groups], what the tolerance of the speed sum scales with: all its terms are
    positive, so two evaluations differ by TOL sum |F| speed for the order of the sum plus sum |F| |d speed|, and a speed 1/sqrt(gg)
    follows a relative error TOL gg_unc/gg of gg with half of it: S1 = sum |F| speed (1 + gg_unc/(2 gg))."""
    fv = np.asarray(facet_vertices)
    tags = np.asarray(facet_tags)
    T = np.asarray(T, dtype=np.float64)
    d = fv.shape[1]
    vel = velocity_ref(coords, fv, T)
    meas = facet_measures(coords, fv)
    first = {}
    for t, grp in enumerate(groups):
        for tag in grp:
            first.setdefault(int(tag), t)
    group_of = np.array([first.get(int(q), -1) for q in tags], dtype=np.int64)
    rows = np.zeros((len(groups), 5))
    rows[:, 2], rows[:, 3] = np.inf, -np.inf
    S1 = np.zeros(len(groups))
    cover = []
    for t in range(len(groups)):
        F = np.nonzero(group_of == t)[0]
        cover.append(F)
        if not len(F):
            continue
        ok = vel["valid"][F]
        rows[t, 0] = meas[F][ok].sum()
        rows[t, 1] = (meas[F][ok] * vel["speed"][F][ok]).sum()
        S1[t] = (meas[F][ok] * vel["speed"][F][ok] * (1.0 + 0.5 * vel["gg_unc"][F][ok] / vel["gg"][F][ok])).sum()
        tv = T[fv[F]]
        fin = np.isfinite(tv)
        if fin.any():
            rows[t, 2], rows[t, 3] = tv[fin].min(), tv[fin].max()
        rows[t, 4] = (meas[F] / d * fin.sum(axis=1)).sum()
    return rows, cover, meas, S1
