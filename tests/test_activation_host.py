"""tests/activation_ref.py, the NumPy restatement the GPU tests of the activation map compare against, pinned on the host: its
crossings against ``diagnostics.threshold_crossings``, hand-made traces for every rule of the detector, and the velocity on fields
whose gradient is known in closed form."""
import math

import numpy as np
import pytest

from activation_ref import TOL, detector_ref, summary_ref, time_tol, velocity_ref
from cgx_hip.activation import parse_activation_key
from cgx_hip.diagnostics import threshold_crossings


def _one(trace, times, thr, down=None):
    r = detector_ref(np.asarray(trace, dtype=np.float64)[:, None], times, thr, down)
    return {k: v[0] for k, v in r.items()}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_count_and_first_crossing_equal_threshold_crossings(seed):
    rng = np.random.default_rng(seed)
    R, n = 40, 200
    times = np.cumsum(rng.uniform(0.1, 2.0, R))
    trace = np.cumsum(rng.normal(0.0, 1.0, (R, n)), axis=0)
    trace[rng.integers(1, R, 30), rng.integers(0, n, 30)] = 0.5          # samples exactly on the threshold
    count, first = threshold_crossings(trace, times, 0.5)
    r = detector_ref(trace, times, 0.5)
    assert count.max() >= 3 and (count == 0).any()
    assert np.array_equal(r["count"], count)
    assert np.array_equal(np.isnan(r["t_act"]), np.isnan(first))
    ok = count > 0
    assert np.array_equal(r["t_act"][ok], first[ok])                     # the same expression in the same order: the same bits
    assert np.all(r["t_last"][ok] >= r["t_act"][ok]) and np.array_equal(r["t_last"][count == 1], r["t_act"][count == 1])


def test_sample_on_the_threshold_counts_once_when_reached_not_when_left():
    t = [0.0, 1.0, 2.0, 3.0]
    r = _one([-1.0, 0.0, 1.0, 2.0], t, 0.0)          # v1 == thr: an upward crossing at the sample's own time
    assert r["count"] == 1 and r["t_act"] == 1.0
    r = _one([0.0, 1.0, 2.0, 3.0], t, 0.0)           # v0 == thr and rising: not one
    assert r["count"] == 0 and math.isnan(r["t_act"]) and math.isnan(r["t_last"])
    r = _one([0.0, -1.0, 0.0, 1.0], t, 0.0)          # leaves downwards, comes back onto it
    assert r["count"] == 1 and r["t_act"] == 2.0


def test_two_crossings_and_repolarisation():
    t = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    r = _one([-2.0, 2.0, -2.0, -1.0, 3.0, 3.0], t, 0.0)
    assert r["count"] == 2 and r["t_act"] == 0.5 and r["t_last"] == 3.25
    assert r["t_repol"] == 1.5 and r["apd"] == 1.0                       # the first fall after the first rise; later ones do not move it
    assert [k for k, _ in r["t_cross"]] == [1, 4]
    # a repolarisation threshold of its own
    r = _one([-2.0, 2.0, -2.0, -1.0, 3.0, 3.0], t, 0.0, down=1.0)
    assert r["t_repol"] == 1.25


def test_fall_before_the_first_rise_is_ignored():
    t = [0.0, 1.0, 2.0, 3.0, 4.0]
    r = _one([1.0, -1.0, -1.0, 1.0, 2.0], t, 0.0)
    assert r["count"] == 1 and r["t_act"] == 2.5 and math.isnan(r["t_repol"]) and math.isnan(r["apd"])


def test_equal_peaks_keep_the_first_and_the_initial_value_counts():
    t = [0.0, 1.0, 2.0, 3.0, 4.0]
    r = _one([0.0, 5.0, 1.0, 5.0, 2.0], t, 10.0)
    assert r["v_peak"] == 5.0 and r["t_peak"] == 1.0 and r["k_peak"] == 1
    r = _one([7.0, 5.0, 1.0, 5.0, 2.0], t, 10.0)
    assert r["v_peak"] == 7.0 and r["t_peak"] == 0.0 and r["k_peak"] == 0
    assert r["dvdt_max"] == 4.0 and r["t_dvdt"] == 2.5 and r["k_dvdt"] == 3


def test_nan_record_leaves_no_crossing():
    t = [0.0, 1.0, 2.0, 3.0, 4.0]
    r = _one([-1.0, float("nan"), 1.0, -1.0, 1.0], t, 0.0)
    assert r["count"] == 1 and r["t_act"] == 3.5                         # -1 -> NaN -> 1 is no crossing: both intervals record nothing
    assert r["v_peak"] == 1.0 and r["t_peak"] == 2.0                     # the value after the NaN still counts as a peak
    assert r["dvdt_max"] == 2.0 and r["k_dvdt"] == 4                     # neither interval next to the NaN has a slope
    r = _one([float("nan"), 1.0, 2.0], t[:3], 0.0)                       # armed on a NaN: v_peak stays NaN (every comparison is false)
    assert r["count"] == 0 and math.isnan(r["v_peak"]) and r["dvdt_max"] == 1.0


def test_non_uniform_times():
    t = [0.0, 0.5, 2.5, 2.75]
    r = _one([-1.0, -0.5, 1.5, 1.0], t, 0.0, down=1.25)
    assert r["t_act"] == 0.5 + 0.25 * 2.0 and r["t_repol"] == 2.5 + 0.5 * 0.25
    assert r["dvdt_max"] == 1.0 and r["t_dvdt"] == 0.25                  # (0.5 / 0.5) beats (2 / 2): strict, the first stays
    assert time_tol(2.75, 0.25) == 8 * 2.0 ** -52 * 2.75


def _plane_case(seed):
    """a planar membrane of arbitrary triangles in 3D: vertices o + s u + t w with orthonormal u, w"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    u, w, nrm = q[:, 0], q[:, 1], q[:, 2]
    st = rng.uniform(-1.0, 1.0, (40, 2))
    X = rng.normal(size=3) + st[:, :1] * u + st[:, 1:] * w
    fv = np.array([rng.choice(40, 3, replace=False) for _ in range(60)])
    return X, fv, nrm


@pytest.mark.parametrize("seed", [3, 4])
def test_plane_wave_on_a_planar_membrane(seed):
    X, fv, nrm = _plane_case(seed)
    k = np.random.default_rng(seed + 10).normal(size=3) * 3.0
    T = X @ k + 0.7
    kt = k - (k @ nrm) * nrm                        # the tangential part of k: the surface gradient of T
    r = velocity_ref(X, fv, T)
    assert r["valid"].all()
    assert np.allclose(r["speed"], 1.0 / np.linalg.norm(kt), rtol=1e-9, atol=0)
    assert np.allclose(r["direction"], kt / np.linalg.norm(kt), rtol=0, atol=1e-9)
    assert np.allclose(np.linalg.norm(r["direction"], axis=1), 1.0, rtol=1e-12)
    assert np.all(r["gg_unc"] >= r["gg"]) and np.all(r["g_unc"] >= np.abs(r["g"]))


def test_segment_formula_and_invalid_facets():
    X = np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 0.0], [6.0, 0.0]])
    fv = np.array([[0, 1], [1, 0], [1, 2], [2, 3], [0, 2]])
    T = np.array([1.0, 3.5, 3.5, float("nan")])
    r = velocity_ref(X, fv, T)
    assert list(r["valid"]) == [True, True, False, False, True]         # equal times: no gradient; a NaN vertex: no velocity
    assert r["speed"][0] == 2.0 and np.array_equal(r["direction"][0], [0.6, 0.8])
    assert r["speed"][1] == 2.0 and np.array_equal(r["direction"][1], [0.6, 0.8])          # the direction does not follow the vertex order
    assert r["speed"][4] == 1.2 and np.array_equal(r["direction"][4], [1.0, 0.0])
    assert np.isnan(r["speed"][2:4]).all() and np.isnan(r["direction"][2:4]).all()
    assert r["gg"][2] == 0.0 and np.isnan(r["gg"][3])
    # triangles: a constant field and a NaN vertex
    X3 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0]])
    r = velocity_ref(X3, np.array([[0, 1, 2], [1, 2, 3], [0, 1, 2]]), np.array([2.0, 2.0, 2.0, float("nan")]))
    assert not r["valid"].any() and np.isnan(r["speed"]).all()
    r = velocity_ref(X3, np.array([[0, 1, 2]]), np.array([0.0, 0.5, 0.0, 0.0]))
    assert r["valid"][0] and r["speed"][0] == 2.0 and np.array_equal(r["direction"][0], [1.0, 0.0, 0.0])


def test_facets_of_measure_zero_have_no_velocity():
    X3 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    r = velocity_ref(X3, np.array([[0, 1, 2], [0, 1, 3]]), np.array([0.0, 1.0, 3.0, 2.0]))      # collinear vertices: det == 0
    assert list(r["valid"]) == [False, True] and np.isnan(r["speed"][0]) and np.isnan(r["direction"][0]).all()
    X2 = np.array([[1.0, 1.0], [1.0, 1.0], [2.0, 1.0]])
    r = velocity_ref(X2, np.array([[0, 1], [0, 2]]), np.array([0.0, 1.0, 2.0]))                   # a segment of length zero
    assert list(r["valid"]) == [False, True] and np.isnan(r["speed"][0]) and r["speed"][1] == 0.5
    rows, _, meas, _ = summary_ref(X2, np.array([[0, 1], [0, 2]]), np.array([4, 4]), np.array([0.0, 1.0, 2.0]), [[4]])
    assert rows[0, 0] == 1.0 and list(meas) == [0.0, 1.0]                                          # it adds nothing to the valid area


def test_summary_rows():
    X = np.array([[0.0, 0.0], [1.0, 0.0], [3.0, 0.0], [6.0, 0.0], [10.0, 0.0]])
    fv = np.array([[0, 1], [1, 2], [2, 3], [3, 4]])
    tags = np.array([5, 5, 7, 9])
    T = np.array([0.0, 0.5, 1.5, float("nan"), float("nan")])
    rows, cover, meas, S1 = summary_ref(X, fv, tags, T, [[5], [11], [7, 9]])
    assert [list(c) for c in cover] == [[0, 1], [], [2, 3]] and list(meas) == [1.0, 2.0, 3.0, 4.0]
    assert list(rows[0]) == [3.0, 1.0 * 2.0 + 2.0 * 2.0, 0.0, 1.5, 3.0]
    assert list(rows[1]) == [0.0, 0.0, np.inf, -np.inf, 0.0]             # an empty group: the identity
    assert list(rows[2]) == [0.0, 0.0, 1.5, 1.5, 1.5]                    # no valid facet, one fired vertex of the four
    assert list(S1) == [1.5 * 6.0, 0.0, 0.0] and TOL == 1e-12               # in 2D nothing cancels: gg_unc = gg


def test_output_key():
    assert parse_activation_key({}, (1, 2)) is None and parse_activation_key({"save_activation": False}, (1, 2)) is None
    assert parse_activation_key({"save_activation": True}, (1, 2)) == {"threshold": 0.0, "repolarisation_threshold": 0.0, "tags": None}
    got = parse_activation_key({"save_activation": {"threshold": -0.02, "tags": [2]}}, (1, 2))
    assert got == {"threshold": -0.02, "repolarisation_threshold": -0.02, "tags": [2]}
    assert parse_activation_key({"save_activation": {"threshold": 0.01, "repolarisation_threshold": -0.05}}, (1,))["repolarisation_threshold"] == -0.05
    for bad in ([1, 2], {"treshold": 0.0}, {"threshold": float("nan")}, {"tags": [1, 1]}, {"tags": [1, 7]}):
        with pytest.raises(ValueError):
            parse_activation_key({"save_activation": bad}, (1, 2))
