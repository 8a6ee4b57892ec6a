"""CPU: the long-double truth of expected hypervolume improvement (tests/_ehvi_truth.py) against three things it does not share
code with -- a Monte Carlo mean of exact hypervolume differences, central differences of itself, and the K = 2 strip formula
written out by hand -- and its own special function against tabulated values."""
import numpy as np
import pytest

import _ehvi_truth as ET

T = ET.T


def _hv(P, ref):
    """Exact dominated hypervolume inside (-inf, ref] by inclusion-exclusion over the points (n <= 6 here): nothing in common
    with the sweeps of the package or the cells of the truth."""
    P = [p for p in np.asarray(P, dtype=float).reshape(-1, len(ref)) if np.all(p < ref)]
    total = 0.0
    for mask in range(1, 1 << len(P)):
        sub = [P[i] for i in range(len(P)) if mask >> i & 1]
        total += (-1) ** (len(sub) + 1) * np.prod(ref - np.max(sub, axis=0))
    return total


def _setup(K, seed, n=5, M=3, D=4):
    rng = np.random.default_rng(seed)
    mean, var = rng.normal(0, 0.6, (K, M)), rng.uniform(0.02, 0.4, (K, M))
    dm, dv = rng.normal(size=(K, M, D)), 0.2 * rng.normal(size=(K, M, D))
    y_mean, y_std = rng.normal(0, 0.3, K), rng.uniform(0.6, 1.8, K)
    P, ref = rng.normal(0, 0.7, (n, K)), np.full(K, 1.6)
    return mean, var, dm, dv, y_mean, y_std, P, ref


def test_erfc_in_long_double():
    # 25-digit values at the float64 arguments (any multiprecision package reproduces them)
    table = {0.0: "1", 0.5: "0.4795001221869534623172533", 1.0: "0.1572992070502851306587794", 2.0: "0.004677734981047265837930744",
             5.0: "1.537459794428034850188343e-12", 10.0: "2.088487583762544757000786e-45", -1.0: "1.842700792949714869341221",
             0.999: "0.1577147297935030583610317"}
    for x, want in table.items():
        got, want = ET.erfc(T(x)), T(want)
        assert abs(got - want) <= 8 * np.finfo(T).eps * want, (x, got, want)


@pytest.mark.parametrize("K", [2, 3])
def test_truth_against_monte_carlo_of_exact_hypervolume_differences(K):
    mean, var, dm, dv, y_mean, y_std, P, ref = _setup(K, 11 + K, M=2)
    levels, lo, hi = ET.cells_of(P, ref)
    t = ET.ehvi(mean, var, None, None, y_mean, y_std, levels, lo, hi, bound=False)
    rng = np.random.default_rng(99)
    base = _hv(P, ref)
    S = 1500
    for j in range(mean.shape[1]):
        y = np.asarray(t.m[:, j], float) + np.asarray(t.s[:, j], float) * rng.standard_normal((S, K))
        gain = np.array([_hv(np.vstack((P, yi)), ref) - base for yi in y])
        se = gain.std(ddof=1) / np.sqrt(S)
        print("EHVI truth K=%d location %d: %.6f, Monte Carlo %.6f +- %.6f" % (K, j, float(t.value[j]), gain.mean(), se))
        assert abs(gain.mean() - float(t.value[j])) <= 4 * se


@pytest.mark.parametrize("K", [2, 3])
def test_gradient_against_central_differences_of_the_truth(K):
    """x enters through the posterior alone: mean(x + h e_d) = mean + h dmdx_d, var(x + h e_d) = var + h dvdx_d to first order, so
    the directional derivative of the truth along (dmdx_d, dvdx_d) in (mean, var) is the gradient's component d."""
    mean, var, dm, dv, y_mean, y_std, P, ref = _setup(K, 21 + K)
    levels, lo, hi = ET.cells_of(P, ref)
    t = ET.ehvi(mean, var, dm, dv, y_mean, y_std, levels, lo, hi, bound=False)
    h = T(1e-7)

    def value(mean_, var_):
        # (long-double inputs: the truth's float64 cast would swallow the step)
        lev = []
        for k in range(K):
            m = mean_[k] * T(y_std[k]) + T(y_mean[k])
            s = np.sqrt(var_[k] * T(y_std[k]) ** 2)
            z = (np.asarray(levels[k], dtype=T)[1:, None] - m[None, :]) / s[None, :]
            lev.append(np.vstack((np.zeros((1, m.size), T), s[None, :] * (z * ET.ndtr(z) + ET.npdf(z)))))
        return np.prod([lev[k][hi[:, k]] - lev[k][lo[:, k]] for k in range(K)], axis=0).sum(0)

    mean_l, var_l = mean.astype(T), var.astype(T)
    for d in range(dm.shape[2]):
        up = value(mean_l + h * dm[:, :, d], var_l + h * dv[:, :, d])
        dn = value(mean_l - h * dm[:, :, d], var_l - h * dv[:, :, d])
        num = (up - dn) / (2 * h)
        # truncation h^2 |f'''| / 6 ~ 1e-14 and cancellation eps |f| / h ~ 1e-12 of values of order one
        assert np.max(np.abs(num - t.grad[:, d])) <= 1e-10 * max(1.0, float(np.max(np.abs(t.grad)))), d


def test_two_objectives_against_the_strip_formula_written_out():
    mean, var, dm, dv, y_mean, y_std, P, ref = _setup(2, 5, n=6)
    levels, lo, hi = ET.cells_of(P, ref)
    t = ET.ehvi(mean, var, None, None, y_mean, y_std, levels, lo, hi, bound=False)
    F = ET.front_of(P[np.all(P < ref, axis=1)])                      # sorted by the first objective
    a = np.concatenate(([-np.inf], F[:, 0], [ref[0]]))
    b = np.concatenate(([ref[1]], F[:, 1]))

    def Psi(c, m, s):
        if not np.isfinite(c):
            return T(0)
        z = (T(c) - m) / s
        return s * (z * ET.ndtr(z) + ET.npdf(z))

    for j in range(mean.shape[1]):
        m, s = t.m[:, j], t.s[:, j]
        want = sum((Psi(a[i + 1], m[0], s[0]) - Psi(a[i], m[0], s[0])) * Psi(b[i], m[1], s[1]) for i in range(len(F) + 1))
        assert abs(want - t.value[j]) <= 1e-17 * max(1.0, abs(float(want)))


def test_the_bound_covers_a_float64_evaluation_and_propagate_covers_a_perturbed_posterior():
    """Not the device, but the same operations in NumPy's float64: the derived bound has to hold for it too; and a posterior moved
    by small amounts moves the truth by no more than ``propagate`` says (first order, so with 1 % to spare)."""
    for K in (2, 3):
        mean, var, dm, dv, y_mean, y_std, P, ref = _setup(K, 31 + K, M=4)
        levels, lo, hi = ET.cells_of(P, ref)
        t = ET.ehvi(mean, var, dm, dv, y_mean, y_std, levels, lo, hi)
        m = mean * y_std[:, None] + y_mean[:, None]
        s = np.sqrt(np.maximum(var * (y_std * y_std)[:, None], 1e-10))
        from scipy.special import erfc
        val = 0.0
        D = []
        for k in range(K):
            z = (levels[k][1:, None] - m[k][None, :]) / s[k][None, :]
            psi = s[k][None, :] * (z * (0.5 * erfc(-z / np.sqrt(2.0))) + np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi))
            psi = np.vstack((np.zeros((1, m.shape[1])), psi))
            D.append(psi[hi[:, k]] - psi[lo[:, k]])
        val = np.prod(D, axis=0).sum(0)
        assert np.all(np.abs(val - t.value) <= t.bound_value)
        rng = np.random.default_rng(K)
        e_mean, e_sd = 1e-7 * rng.uniform(0.2, 1, mean.shape), 1e-7 * rng.uniform(0.2, 1, mean.shape)
        e_dm, e_dv = 1e-7 * rng.uniform(0.2, 1, dm.shape), 1e-7 * rng.uniform(0.2, 1, dv.shape)
        sd = np.sqrt(var)
        sign = rng.choice([-1.0, 1.0], mean.shape)
        t2 = ET.ehvi(mean + sign * e_mean, (sd + sign * e_sd) ** 2, dm + e_dm, dv - e_dv, y_mean, y_std, levels, lo, hi, bound=False)
        tv, tg = ET.propagate(t, y_std, lo, hi, e_mean, e_sd, e_dm, e_dv, dm, dv)
        assert np.all(np.abs(t2.value - t.value) <= 1.01 * tv + 1e-18)
        assert np.all(np.abs(t2.grad - t.grad) <= 1.01 * tg + 1e-18)
