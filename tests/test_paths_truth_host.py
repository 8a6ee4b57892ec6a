"""CPU: the long-double truth of the posterior paths (tests/_paths_truth.py) against plain NumPy double, its gradient against
central differences of its own value, the interpolation identity, and the laws of ``posterior_paths.unit_frequencies`` and of the
paths themselves against the oracle's posterior."""
import numpy as np
import pytest

from gaussian_process_optimization_amd import posterior_paths as PP
from oracle import cpu_ref as O

import _kernel_families as KF
import _paths_truth as PT
import _sparse_ref as SR

T = PT.T
FAMS = ("rbf", "Mat52", "Mat32", "Exponential")


def _small(fam, N=20, D=2, S=3, F=30, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(4 * X.sum(1)) + 0.1 * rng.standard_normal(N)
    ls = np.array([0.4, 0.7])[:D]
    Xq = np.vstack([rng.uniform(0, 1, (4, D)), X[:1]])
    return X, y, ls, Xq, PT.draws(fam, N, D, S, F, seed + 1)


@pytest.mark.parametrize("fam", FAMS)
def test_truth_against_plain_numpy_double(fam):
    X, y, ls, Xq, dr = _small(fam)
    d = PT.sigma2(PT.NOISE)
    a = PT.evaluate(fam, 1.3, ls, d, X, y, dr, Xq, lin=PT.LD)
    b = PT.evaluate(fam, 1.3, ls, d, X, y, dr, Xq, lin=PT.F64, bounds=False)
    # two arithmetics on cond(K + d I) ~ 1e4 at most: double loses ~1e-12 of the targets' size in the solve
    scale = float(np.abs(a.r).max())
    for name in ("prior", "update", "dprior", "dupdate"):
        err = float(np.abs(getattr(a, name) - getattr(b, name)).max())
        ref = max(float(np.abs(getattr(a, name)).max()), scale)
        assert err <= 1e-9 * ref, (name, err, ref)


@pytest.mark.parametrize("fam", FAMS)
def test_gradient_against_central_differences_of_the_value(fam):
    X, y, ls, Xq, dr = _small(fam)
    Xq = Xq[:4]                                   # (the coincident row sits on the Exponential's kink: next test)
    d = PT.sigma2(PT.NOISE)
    a = PT.evaluate(fam, 1.3, ls, d, X, y, dr, Xq, bounds=False)
    e = T(2.0) ** -20
    for q in range(X.shape[1]):
        step = np.zeros(X.shape[1], dtype=T)
        step[q] = e
        up = PT.evaluate(fam, 1.3, ls, d, X, y, dr, np.asarray(Xq, dtype=T) + step, grad=False, bounds=False)
        dn = PT.evaluate(fam, 1.3, ls, d, X, y, dr, np.asarray(Xq, dtype=T) - step, grad=False, bounds=False)
        for part in ("prior", "update"):
            fd = (getattr(up, part) - getattr(dn, part)) / (2 * e)
            an = getattr(a, "d" + part)[:, :, q]
            # truncation e^2 |f'''| / 6 ~ 1e-12 x (a few hundred at these lengthscales)
            assert float(np.abs(fd - an).max()) <= 1e-8 * max(1.0, float(np.abs(an).max())), (part, q)


def test_exponential_gradient_skips_the_coincident_training_point():
    X, y, ls, Xq, dr = _small("Exponential")
    d = PT.sigma2(PT.NOISE)
    at = PT.evaluate("Exponential", 1.3, ls, d, X, y, dr, X[:1], bounds=False)
    V = at.V.copy()
    V[:, 0] = 0                                    # the same sum without the coincident term
    diff, r = PT._scaled_diff(np.asarray(X[:1], dtype=T), np.asarray(X, dtype=T), np.asarray(ls, dtype=T))
    G = np.where(r > 0, SR.dk_dr("Exponential", T(1.3), r) / np.where(r > 0, r, 1), 0)
    want = np.einsum("sn,mn,mnq->smq", V, G, diff) / np.asarray(ls, dtype=T)
    assert np.array_equal(at.dupdate, want)


@pytest.mark.parametrize("fam", FAMS)
def test_paths_interpolate_the_perturbed_data_whatever_F_is(fam):
    """f_s(X_i) = y_i - eps_si - d V_is: the prior term at X is Phi(X) w_s, the update K V_s = r_s - d V_s."""
    for F in (3, 30):
        X, y, ls, _, dr = _small(fam, F=F)
        d = PT.sigma2(PT.NOISE)
        a = PT.evaluate(fam, 1.3, ls, d, X, y, dr, X, grad=False, bounds=False)
        want = np.asarray(y, dtype=T)[None, :] - np.sqrt(T(d)) * np.asarray(dr[3], dtype=T) - T(d) * a.V
        # the truth's own rounding: cond(K + d I) <= N variance / d ~ 3e3 long-double ulp of the targets
        assert float(np.abs(a.prior + a.update - want).max()) <= 1e-14


@pytest.mark.parametrize("fam", FAMS)
def test_law_of_unit_frequencies(fam):
    """The mean of cos(omega^T delta) over 2^18 fixed-seed frequencies is within 4 / sqrt(2 F) of k(delta) / variance."""
    F, D = 2 ** 18, 3
    om = PP.unit_frequencies(fam, D, F, np.random.default_rng(2026))
    assert np.array_equal(om, PT.unit_frequencies(fam, D, F, np.random.default_rng(2026)))    # the truth's recipe is the module's
    deltas = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1], [1.0, 0.5, -0.7], [2.0, 1.5, 1.0], [0.0, 3.0, 0.0]])
    for dl in deltas:
        k = float(SR.k_of_r(fam, T(1.0), np.array([np.sqrt(T((dl * dl).sum()))], dtype=T))[0])
        got = float(np.cos(om @ dl).mean())
        assert abs(got - k) <= 4.0 / np.sqrt(2.0 * F), (fam, dl, got, k)


def test_kernel_id_and_draw_shapes():
    import gaussian_process_optimization_amd as gpo
    assert PP.kernel_id(gpo.kern.OU(2)) == PP.kernel_id("exponential") == 3
    assert PP.kernel_id(gpo.kern.ExpQuad(2)) == PP.kernel_id(0) == 0
    with pytest.raises(ValueError):
        PP.kernel_id("periodic")
    om, ph, w, z = PP.draw("Mat52", 11, 3, 4, 9, seed=1)
    assert om.shape == (9, 3) and ph.shape == (9,) and w.shape == (4, 9) and z.shape == (11, 4)[::-1]
    assert np.all((ph >= 0) & (ph < 2 * np.pi))
    again = PP.draw("Mat52", 11, 3, 4, 9, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip((om, ph, w, z), again))


LAW_SEED = 11     # chosen on the CPU: with it the truth alone passes for all four families


@pytest.mark.parametrize("fam", FAMS)
def test_law_of_the_paths(fam):
    """4096 fixed-seed paths of F = 4096 features at 5 locations: the empirical mean and covariance are within 5 standard errors
    of the oracle's posterior, plus the feature term's 4 / sqrt(2 F) variance."""
    N, D, S, F = 20, 2, 4096, 4096
    rng = np.random.default_rng(LAW_SEED)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(4 * X.sum(1)) + 0.1 * rng.standard_normal(N)
    ls = np.array([0.4, 0.7])
    Xq = rng.uniform(0, 1, (5, D))
    variance, noise = 1.3, 0.05
    d = PT.sigma2(noise)
    a = PT.evaluate(fam, variance, ls, d, X, y, PT.draws(fam, N, D, S, F, LAW_SEED + 1), Xq, lin=PT.F64, grad=False, bounds=False)
    f = (a.prior + a.update).astype(np.float64)                     # [S, 5]
    gp = O.OracleGP(X, y[:, None], KF.make(fam, D, variance, ls, True), noise)
    mu, C = gp.predict(Xq, full_cov=True, include_likelihood=False)
    mu, C = np.ravel(mu), np.asarray(C)
    feat = 4.0 / np.sqrt(2.0 * F) * variance
    sd = np.sqrt(np.diag(C))
    assert np.all(np.abs(f.mean(0) - mu) <= 5 * sd / np.sqrt(S) + feat), (f.mean(0) - mu, sd / np.sqrt(S))
    emp = np.cov(f.T, bias=True)
    se = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / S)
    assert np.all(np.abs(emp - C) <= 5 * se + feat), (np.abs(emp - C) / (5 * se + feat)).max()
