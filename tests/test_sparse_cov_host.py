"""Host side of the sparse model's joint posterior (no GPU).

* tests/_sparse_cov_ref.py: the long-double restatement of the full covariance against the float64 closed form and against the
  factored form ``Kss - U U^T + T T^T`` the device sums in, to 1e-12 of the largest entry.  "The largest entry" is that of the
  terms of the difference, K(Xs, Xs) -- the prior variance 1.3 on every run --, not of the result: the float64 closed form's worst
  own error on these runs is 6.1e-13 (S2 rbf ard, where the covariance's largest entry is 0.274: 2.2e-12 of THAT), an error of its
  woodbury_inv at cond(Kmm) 8.9e4 and the figure the bound was chosen over.  Both figures are printed.  The between-points
  restatement is held to the block of the stacked full covariance in long double, entry for entry.
* The condition the GPU suite's "no jitter step" rests on: per run the noiseless 130 x 130 covariance has a smallest eigenvalue
  >= 1e-7 (2.1e-7 on S5 rbf iso, >= 4.7e-5 elsewhere, against largest diagonals of 0.27 to 1.3) and numpy's Cholesky factors it.
* The Python layer -- ``SparseGPRegression`` (``full_cov``, ``posterior_samples_f``, ``posterior_covariance_between_points``),
  ``GPModel(sparse=True)`` and ``AcquisitionEntropySearch`` -- over a recording stand-in handle that answers from the float64
  oracle: call order, resident-set reuse, the transposes, the normaliser, and entropy search's block calls for a sparse model.
Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import entropy_search as E

import _sparse_ref as R
import _sparse_cov_ref as C
from test_gpu_sparse_gp import RUNS, IDS
from test_sparse_acq_host import _OracleHandle

JOINT = ("sparse_predict_full_cov", "sparse_posterior_samples", "sparse_cov_set_points", "sparse_cov_between")


# ---- the restatement and the runs' condition ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forms(case, fam, ard):
    X, Y, Z, Xs = R.case_inputs(case)
    ls = R.case_lengthscale(X.shape[1], ard)
    X1 = C.second_draw(case)
    out = {}
    for tag, lin in (("f64", R.F64), ("ld", R.LD)):
        f = R.inference(fam, X, Z, Y, R.VARIANCE, ls, ard, R.NOISE, lin, grads=False)
        mean, cov, var = C.full_cov(f, Z, Xs, R.NOISE, False, lin)
        out[tag] = dict(cov=cov, var=var, factored=C.factored(f, Z, Xs, lin), between=C.cov_between(f, Z, X1, Xs, lin),
                        stacked=C.full_cov(f, Z, np.vstack([X1[:9], Xs[:50]]), R.NOISE, False, lin)[1])
    return out


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - np.asarray(b, dtype=np.longdouble))))


@pytest.mark.parametrize("case,fam,ard", RUNS, ids=IDS)
def test_restatement_forms_and_the_runs_condition(case, fam, ard):
    r = _forms(case, fam, ard)
    ld, f64 = r["ld"], r["f64"]
    terms = R.VARIANCE                                           # the largest entry of K(Xs, Xs), the minuend
    figs = dict(closed64=_err(f64["cov"], ld["cov"]), factored_ld=_err(ld["factored"], ld["cov"]), factored64=_err(f64["factored"], ld["cov"]),
                diag=_err(np.diag(ld["cov"]), ld["var"]), block=_err(ld["stacked"][:9, 9:], ld["between"][:9, :50]))
    cov = np.asarray(ld["cov"], dtype=float)
    eig = np.linalg.eigvalsh(cov)
    print("%s %s %s: %s  (absolute; bound %.1e; the covariance's largest entry %.3g)  between64 %.2e  smallest eigenvalue %.3e"
          % (case, fam, "ard" if ard else "iso", "  ".join("%s %.2e" % kv for kv in figs.items()), 1e-12 * terms,
             np.max(np.abs(cov)), _err(f64["between"], ld["between"]), eig[0]))
    assert all(v <= 1e-12 * terms for v in figs.values()), figs
    assert figs["block"] == 0.0
    assert eig[0] >= 1e-7
    np.linalg.cholesky(cov)                                      # no jitter needed: a property of the inputs


# ---- the Python layer over a recording stand-in -----------------------------------------------------------------------------------------
class _JointHandle(_OracleHandle):
    """tests/test_sparse_acq_host.py's stand-in with the four joint-posterior methods, answered from tests/_sparse_cov_ref.py."""
    sparse_R = 0

    def sparse_predict_full_cov(self, Xs, include_noise=True):
        self.log.append("sparse_predict_full_cov")
        mean, cov, _ = C.full_cov(self.f, self.Z, Xs, self.par[4], include_noise, R.F64)
        return mean, cov

    def sparse_posterior_samples(self, Xs, Z, include_noise=False, maxtries=5):
        self.log.append("sparse_posterior_samples")
        mean, cov, _ = C.full_cov(self.f, self.Z, Xs, self.par[4], include_noise, R.F64)
        assert Z.shape[1] == Xs.shape[0]
        return mean, Z @ np.linalg.cholesky(cov).T, 0.0

    def sparse_cov_set_points(self, X2):
        self.log.append("sparse_cov_set_points")
        self.points = np.array(X2, dtype=float)
        self.sparse_R = self.points.shape[0]

    def sparse_cov_between(self, X1):
        self.log.append("sparse_cov_between")
        return C.cov_between(self.f, self.Z, X1, self.points, R.F64)


@pytest.fixture
def joint_handle(monkeypatch):
    monkeypatch.setattr(_lib, "Handle", _JointHandle)
    return _JointHandle


def _data(N=40, D=2, P=1, seed=5):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = 2.0 + 3.0 * np.sin(3 * X.sum(1))[:, None] * np.linspace(1.0, 0.5, P)[None, :] + 0.1 * rng.standard_normal((N, P))
    return X, Y


def _sparse(P=1, normalizer=None):
    X, Y = _data(P=P)
    m = gpo.models.SparseGPRegression(X, Y, kernel=gpo.kern.Matern52(2, variance=1.3, lengthscale=0.4), Z=X[:6].copy(),
                                      normalizer=normalizer)
    m.likelihood.variance.set(0.05)
    return m, X, Y


def _joint(m):
    return [c for c in m._h.log if c in JOINT]


def test_full_cov_and_the_normaliser(joint_handle):
    m, X, Y = _sparse(P=2, normalizer=True)
    Xn = np.random.RandomState(1).uniform(0, 1, (7, 2))
    raw_mean, raw_cov = m._raw_predict(Xn, full_cov=True)
    assert _joint(m) == ["sparse_predict_full_cov"] and raw_mean.shape == (7, 2) and raw_cov.shape == (7, 7)
    std, mu = np.asarray(m.normalizer.std, dtype=float), np.asarray(m.normalizer.mean, dtype=float)
    mean, cov = m.predict(Xn, full_cov=True)
    assert mean.shape == (7, 2) and cov.shape == (7, 7, 2)
    assert np.allclose(mean, raw_mean * std + mu, rtol=1e-14, atol=0)
    assert np.allclose(cov, (raw_cov + 0.05 * np.eye(7))[:, :, None] * std ** 2, rtol=1e-14, atol=0)       # inverse_covariance, noise in
    _, nl = m.predict_noiseless(Xn, full_cov=True)
    assert np.allclose(nl, raw_cov[:, :, None] * std ** 2, rtol=1e-14, atol=0)
    _, c1 = m.predict(Xn, full_cov=True, include_likelihood=False)
    assert np.array_equal(c1, nl)
    # one output: inverse_variance, a matrix
    m1, _, _ = _sparse(P=1, normalizer=True)
    mean, cov = m1.predict(Xn, full_cov=True)
    assert mean.shape == (7, 1) and cov.shape == (7, 7)
    # no locations: the shapes NumPy gives the reference
    e = m.predict(np.empty((0, 2)), full_cov=True)
    assert e[0].shape == (0, 2) and e[1].shape == (0, 0)
    with pytest.raises(ValueError, match="columns"):
        m.predict(np.zeros((3, 5)), full_cov=True)


def test_posterior_samples_f(joint_handle):
    m, X, Y = _sparse(P=2, normalizer=True)
    Xn = np.random.RandomState(2).uniform(0, 1, (5, 2))
    normals = np.random.RandomState(3).standard_normal((2, 4, 5))
    f1 = m.posterior_samples_f(Xn, size=4, normals=normals)
    assert _joint(m) == ["sparse_posterior_samples"] and f1.shape == (5, 2, 4) and m.posterior_samples_jitter_ == 0.0
    assert np.array_equal(f1, m.posterior_samples_f(Xn, size=4, normals=normals))
    raw_mean, raw_cov = m._raw_predict(Xn, full_cov=True)
    std, mu = np.asarray(m.normalizer.std, dtype=float), np.asarray(m.normalizer.mean, dtype=float)
    Cf = np.linalg.cholesky(raw_cov)
    for d in range(2):
        want = (raw_mean[:, d:d + 1] * std[d] + mu[d]) + (Cf @ normals[d].T) * std[d]      # the normaliser's std on the deviations
        assert np.allclose(f1[:, d, :], want, rtol=1e-12, atol=1e-14)
    np.random.seed(0)
    assert m.posterior_samples_f(Xn, size=3).shape == (5, 2, 3)


def test_between_points_resident_set_and_transpose(joint_handle):
    m, X, Y = _sparse()
    rng = np.random.RandomState(4)
    X1, X2 = rng.uniform(0, 1, (5, 2)), rng.uniform(0, 1, (3, 2))
    blk = m.posterior_covariance_between_points(X1, X2)
    assert _joint(m) == ["sparse_cov_set_points", "sparse_cov_between"]                   # X1 resident, X2 travels
    assert np.array_equal(m._h.points, X1) and blk.shape == (5, 3)
    _, stacked = m._raw_predict(np.vstack([X1, X2]), full_cov=True)
    assert np.allclose(blk, stacked[:5, 5:], rtol=0, atol=1e-13)                           # the block of the stacked covariance
    m._h.log[:] = []
    again = m.posterior_covariance_between_points(X1.copy(), X2[:1])                       # equal bit for bit: not uploaded again
    assert _joint(m) == ["sparse_cov_between"] and np.allclose(again, blk[:, :1], rtol=0, atol=1e-13)
    m.kern.lengthscale.set(0.5)                                                            # across a refit too
    m._h.log[:] = []
    moved = m.posterior_covariance_between_points(X1, X2)
    assert _joint(m) == ["sparse_cov_between"] and not np.array_equal(moved, blk)
    m._h.log[:] = []
    m.posterior_covariance_between_points(X1[:4], X2)                                      # another set: uploaded
    assert _joint(m) == ["sparse_cov_set_points", "sparse_cov_between"]
    assert m.posterior_covariance_between_points(X1[0], X2[0]).shape == (1, 1)


def test_gpmodel_front_door(joint_handle):
    X, Y = _data()
    np.random.seed(4)
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(2, variance=1.3, lengthscale=0.4), sparse=True, num_inducing=6, max_iters=0, verbose=False)
    gm.updateModel(X, Y, None, None)
    Xn = np.random.RandomState(6).uniform(0, 1, (4, 2))
    cov = gm.predict_covariance(Xn)
    _, want = gm.model.predict(Xn, full_cov=True)
    assert cov.shape == (4, 4) and np.array_equal(cov, np.maximum(want, 1e-10))
    noiseless = gm.predict_covariance(Xn, with_noise=False)
    assert np.all(np.diag(cov) > np.diag(noiseless))
    blk = gm.get_covariance_between_points(Xn, Xn[:2])
    assert blk.shape == (4, 2) and np.array_equal(blk, gm.model.posterior_covariance_between_points(Xn, Xn[:2]))


class _FixedSampler(E.McmcSampler):
    def __init__(self, space, points):
        super().__init__(space)
        self.points = points

    def get_samples(self, n_samples, log_p_function, burn_in_steps=50):
        pts = self.points[:n_samples]
        return pts, -0.5 * np.sum((pts - 0.5) ** 2, axis=1).reshape(-1, 1)


def test_entropy_search_scores_a_block_in_two_calls(joint_handle):
    X, Y = _data()
    np.random.seed(4)
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(2, variance=1.3, lengthscale=0.4), sparse=True, num_inducing=6, max_iters=0, verbose=False)
    gm.updateModel(X, Y, None, None)
    gm.model.likelihood.variance.set(0.05)
    space = gpo.Design_space([{"name": "x", "type": "continuous", "domain": (0.0, 1.0), "dimensionality": 2}])
    rng = np.random.RandomState(8)
    pts = rng.uniform(0, 1, (9, 2))
    es = gpo.AcquisitionEntropySearch(gm, space, _FixedSampler(space, pts), num_samples=15, num_representer_points=9)
    assert not es._es_device_ok()
    Xc = rng.uniform(0, 1, (7, 2))
    got = es.acquisition_function(Xc)
    h = gm.model._h
    # the belief: one predict and one full covariance of the representers; the block: ONE predict and ONE between-points call
    assert h.log.count("sparse_predict_full_cov") == 1 and h.log.count("sparse_cov_set_points") == 1
    assert h.log.count("sparse_cov_between") == 1 and h.log.count("sparse_predict") == 2
    assert np.array_equal(h.points, pts)
    # ... and the scores are the per-candidate arithmetic of the reference
    want = np.empty((7, 1))
    for j in range(7):
        row = Xc[[j]]
        _, sd = gm.predict(row, with_noise=False)
        want[j, 0] = -E.score(gm.get_covariance_between_points(es.repr_points, row) / sd, es.logP, es.repr_points_log, es.dlogPdMu, es._Q, es.W)
    fig = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("entropy search, block against per-candidate calls: %.2e" % fig)
    assert got.shape == (7, 1) and fig <= 1e-12
    h.log[:] = []
    es.acquisition_function(Xc[:3])                              # the representers stay resident
    assert [c for c in h.log if c in JOINT] == ["sparse_cov_between"]
