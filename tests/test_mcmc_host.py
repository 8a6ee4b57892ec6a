"""Host side of the MCMC surrogate (no GPU): the Gamma prior and the prior terms of the objective, the HMC sampler against the
independent restatement of tests/_hmc_ref.py, ``GPModel_MCMC`` over a handle answered by the oracle, and the front door.

Reference: GPy/GPy/core/parameterization/priors.py (Gamma), priorizable.py:49-82, GPy/GPy/inference/mcmc/hmc.py:20-68,
GPyOpt/GPyOpt/models/gpmodel.py:180-355, GPyOpt/GPyOpt/acquisitions/{EI,MPI,LCB}_mcmc.py.

Bounds.
* Gamma: closed form; the gradient against central differences of step 1e-6 at x in [0.3, 5]: truncation h^2 |f'''| / 6 <=
  1e-12 * 2 (a - 1) / x^3 / 6 (zero for a = 1), rounding 2^-52 |f| / h ~ 1e-9: bound 1e-8.
* HMC: the chains and the accept decisions must be identical to the bit.
* Leapfrog energy error: second order, so each halving of the step divides it by 4; asked: 3.5 .. 4.5.  The algorithm alone gives
  2.20e-3, 5.50e-4, 1.37e-4 at eps = 0.1, 0.05, 0.025 over two time units.
* Moments on N(0, diag(1, 4)), 2000 samples, eps = 0.1, 20 steps, first 200 dropped, seeds 0, 1, 2: |mean| <= 0.25 sigma, variance
  within 15 % (the algorithm alone in NumPy: means within 0.13 sigma, variances within 6 %).
Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib, priors
from gaussian_process_optimization_amd.mcmc import HMC
from gaussian_process_optimization_amd.parameterization import Logexp
from gaussian_process_optimization_amd.bayesian_optimization import InvalidConfigError
from oracle import cpu_ref as O

import _hmc_ref as R

KID = {0: "rbf", 1: "Mat52"}


# ---- Gamma prior -------------------------------------------------------------------------------------------------------------------
def test_gamma_from_EV_and_closed_form():
    g = priors.Gamma.from_EV(2., 4.)
    assert g.a == 1.0 and g.b == 0.5
    x = np.array([0.3, 1.0, 2.5, 5.0])
    ref = np.log(0.5) - 0.5 * x                       # a = 1: the exponential density with rate 0.5
    e = np.max(np.abs(g.lnpdf(x) - ref))
    print("lnpdf: %.2e" % e)
    assert e <= 4e-16
    g2 = priors.Gamma(3.0, 2.0)                         # ln p = 3 ln 2 - ln Gamma(3) + 2 ln x - 2 x
    ref2 = 3 * np.log(2.0) - np.log(2.0) + 2 * np.log(x) - 2 * x
    e2 = np.max(np.abs(g2.lnpdf(x) - ref2))
    print("lnpdf(3, 2): %.2e" % e2)
    assert e2 <= 1e-14


@pytest.mark.parametrize("a,b", [(1.0, 0.5), (3.0, 2.0), (0.7, 1.3)])
def test_gamma_gradient_against_central_differences(a, b):
    g = priors.Gamma(a, b)
    x, h = np.array([0.3, 1.0, 2.5, 5.0]), 1e-6
    num = (g.lnpdf(x + h) - g.lnpdf(x - h)) / (2 * h)
    e = np.max(np.abs(g.lnpdf_grad(x) - num))
    print("Gamma(%g, %g) gradient: %.2e" % (a, b, e))
    assert e <= 1e-8


class _OracleHandle(object):
    """What GPRegression and GPModel_MCMC ask of _lib.Handle, answered by oracle/cpu_ref.py in float64 (no device)."""
    log = []

    def __init__(self, device=0):
        self.device, self.h, self.ens = device, object(), None

    def close(self):
        self.h = None

    def set_option(self, name, value):
        pass

    def set_gower(self, *a):
        assert not a

    def set_data(self, X, Y):
        self.X, self.Y = np.array(X, dtype=float), np.array(Y, dtype=float)
        self.N, self.D, self.P = X.shape[0], X.shape[1], Y.shape[1]
        self.ens = None

    def set_params(self, kernel, ard, variance, lengthscale, noise):
        self.par = (kernel, bool(ard), float(variance), np.array(lengthscale, dtype=float), float(noise))
        self.n_ls = self.par[3].size

    def _gp(self, var=None, ls=None, noise=None):
        kernel, ard, v0, l0, n0 = self.par
        kern = O.make_kernel(KID[kernel], self.D, v0 if var is None else var, l0 if ls is None else ls, ARD=ard)
        return O.OracleGP(self.X, self.Y, kern, n0 if noise is None else noise)

    def fit(self, maxtries=5):
        p = self._gp().posterior
        return float(p["lml"]), float(p["logdet"]), float(p["jitter"])

    def fit_grad(self, nls, maxtries=5):
        gp = self._gp()
        p = gp.posterior
        dv, dl, dn = gp.gradients()
        type(self).log.append("fit_grad")
        return (float(p["lml"]), float(p["logdet"]), float(p["jitter"])), (float(dv), np.atleast_1d(dl), float(dn))

    def lml_grad(self, nls):
        dv, dl, dn = self._gp().gradients()
        return float(dv), np.atleast_1d(dl), float(dn)

    def ens_fit(self, variances, lengthscales, noises, maxtries=5):
        type(self).log.append(("ens_fit", np.array(variances), np.array(lengthscales), np.array(noises), self.par))
        self.ens = [self._gp(v, l, n) for v, l, n in zip(variances, lengthscales, noises)]
        S = len(self.ens)
        fmin = np.array([g.predict(self.X)[0].min() for g in self.ens])
        return (np.array([float(g.posterior["lml"]) for g in self.ens]), np.zeros(S), np.zeros(S), fmin)

    def ens_predict_rows(self, Xs, include_noise=True, grad=False):
        assert Xs.shape[0] <= 8
        mu = np.stack([g.predict(Xs, include_likelihood=include_noise)[0][:, 0] for g in self.ens])
        var = np.stack([g.predict(Xs, include_likelihood=include_noise)[1][:, 0] for g in self.ens])
        if not grad:
            return mu, var
        gr = [g.predictive_gradients(Xs) for g in self.ens]
        return mu, var, np.stack([a[:, :, 0] for a, _ in gr]), np.stack([b for _, b in gr])


@pytest.fixture
def oracle_handle(monkeypatch):
    monkeypatch.setattr(_lib, "Handle", _OracleHandle)
    _OracleHandle.log = []
    return _OracleHandle


def _data(N=12, D=2, seed=3):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    return X, Y


def test_log_prior_with_logexp_jacobians(oracle_handle):
    X, Y = _data()
    m = gpo.models.GPRegression(X, Y, gpo.kern.RBF(2, variance=1.7, lengthscale=0.6), noise_var=0.05)
    assert m.log_prior() == 0.0 and np.all(m._log_prior_gradients() == 0.)
    g = priors.Gamma(3.0, 2.0)
    m.kern.set_prior(g)
    m.likelihood.variance.set_prior(priors.Gamma.from_EV(2., 4.))
    vals = np.array([1.7, 0.6, 0.05])
    # priorizable.py:49-65: sum ln p(theta) + sum ln |d theta / d x| of the Logexp transform, ln(1 - exp(-theta))
    ref = g.lnpdf(vals[:2]).sum() + (np.log(0.5) - 0.5 * 0.05) + np.log(-np.expm1(-vals)).sum()
    print("log_prior: %.17g against %.17g" % (m.log_prior(), ref))
    assert abs(m.log_prior() - ref) <= 1e-14 * abs(ref)
    # priorizable.py:67-82: ln p' + d/d theta ln(1 - exp(-theta)) = 1 / (exp(theta) - 1)
    gref = np.r_[g.lnpdf_grad(vals[:2]), -0.5] + 1.0 / np.expm1(vals)
    e = np.max(np.abs(m._log_prior_gradients() - gref))
    print("log_prior gradients: %.2e" % e)
    assert e <= 1e-14 * np.max(np.abs(gref))
    # the transform's own pair, against central differences (bound as for the Gamma's gradient)
    t, h = Logexp(), 1e-6
    num = (t.log_jacobian(vals + h) - t.log_jacobian(vals - h)) / (2 * h)
    e = np.max(np.abs(t.log_jacobian_grad(vals) - num) / np.abs(num))
    print("Logexp.log_jacobian_grad: %.2e" % e)
    assert e <= 1e-8
    assert np.array_equal(m.unfixed_param_array, vals)
    m.Gaussian_noise.constrain_fixed(1e-6)
    assert np.array_equal(m.unfixed_param_array, vals[:2])


def test_objective_bits_unchanged_without_priors_and_shifted_with(oracle_handle):
    X, Y = _data()
    m = gpo.models.GPRegression(X, Y, gpo.kern.RBF(2, variance=1.7, lengthscale=0.6), noise_var=0.05)
    f0, g0 = m.objective_function(), m.objective_function_gradients()
    assert f0 == -float(m.log_likelihood())
    nat = m._log_likelihood_gradients_natural()
    assert np.array_equal(g0, -m._transform_gradients(nat))            # the expression of the code without priors: the same bits
    m.kern.set_prior(priors.Gamma.from_EV(2., 4.))
    m.likelihood.variance.set_prior(priors.Gamma.from_EV(2., 4.))
    f1, g1 = m.objective_function(), m.objective_function_gradients()
    assert f1 == f0 - m.log_prior()
    x, h = m.optimizer_array.copy(), 1e-6
    num = np.empty_like(x)
    for i in range(x.size):
        e = np.zeros_like(x)
        e[i] = h
        m.optimizer_array = x + e
        fp = m.objective_function()
        m.optimizer_array = x - e
        num[i] = (fp - m.objective_function()) / (2 * h)
    m.optimizer_array = x
    err = np.max(np.abs(g1 - num) / np.maximum(np.abs(num), 1.0))
    print("objective gradient with priors against central differences: %.2e" % err)
    assert err <= 1e-6           # h^2 f''' / 6 ~ 1e-11 and 2^-52 |f| / h ~ 1e-8 at |f| ~ 20
    m.unset_priors()      # (the parameters went through the transform and back: compare at the values they have now)
    assert m.objective_function() == -float(m.log_likelihood())
    assert np.array_equal(m.objective_function_gradients(), -m._transform_gradients(m._log_likelihood_gradients_natural()))


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [None, np.array([[2.0, 0.3], [0.3, 0.5]])])
def test_hmc_chain_is_the_restatements_bit_for_bit(mass):
    var, x0 = np.array([1.0, 4.0]), np.array([0.7, -1.1])
    model = R.Quadratic(x0, var)
    np.random.seed(11)
    s = HMC(model, M=mass, stepsize=0.17)
    got = s.sample(num_samples=60, hmc_iters=7)
    np.random.seed(11)
    ref, accepts = R.chain(x0, model.U, model.grad_U, 60, 0.17, 7, M=mass)
    print("accepted %d of 60" % sum(accepts))
    assert 0 < sum(accepts) and np.array_equal(got, ref)
    assert s.accepted == accepts
    assert model.gradient_calls == 60 * 7 * 2


def test_rejection_repeats_the_state_before_the_trajectory():
    """A step far too large for the narrow direction: most proposals are rejected, and row i is then the state row i - 1 ended in."""
    var, x0 = np.array([1.0, 1e-4]), np.array([0.5, 0.01])
    model = R.Quadratic(x0, var)
    np.random.seed(5)
    s = HMC(model, stepsize=0.05)
    got = s.sample(num_samples=40, hmc_iters=5)
    np.random.seed(5)
    ref, accepts = R.chain(x0, model.U, model.grad_U, 40, 0.05, 5)
    assert np.array_equal(got, ref) and s.accepted == accepts
    print("accepted %d of 40" % sum(accepts))
    assert sum(accepts) < 40
    for i in range(1, 40):
        if not accepts[i]:
            assert np.array_equal(got[i], got[i - 1])


def test_leapfrog_energy_error_is_second_order():
    var, x0, p0 = np.array([1.0, 4.0]), np.array([0.7, -1.1]), np.array([0.4, 0.9])
    errs = []
    for eps in (0.1, 0.05, 0.025):
        model = R.Quadratic(x0, var)
        s = HMC(model, stepsize=eps)
        s.p[:] = p0
        H0 = s._computeH()
        s._update(int(round(2.0 / eps)))
        errs.append(abs(s._computeH() - H0))
    print("energy errors: %.3e %.3e %.3e; ratios %.2f %.2f" % (errs[0], errs[1], errs[2], errs[0] / errs[1], errs[1] / errs[2]))
    assert 3.5 <= errs[0] / errs[1] <= 4.5 and 3.5 <= errs[1] / errs[2] <= 4.5


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sample_moments(seed):
    var = np.array([1.0, 4.0])
    model = R.Quadratic(np.zeros(2), var)
    np.random.seed(seed)
    ss = HMC(model, stepsize=0.1).sample(num_samples=2000, hmc_iters=20)[200:]
    mean, v = ss.mean(0), ss.var(0)
    print("seed %d: mean / sigma %s, variance ratio %s" % (seed, mean / np.sqrt(var), v / var))
    assert np.all(np.abs(mean) <= 0.25 * np.sqrt(var)) and np.all(np.abs(v / var - 1.0) <= 0.15)


# ---- GPModel_MCMC over the oracle's handle -----------------------------------------------------------------------------------------
class _Recorder(object):
    """np.random's draws, in order, while the model updates."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("randn", "multivariate_normal", "rand"):
            real = getattr(np.random, name)
            monkeypatch.setattr(np.random, name, self._wrap(name, real))

    def _wrap(self, name, real):
        def f(*a, **k):
            self.calls.append(name)
            if name == "randn":
                self.mark = len(_OracleHandle.log)       # what the handle had been asked before the chain started
            return real(*a, **k)
        return f


@pytest.mark.parametrize("exact", [False, True])
def test_gpmodel_mcmc_update(oracle_handle, monkeypatch, exact):
    X, Y = _data()
    rec = _Recorder(monkeypatch)
    np.random.seed(4)
    mm = gpo.GPModel_MCMC(exact_feval=exact, n_samples=3, n_burnin=5, subsample_interval=2, leapfrog_steps=3)
    assert mm.MCMC_sampler and mm.analytical_gradient_prediction and gpo.models.GPModel_MCMC is gpo.GPModel_MCMC
    mm.updateModel(X, Y, None, None)
    gp = mm.model
    # defaults: RBF with variance 1 at creation, noise 1 % of Var(Y), Gamma(1, 0.5) priors everywhere
    assert type(gp.kern).__name__ == "RBF" and all(p.prior.a == 1.0 and p.prior.b == 0.5 for p in gp.flattened_parameters())
    assert gp.likelihood.variance.is_fixed == exact
    # the draws: ONE randn for the perturbation, then (multivariate_normal, rand) per sample
    total = 5 + 3 * 2
    assert rec.calls == ["randn"] + ["multivariate_normal", "rand"] * total
    assert mm.hmc.accepted and len(mm.hmc.accepted) == total
    # the thinning
    assert mm.hmc_samples.shape == (3, 2 if exact else 3)
    # what reached ens_fit: the thinned samples, column by column; the handle's parameters name family and ARD
    tag, var, ls, noise, par = [e for e in oracle_handle.log if not isinstance(e, str)][-1]
    assert tag == "ens_fit" and par[0] == 0 and par[1] is False
    assert np.array_equal(var, mm.hmc_samples[:, 0]) and np.array_equal(ls[:, 0], mm.hmc_samples[:, 1])
    if exact:
        assert np.all(noise == float(gp.likelihood.variance)) and abs(noise[0] - 1e-6) <= 1e-7   # fixed at 1e-6, then perturbed by 1 %
    else:
        assert np.array_equal(noise, mm.hmc_samples[:, 2])
    # the chain's device calls: ONE fit_grad per leapfrog position (the half step that ends a leapfrog step and the one that
    # begins the next share their point, and so do the trajectory's ends and the energies taken there), nothing else
    during = oracle_handle.log[rec.mark:-1]
    assert during.count("fit_grad") == len(during) and total * 3 <= len(during) <= total * 3 + total + 1
    # the list-shaped returns
    Xs = np.random.RandomState(0).uniform(0, 1, (11, 2))
    means, stds = mm.predict(Xs)
    assert len(means) == len(stds) == 3 and all(a.shape == (11, 1) for a in means + stds)
    m2, s2, dm, ds = mm.predict_withGradients(Xs)
    assert all(np.array_equal(a, b) for a, b in zip(means + stds, m2 + s2)) and all(a.shape == (11, 2) for a in dm + ds)
    fmins = mm.get_fmin()
    assert isinstance(fmins, list) and len(fmins) == 3
    for z in range(3):
        g = gp._h.ens[z]
        mu, v = g.predict(Xs)
        # (the model asks for eight rows per call, the check for all eleven at once: BLAS blocks the two differently)
        assert np.allclose(means[z], mu, rtol=0, atol=1e-12) and np.allclose(stds[z], np.sqrt(np.clip(v, 1e-10, np.inf)), rtol=0, atol=1e-12)
        assert np.allclose(ds[z], g.predictive_gradients(Xs)[1] / (2 * stds[z]), rtol=0, atol=1e-10)
        assert fmins[z] == g.predict(X)[0].min()
    assert mm.get_model_parameters().shape == (1, 3) and len(mm.get_model_parameters_names()) == 3
    # the integrated acquisitions on the host route (a constraint-free space with a cost switches the device route off)
    for cls, kw in ((gpo.AcquisitionEI_MCMC, {}), (gpo.AcquisitionMPI_MCMC, {}), (gpo.AcquisitionLCB_MCMC, {})):
        acq = cls(mm, **kw)
        acq.cost_withGradients = lambda x: (np.ones((x.shape[0], 1)), np.zeros(x.shape))
        val, dval = acq.acquisition_function_withGradients(Xs[:3])
        ref = 0
        for z in range(3):
            ref = ref + acq._rule.value(acq._par(), fmins[z], means[z][:3].copy(), stds[z][:3].copy())
        assert np.allclose(val, -ref / 3, rtol=0, atol=1e-12 * np.max(np.abs(ref))) and dval.shape == (3, 2)   # (BLAS blocking, as above)
        assert np.array_equal(acq.acquisition_function(Xs[:3]), val)


def test_copy_is_a_working_mcmc_model(oracle_handle):
    X, Y = _data()
    np.random.seed(1)
    mm = gpo.GPModel_MCMC(n_samples=2, n_burnin=1, subsample_interval=1, leapfrog_steps=2)
    mm.updateModel(X, Y, None, None)
    twin = mm.copy()
    assert isinstance(twin, gpo.GPModel_MCMC) and twin.hmc_samples.shape == (2, 3) and len(twin.get_fmin()) == 2


# ---- the front door ------------------------------------------------------------------------------------------------------------------
_DOMAIN = [{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}]


def test_front_door(oracle_handle):
    X, Y = _data()
    for name, cls in (("EI_MCMC", gpo.AcquisitionEI_MCMC), ("MPI_MCMC", gpo.AcquisitionMPI_MCMC), ("LCB_MCMC", gpo.AcquisitionLCB_MCMC)):
        bo = gpo.BayesianOptimization(None, _DOMAIN, X=X, Y=Y, model=gpo.GPModel_MCMC(n_samples=2), acquisition_type=name)
        assert isinstance(bo.acquisition, cls) and bo.acquisition.analytical_gradient_acq
    with pytest.raises(InvalidConfigError):
        gpo.BayesianOptimization(None, _DOMAIN, X=X, Y=Y, model=gpo.GPModel(), acquisition_type='EI_MCMC')
    with pytest.raises(InvalidConfigError):
        gpo.BayesianOptimization(None, _DOMAIN, X=X, Y=Y, acquisition_type='EI_MCMC')
    with pytest.raises(InvalidConfigError):
        gpo.BayesianOptimization(None, _DOMAIN, X=X, Y=Y, model=gpo.GPModel_MCMC(), acquisition_type='EI')
    with pytest.raises(NotImplementedError):
        gpo.BayesianOptimization(None, _DOMAIN, X=X, Y=Y, model_type='GP_MCMC')
    for ev in ('local_penalization', 'thompson_sampling'):
        with pytest.raises(NotImplementedError):
            gpo.BayesianOptimization(None, _DOMAIN, X=X, Y=Y, model=gpo.GPModel_MCMC(), acquisition_type='EI_MCMC',
                                     evaluator_type=ev, batch_size=2)
    gpo.BayesianOptimization(None, _DOMAIN, X=X, Y=Y, model=gpo.GPModel_MCMC(), acquisition_type='EI_MCMC', evaluator_type='random',
                             batch_size=2)
    with pytest.raises(AssertionError):
        gpo.AcquisitionEI_MCMC(gpo.GPModel())
