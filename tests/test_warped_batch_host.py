"""CPU: ``_batch_objective`` of ``InputWarpedGP`` and ``WarpedGP`` over a handle without a device (tests/_warped_batch_cases.py:
the oracle behind the single-member methods, the two batch methods a loop over them) agrees with ``_obj_grad`` on every row to
the last bit -- with a prior set, with the noise fixed (``exact_feval``) and with a member that fails (the wall, 1e10 with a zero
gradient) -- and the predicate of the lockstep route (``_lockstep_applies`` of ``InputWarpedGP``; ``_warp_lockstep_applies`` of
``WarpedGP``, whose ``_lockstep_applies`` -- the plain batch entry over shared targets -- stays False) keeps the plain model's size rule.  The restarts in lockstep draw ``np.random`` as the
serial loop does and end on its bits."""
import numpy as np
import pytest

import _warped_batch_cases as C


def _problem(N=26, D=2, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.exp(np.sin(5 * X).sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    return X, Y


def _input_warped(monkeypatch, fixed_noise=False, prior=False, ard=True):
    import gaussian_process_optimization_amd as gpo
    from gaussian_process_optimization_amd import _lib
    from gaussian_process_optimization_amd.input_warped_gp import InputWarpedGP
    from gaussian_process_optimization_amd.input_warping import LogGaussian
    monkeypatch.setattr(_lib, "Handle", C.BatchOverSingles)
    X, Y = _problem()
    m = InputWarpedGP(X, Y, kernel=gpo.kern.Matern52(2, variance=1.0, ARD=ard), Xmin=[0.0, 0.0], Xmax=[1.0, 1.0])
    m.Gaussian_noise.variance.set(0.05)
    if fixed_noise:
        m.Gaussian_noise.constrain_fixed(1e-6, warning=False)
    else:
        m.Gaussian_noise.constrain_bounded(1e-9, 1e6, warning=False)
    if prior:      # (the warping parameters carry their LogGaussian priors already: one more, on a kernel parameter)
        m.kern.variance.prior = LogGaussian(0.3, 1.2)
    return m


def _warped(monkeypatch, fixed_noise=False, prior=False, terms=2, warping_function=None):
    import gaussian_process_optimization_amd as gpo
    from gaussian_process_optimization_amd import _lib
    from gaussian_process_optimization_amd.input_warping import LogGaussian
    monkeypatch.setattr(_lib, "Handle", C.BatchOverSingles)
    X, Y = _problem(seed=6)
    m = gpo.models.WarpedGP(X, Y, kernel=gpo.kern.RBF(2, variance=1.0, ARD=True), warping_terms=terms,
                            warping_function=warping_function)
    m.Gaussian_noise.variance.set(0.05)
    if fixed_noise:
        m.Gaussian_noise.constrain_fixed(1e-6, warning=False)
    else:
        m.Gaussian_noise.constrain_positive(warning=False)
    if prior:
        m.kern.variance.prior = LogGaussian(0.3, 1.2)
        m.warping_function.d.prior = LogGaussian(0.0, 0.5)
    return m


MODELS = {"input_warped": _input_warped, "warped": _warped}
BATCH = {"input_warped": "fit_grad_x_batch", "warped": "fit_grad_warp_batch"}
SINGLE = {"input_warped": "fit_grad_x", "warped": "fit_grad_warp"}
APPLIES = {"input_warped": "_lockstep_applies", "warped": "_warp_lockstep_applies"}


def _rows(m, k, seed):
    rng = np.random.default_rng(seed)
    return m.optimizer_array[None, :] + 0.4 * rng.standard_normal((k, m.optimizer_array.size))


@pytest.mark.parametrize("which", ["input_warped", "warped"])
@pytest.mark.parametrize("fixed_noise,prior", [(False, False), (False, True), (True, False), (True, True)])
def test_batch_objective_is_obj_grad_on_every_row(monkeypatch, which, fixed_noise, prior):
    m = MODELS[which](monkeypatch, fixed_noise, prior)
    xs = _rows(m, 4, seed=11)
    m._push_params()      # (as the lockstep search does first: kernel family and ARD of the context the batch reads)
    f, g = m._batch_objective(xs)
    assert f.shape == (4,) and g.shape == xs.shape
    assert m._h.calls[BATCH[which]] == 1 and m._h.batch_sizes == [4] and m._h.calls[SINGLE[which]] == 0
    for j in range(4):
        fj, gj = m._obj_grad(xs[j])
        assert np.float64(fj).tobytes() == np.float64(f[j]).tobytes(), (j, fj, f[j])
        assert C.same_bits(gj, g[j]), (j, gj, g[j])
        assert np.all(np.isfinite(gj)) and np.any(gj != 0.0)
    assert m._h.calls[SINGLE[which]] == 4


@pytest.mark.parametrize("which", ["input_warped", "warped"])
def test_a_failed_member_is_the_wall(monkeypatch, which):
    m = MODELS[which](monkeypatch)
    xs = _rows(m, 3, seed=12)
    m.optimizer_array = xs[1]
    bad = float(m.kern.variance)
    m._h.fail_when = lambda v, ls, n: v == bad
    m.optimizer_array = xs[0]
    m._push_params()
    f, g = m._batch_objective(xs)
    assert f[1] == 1e10 and not g[1].any()
    for j in range(3):
        fj, gj = m._obj_grad(xs[j])           # the serial evaluation meets the same wall (LinAlgError -> 1e10, zeros)
        assert fj == f[j] and C.same_bits(gj, g[j])
    assert f[0] != 1e10 and f[2] != 1e10 and g[0].any() and g[2].any()


@pytest.mark.parametrize("which", ["input_warped", "warped"])
def test_the_batch_leaves_the_resident_data_alone(monkeypatch, which):
    m = MODELS[which](monkeypatch)
    m._ensure_fit()
    X0, Y0, warp0 = m._h.X.copy(), m._h.Yraw.copy(), m._h.warp
    sig = getattr(m, "_warp_signature", None)
    m._batch_objective(_rows(m, 3, seed=13))
    assert np.array_equal(m._h.X, X0) and np.array_equal(m._h.Yraw, Y0) and m._h.warp is warp0
    assert getattr(m, "_warp_signature", None) == sig


@pytest.mark.parametrize("which", ["input_warped", "warped"])
def test_lockstep_applies_by_the_plain_models_size_rule(monkeypatch, which):
    m = MODELS[which](monkeypatch)
    applies = getattr(m, APPLIES[which])
    assert applies(1) and applies(64) and not applies(65) and not applies(0)
    m.num_data = 2048
    assert applies(5)
    m.num_data = 2049
    assert not applies(5)


def test_identity_warp_keeps_the_serial_loop(monkeypatch):
    from gaussian_process_optimization_amd.warping_functions import IdentityFunction
    m = _warped(monkeypatch, warping_function=IdentityFunction())
    assert not m._warp_lockstep_applies(5) and not m._lockstep_applies(5)
    assert not _warped(monkeypatch)._lockstep_applies(5)      # the plain batch entry never applies to an output-warped model


@pytest.mark.parametrize("which", ["input_warped", "warped"])
def test_parallel_restarts_follow_the_serial_restarts(monkeypatch, which):
    ms, mp = MODELS[which](monkeypatch), MODELS[which](monkeypatch)
    np.random.seed(99)
    rs = ms.optimize_restarts(3, verbose=False, max_iters=25)
    state_s = np.random.get_state()
    np.random.seed(99)
    rp = mp.optimize_restarts(3, verbose=False, max_iters=25, parallel=True)
    state_p = np.random.get_state()
    assert state_s[0] == state_p[0] and np.array_equal(state_s[1], state_p[1]) and state_s[2:] == state_p[2:]
    assert len(rs) == len(rp) == 3
    for (fs, xs), (fp, xp) in zip(rs, rp):
        assert fs == fp and np.array_equal(xs, xp)
    assert np.array_equal(ms.optimizer_array, mp.optimizer_array) and ms.log_likelihood() == mp.log_likelihood()
    assert mp._h.calls[SINGLE[which]] == 0 and mp._h.calls[BATCH[which]] >= 1 and max(mp._h.batch_sizes) == 3
    assert ms._h.calls[BATCH[which]] == 0 and ms._h.calls[SINGLE[which]] > 0


def test_the_bo_models_forward_parallel_restarts(monkeypatch):
    import gaussian_process_optimization_amd as gpo
    from gaussian_process_optimization_amd import _lib
    monkeypatch.setattr(_lib, "Handle", C.BatchOverSingles)
    X, Y = _problem(N=18)
    space = gpo.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0.0, 1.0)},
                              {'name': 'y', 'type': 'continuous', 'domain': (0.0, 1.0)}])
    assert gpo.models.InputWarpedGPModel(space).parallel_restarts is False
    assert gpo.models.WarpedGPModel().parallel_restarts is False
    for flag in (False, True):
        gm = gpo.models.InputWarpedGPModel(space, optimize_restarts=3, max_iters=8, parallel_restarts=flag)
        np.random.seed(1)
        gm.updateModel(X, Y, None, None)
        assert (gm.model._h.calls["fit_grad_x_batch"] > 0) == flag and (gm.model._h.calls["fit_grad_x"] == 0) == flag
        wm = gpo.models.WarpedGPModel(optimize_restarts=3, max_iters=8, warping_terms=2, parallel_restarts=flag)
        np.random.seed(1)
        wm.updateModel(X, Y, None, None)
        assert (wm.model._h.calls["fit_grad_warp_batch"] > 0) == flag and (wm.model._h.calls["fit_grad_warp"] == 0) == flag


def test_null_contexts_are_argument_errors():
    from gaussian_process_optimization_amd import _lib
    lib = _lib.load_library()
    assert lib.gp_fit_grad_x_batch(None, 1, None, None, None, None, 5, None, None, None, None, None, None, None,
                                   None) == _lib.GP_ERR_ARG
    assert b"null" in lib.gp_last_error()
    assert lib.gp_fit_grad_warp_batch(None, 1, 1, None, None, None, None, None, 5, None, None, None, None, None, None, None, None,
                                      None, None) == _lib.GP_ERR_ARG
    assert b"null" in lib.gp_last_error()
