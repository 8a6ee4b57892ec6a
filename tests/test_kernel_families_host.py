"""CPU: the host side of the Matern-3/2 / Exponential families -- the oracle helper's derivatives, the constants of the C header
against the binding, the kernel classes (ids, names, shapes, copy, pickle) and BayesianOptimization's kernel names."""
import os
import pickle
import re

import numpy as np
import pytest

import _kernel_families as KF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["Mat32", "Exponential"])
def test_helper_dk_dr_is_the_derivative_of_k_of_r(name):
    """dK_dr against a central difference of K_of_r in long double over r in [1e-3, 20], 1e-9 relative to |dK_dr|.
    Step h = 3e-7 (1 + r).  Truncation h^2 |k'''| / 6: for Matern-3/2 near r = 0, k''' ~ 6 sqrt3 variance against
    k' ~ -3 variance r, so 9e-14 * 1.7 / 1e-3 ~ 2e-10 at r = 1e-3, and |k''' / k'| <= 3 for large r (4e-11 * 3 / 6); for
    the Exponential h^2 / 6 <= 7e-12.  Rounding 2^-64 |k| / (h |k'|) <= 5e-20 * 1.3 / (3e-7 * 3.9e-3) ~ 6e-11 at r = 1e-3."""
    k = KF.make(name, 1, 1.3, [1.0], False)
    r = np.exp(np.linspace(np.log(1e-3), np.log(20.0), 400)).astype(np.longdouble)
    h = np.longdouble(3e-7) * (1 + r)
    fd = (k.K_of_r(r + h) - k.K_of_r(r - h)) / (2 * h)
    an = k.dK_dr(r)
    assert fd.dtype == np.longdouble and an.dtype == np.longdouble
    assert np.max(np.abs(fd - an) / np.abs(an)) <= 1e-9
    # float64 evaluation (what the oracle runs on) agrees with the long-double one to rounding
    r64 = r.astype(np.float64)
    assert np.max(np.abs(k.dK_dr(r64) - an) / np.abs(an)) <= 1e-14
    assert np.max(np.abs(k.K_of_r(r64) - k.K_of_r(r)) / np.abs(k.K_of_r(r))) <= 1e-14


@pytest.mark.parametrize("ard", [False, True], ids=["iso", "ard"])
@pytest.mark.parametrize("name", ["Mat32", "Exponential"])
def test_direct_distance_oracle_is_the_gram_trick_oracle_away_from_coincident_points(name, ard):
    """The two oracle variants on the problem of tests/test_gpu_kernel_families.py (N = 300, M = 130, Xs[0] = X[5]).  The Gram trick
    (stationary.py:155-173) loses ~ eps |x / l|^2 ~ 2e-15 in r^2, 1e-13 in r at the closest distinct pairs (r >= 0.01), amplified by
    at most |Ky^-1| ~ 1 / noise = 1e2: every output off the coincident candidate agrees to 1e-9 of its largest entry with two
    decades to spare.  AT the coincident candidate the Gram trick gives r ~ 1e-8, not 0; its effect there is reported, and is why
    the GPU tests take the direct variant wherever candidates are involved."""
    import test_gpu_kernel_families as T
    from oracle import cpu_ref as O
    X, Y, Xs, _ = T._problem()
    ls = T._ls(ard)
    gg = O.OracleGP(X, Y, KF.make(name, 3, T.VAR, ls, ard), T.NOISE)
    gd = O.OracleGP(X, Y, KF.make(name, 3, T.VAR, ls, ard, direct=True), T.NOISE)

    def rel(a, b):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    assert abs(gg.log_likelihood() - gd.log_likelihood()) <= 1e-12 * abs(gd.log_likelihood())
    assert rel(gg.kern.K(X), gd.kern.K(X)) <= 1e-12
    for a, b in zip(gg.gradients(), gd.gradients()):
        assert rel(np.atleast_1d(a), np.atleast_1d(b)) <= 1e-9
    (mg, vg), (md, vd) = gg.predict(Xs), gd.predict(Xs)
    (dmg, dvg), (dmd, dvd) = gg.predictive_gradients(Xs), gd.predictive_gradients(Xs)
    for what, a, b in (("mean", mg, md), ("var", vg, vd), ("dmdx", dmg, dmd), ("dvdx", dvg, dvd)):
        print("%s %s %-5s off the coincident row %.2e, on it %.2e" % (name, "ard" if ard else "iso", what, rel(a[1:], b[1:]),
                                                                     float(np.max(np.abs(a[0] - b[0])) / np.max(np.abs(b)))))
        assert rel(a[1:], b[1:]) <= 1e-9, what
    assert np.all(np.isfinite(dmd[0])) and np.all(np.isfinite(dvd[0]))


def test_header_and_binding_constants_agree():
    from gaussian_process_optimization_amd import _lib
    src = open(os.path.join(ROOT, "include", "gphip.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(GP_KERNEL_\w+)\s+(\d+)", src)}
    assert header == {"GP_KERNEL_RBF": 0, "GP_KERNEL_MATERN52": 1, "GP_KERNEL_MATERN32": 2, "GP_KERNEL_EXPONENTIAL": 3}
    for name, value in header.items():
        assert getattr(_lib, name) == value, name


CLASSES = [("Matern32", 2, "Mat32"), ("Exponential", 3, "Exponential"), ("OU", 3, "OU"), ("ExpQuad", 0, "ExpQuad")]


@pytest.mark.parametrize("cls,kid,default_name", CLASSES)
def test_new_classes_ids_names_shapes(cls, kid, default_name):
    import inspect
    import gaussian_process_optimization_amd as gpo
    C = getattr(gpo.kern, cls)
    assert list(inspect.signature(C.__init__).parameters)[1:] == ["input_dim", "variance", "lengthscale", "ARD", "active_dims", "name"]
    k = C(3)
    assert k._kernel_id == kid and k.name == default_name
    assert k.lengthscale.values.shape == (1,) and float(k.variance) == 1.0 and not k.ARD
    k = C(3, 1.3, [0.4, 0.7, 1.1], ARD=True)
    assert k.lengthscale.values.shape == (3,) and k.ARD and float(k.variance) == 1.3
    assert C(3, ARD=True).lengthscale.values.shape == (3,)
    assert C(3, lengthscale=0.5, ARD=True).lengthscale.values.tolist() == [0.5] * 3
    assert np.array_equal(k.Kdiag(np.zeros((5, 3))), np.full(5, 1.3))
    with pytest.raises(TypeError):
        C(3, Gower=True)
    with pytest.raises(TypeError):
        C(3, space=None)
    with pytest.raises(NotImplementedError):
        C(3, active_dims=[0, 2])


@pytest.mark.parametrize("cls,kid,default_name", CLASSES)
def test_new_classes_copy_and_pickle(cls, kid, default_name):
    import gaussian_process_optimization_amd as gpo
    C = getattr(gpo.kern, cls)
    k = C(3, 1.3, [0.4, 0.7, 1.1], ARD=True, name="mine")
    for twin in (k.copy(), pickle.loads(pickle.dumps(k))):
        assert type(twin) is C and twin is not k and twin._kernel_id == kid
        assert twin.name == "mine" and twin.ARD and twin.input_dim == 3
        assert float(twin.variance) == 1.3 and np.array_equal(twin.lengthscale.values, [0.4, 0.7, 1.1])
        assert twin.lengthscale.values is not k.lengthscale.values
    # the families that have the fork's Gower option keep it through copy()
    g = gpo.kern.Matern52(3, Gower=True, space=None).copy()
    assert g.Gower is True and type(g) is gpo.kern.Matern52


def test_bayesian_optimization_kernel_names():
    import gaussian_process_optimization_amd as gpo
    from gaussian_process_optimization_amd.bayesian_optimization import kernel_from_name
    want = {"RBF": gpo.kern.RBF, "ExpQuad": gpo.kern.ExpQuad, "Matern52": gpo.kern.Matern52, "Matern32": gpo.kern.Matern32,
            "Exponential": gpo.kern.Exponential, "OU": gpo.kern.OU}
    for name, C in want.items():
        k = kernel_from_name(name, 4, ARD=True)
        assert type(k) is C and k.input_dim == 4 and k.ARD and k.lengthscale.values.shape == (4,)
        assert not kernel_from_name(name, 4).ARD
    with pytest.raises(ValueError) as e:
        kernel_from_name("Matern12", 4)
    for name in want:
        assert name in str(e.value)


class _Recorder(object):
    """Stands in for _lib.Handle and refuses what the device refuses: Matern32 / Exponential while Gower is on, in either order."""

    def __init__(self):
        self.gower, self.kernel, self.calls = False, None, []

    def set_data(self, X, Y):
        self.N = X.shape[0]

    def set_params(self, kernel, ard, variance, lengthscale, noise):
        if self.gower and kernel in (2, 3):
            raise ValueError("gp_set_params after gp_set_gower")
        self.kernel = kernel
        self.calls.append("params")

    def set_gower(self, is_discrete=None, ranges=None):
        if is_discrete is not None and self.kernel in (2, 3):
            raise ValueError("gp_set_gower after gp_set_params")
        self.gower = is_discrete is not None
        self.calls.append("gower on" if self.gower else "gower off")

    def kernel_matrix(self):
        return np.zeros((self.N, self.N))


class _Space(object):
    def get_continuous_dims(self):
        return [0, 1, 2]

    def get_discrete_dims(self):
        return []

    def lengthscales(self):
        return [1.0, 1.0, 1.0]


def test_kern_K_orders_gower_and_parameters_on_the_shared_scratch_context(monkeypatch):
    """kern.K evaluates on ONE context per device: whatever an earlier kernel left there, the next one's calls must be accepted."""
    import gaussian_process_optimization_amd as gpo
    rec = _Recorder()
    monkeypatch.setattr(gpo.kern, "_scratch_handle", lambda device=0: rec)
    X = np.zeros((4, 3))
    for k in (gpo.kern.Matern52(3, Gower=True, space=_Space()), gpo.kern.Exponential(3), gpo.kern.RBF(3, Gower=True, space=_Space()),
              gpo.kern.Matern32(3), gpo.kern.OU(3), gpo.kern.Matern52(3), gpo.kern.RBF(3, Gower=True, space=_Space())):
        k.K(X)
    assert rec.calls[:4] == ["params", "gower on", "gower off", "params"]
