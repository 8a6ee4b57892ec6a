"""Host side of the sparse GP's restarts in lockstep (no GPU): the conditions of the members tests/test_gpu_sparse_batch.py runs,
asserted on the float64 reference of tests/_sparse_ref.py so that the GPU suite cannot quietly become a jitter lottery; and the
host logic -- ``SparseGPRegression._batch_objective`` / ``_lockstep_applies`` / ``optimize_restarts(parallel=True)``,
``GPModel(sparse=True, lockstep_restarts=...)`` -- over a NumPy stand-in handle answered by that reference.

Conditions (tests/_sparse_batch_cases.py): for every run of the sparse GPU suite's RUNS and all five members, cond(Kmm) inside the
sparse suite's cap of 8.9e4 -- the worst is 4.94e4 to the three digits it is quoted with (49415.5, S2 RBF ARD member 0), and the
test holds it to that figure at that precision -- and no step of either ladder; a lengthscale factor 1.1 on a perturbed
Z leaves the cap (S2 RBF: 1.2e6), which is why the members' factors are <= 1.  The stepped member (Z[1] = Z[0], variance 2^30) steps
the Kmm ladder exactly once, to 1e-6 x 2^30 = 1073.741824, with jitter_b = 0 and finite gradients, on S1 (all families) and S3 RBF;
with maxtries = 0 it fails.
Restarts: lockstep ends where the serial restarts end by the ``_compare_runs`` criterion of tests/test_gpu_fit_grad_batch.py (1e-8
relative per run, the same arg-min), consumes ``np.random`` as the serial loop does and makes no single-call evaluation during the
search.  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import sparse_gp as SG
from oracle import cpu_ref as O

import _sparse_ref as R
import _sparse_batch_cases as C

KID = {0: "rbf", 1: "Mat52", 2: "Mat32", 3: "Exponential"}


# ---- the members' conditions ------------------------------------------------------------------------------------------------------
def test_conditions_of_the_members():
    worst = (0.0, None)
    for case, fam, ard in C.RUNS:
        X, Y, Zs, var, lss, noise = C.members(case, ard)
        assert Zs.shape[0] == var.size == lss.shape[0] == noise.size == C.NMEMBERS
        for r in range(C.NMEMBERS):
            f = R.inference(fam, X, Zs[r], Y, var[r], lss[r], ard, noise[r], R.F64, grads=False)
            cond = float(np.linalg.cond(f["Kmm"]))
            if cond > worst[0]:
                worst = (cond, (case, fam, ard, r))
            print("%s %-12s ard=%d member %d cond(Kmm) %.3g  jitters %g %g" % (case, fam, ard, r, cond, f["jitter_kmm"], f["jitter_b"]))
            assert cond <= 8.9e4 and f["jitter_kmm"] == 0.0 and f["jitter_b"] == 0.0
    print("worst cond(Kmm) %.6g at %s" % worst)
    assert worst[1] == ("S2", "rbf", True, 0) and float("%.3g" % worst[0]) == 4.94e4
    # member 0 is the sparse suite's own run
    X, Y, Z, _ = R.case_inputs("S2")
    _, _, Zs, var, lss, noise = C.members("S2", True)
    assert np.array_equal(Zs[0], Z) and np.array_equal(lss[0], R.case_lengthscale(3, True))


def test_longer_lengthscales_leave_the_cap():
    X, Y, Zs, var, lss, noise = C.members("S2", True)
    f = R.inference("rbf", X, Zs[1], Y, var[1], 1.1 * R.case_lengthscale(3, True), True, noise[1], R.F64, grads=False)
    cond = float(np.linalg.cond(f["Kmm"]))
    print("S2 rbf, perturbed Z, lengthscale factor 1.1: cond(Kmm) %.3g" % cond)
    assert cond > 8.9e4


@pytest.mark.parametrize("case,fam,ard", [("S1", f, True) for f in C.FAMS] + [("S3", "rbf", False)])
def test_the_stepped_member_steps_once(case, fam, ard):
    X, Y, Zs, var, lss, noise = C.members(case, ard)
    Zs, var, lss, noise = C.with_stepped(Zs, var, lss, noise, slot=2)
    assert np.array_equal(Zs[2, 1], Zs[2, 0]) and var[2] == 2.0 ** 30
    f = R.inference(fam, X, Zs[2], Y, var[2], lss[2], ard, noise[2], R.F64)
    K = f["Kmm"]
    print("%s %s: Kmm[0,0] %.17g Kmm[1,1] %.17g Kmm[0,1] %.17g  jitters %.17g %g" % (case, fam, K[0, 0], K[1, 1], K[0, 1], f["jitter_kmm"],
                                                                                     f["jitter_b"]))
    assert K[0, 0] == K[0, 1] == K[1, 1] == 2.0 ** 30                # the 1e-8 is absorbed: the second pivot is exactly 0
    assert f["jitter_kmm"] == C.STEPPED_JITTER and f["jitter_b"] == 0.0
    for q in ("lml", "dvariance", "dlengthscale", "dnoise", "dZ"):
        assert np.all(np.isfinite(np.asarray(f[q], dtype=float))), q
    with pytest.raises(np.linalg.LinAlgError):
        O.jitchol(np.ascontiguousarray(K), maxtries=0)
    # the other members of the call stay unstepped
    for r in (0, 1, 3, 4):
        g = R.inference(fam, X, Zs[r], Y, var[r], lss[r], ard, noise[r], R.F64, grads=False)
        assert g["jitter_kmm"] == 0.0 and g["jitter_b"] == 0.0


# ---- host logic over a handle answered by the reference ---------------------------------------------------------------------------
class _RefHandle(object):
    """What SparseGPRegression asks of _lib.Handle, answered by tests/_sparse_ref.py in float64 (no device)."""
    calls = None
    bytes_per_member = 1000

    def __init__(self, device=0):
        self.device, self.h = device, object()

    def close(self):
        self.h = None

    def set_option(self, name, value):
        pass

    def set_gower(self, *a):
        assert not a

    def set_data(self, X, Y):
        self.X, self.Y = np.array(X, dtype=float), np.array(Y, dtype=float)
        self.N, self.D, self.P = X.shape[0], X.shape[1], Y.shape[1]

    def set_params(self, kernel, ard, variance, lengthscale, noise):
        self.par = (KID[kernel], float(variance), np.array(lengthscale, dtype=float), bool(ard), float(noise))
        self.n_ls = self.par[2].size

    def sparse_set_inducing(self, Z):
        self.Z = np.array(Z, dtype=float)
        self.Mz = self.Z.shape[0]

    def _fit(self, grads):
        fam, var, ls, ard, noise = self.par
        self.f = R.inference(fam, self.X, self.Z, self.Y, var, ls, ard, noise, R.F64, grads=grads)
        return self.f

    def sparse_fit(self, maxtries=5):
        type(self).calls["sparse_fit"] += 1
        f = self._fit(False)
        return float(f["lml"]), f["jitter_kmm"], f["jitter_b"]

    def sparse_fit_grad(self, nls, maxtries=5):
        type(self).calls["sparse_fit_grad"] += 1
        f = self._fit(True)
        return float(f["lml"]), (float(f["dvariance"]), f["dlengthscale"], float(f["dnoise"]), f["dZ"])

    def sparse_fit_grad_batch(self, Z, variances, lengthscales, noises, maxtries=5):
        type(self).calls["sparse_fit_grad_batch"] += 1
        fam, ard = self.par[0], self.par[3]
        k = len(variances)
        assert Z.shape == (k, Z.shape[1], self.D) and lengthscales.shape == (k, self.n_ls)
        lml, jk, jb, dv, dn = (np.full(k, np.nan) for _ in range(5))
        dl, dZ, status = np.full((k, self.n_ls), np.nan), np.full(Z.shape, np.nan), np.zeros(k, dtype=np.int32)
        for j in range(k):
            try:
                f = R.inference(fam, self.X, Z[j], self.Y, variances[j], lengthscales[j], ard, noises[j], R.F64)
            except np.linalg.LinAlgError:
                status[j] = 1
                continue
            lml[j], jk[j], jb[j], dv[j], dl[j], dn[j], dZ[j] = (f["lml"], f["jitter_kmm"], f["jitter_b"], f["dvariance"], f["dlengthscale"],
                                                               f["dnoise"], f["dZ"])
        return (lml, jk, jb), (dv, dl, dn, dZ), status

    def sparse_batch_bytes(self, R_, Mz):
        assert hasattr(self, "par")                     # the context holds data and parameters when it is asked
        return int(R_) * type(self).bytes_per_member

    def sparse_fmin(self):
        return float(R.fmin(self.f, self.X))


@pytest.fixture
def ref_handle(monkeypatch):
    monkeypatch.setattr(_lib, "Handle", _RefHandle)
    _RefHandle.calls = {"sparse_fit": 0, "sparse_fit_grad": 0, "sparse_fit_grad_batch": 0}
    _RefHandle.bytes_per_member = 1000
    return _RefHandle


def _data(seed=5, N=40, D=2):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    return X, Y


def _model(X, Y, seed=3):
    np.random.seed(seed)
    m = gpo.models.SparseGPRegression(X, Y, kernel=gpo.kern.Matern52(2, ARD=True), num_inducing=6)
    m.Gaussian_noise.constrain_bounded(1e-9, 1e6, warning=False)
    return m


def _compare_runs(rs, rp):
    assert len(rs) == len(rp)
    for (fs, _), (fp, _) in zip(rs, rp):
        print("serial %.12f  lockstep %.12f  relative %.2e" % (fs, fp, abs(fs - fp) / abs(fs)))
        assert abs(fs - fp) <= 1e-8 * abs(fs), (fs, fp)
    assert int(np.argmin([f for f, _ in rs])) == int(np.argmin([f for f, _ in rp]))


@pytest.mark.parametrize("restarts", [3, 4])
def test_lockstep_restarts_end_where_the_serial_ones_end(ref_handle, restarts):
    X, Y = _data()
    ms, mp = _model(X, Y), _model(X, Y)
    np.random.seed(77)
    rs = ms.optimize_restarts(restarts, verbose=False, max_iters=60)
    after_serial = np.random.uniform()
    serial_calls = dict(ref_handle.calls)
    for k in ref_handle.calls:
        ref_handle.calls[k] = 0
    np.random.seed(77)
    rp = mp.optimize_restarts(restarts, verbose=False, max_iters=60, parallel=True)
    after_lockstep = np.random.uniform()
    print("serial calls %s; lockstep calls %s" % (serial_calls, ref_handle.calls))
    _compare_runs(rs, rp)
    assert after_serial == after_lockstep                           # np.random consumed as the serial loop consumes it
    assert serial_calls["sparse_fit_grad"] >= restarts and serial_calls["sparse_fit_grad_batch"] == 0
    assert ref_handle.calls["sparse_fit_grad"] == 0 and ref_handle.calls["sparse_fit_grad_batch"] >= 1
    assert abs(ms.log_likelihood() - mp.log_likelihood()) <= 1e-8 * abs(ms.log_likelihood())


def test_batch_objective_is_obj_grad_per_row(ref_handle):
    """Z first, the transforms' chain rule (bounded noise), one batch call for all rows; a failed member is a wall."""
    X, Y = _data()
    m = _model(X, Y)
    x0 = m.optimizer_array.copy()
    rng = np.random.RandomState(0)
    xs = np.stack([x0 + 0.1 * rng.standard_normal(x0.size) for _ in range(3)])
    want = [m._obj_grad(x) for x in xs]
    before = ref_handle.calls["sparse_fit_grad_batch"]
    f, g = m._batch_objective(xs)
    assert ref_handle.calls["sparse_fit_grad_batch"] == before + 1
    for j in range(3):
        assert f[j] == want[j][0] and np.array_equal(g[j], want[j][1])
    # fixed noise: its entry leaves the optimiser vector
    m.Gaussian_noise.constrain_fixed(1e-6, warning=False)
    xs = xs[:, :-1]
    want = [m._obj_grad(x) for x in xs]
    f, g = m._batch_objective(xs)
    for j in range(3):
        assert f[j] == want[j][0] and np.array_equal(g[j], want[j][1]) and g[j].size == xs.shape[1]
    # a member whose ladders end without a factor
    orig = _RefHandle.sparse_fit_grad_batch

    def failing(self, *a, **k):
        out = orig(self, *a, **k)
        out[2][1] = 7
        return out

    _RefHandle.sparse_fit_grad_batch = failing
    try:
        f, g = m._batch_objective(xs)
    finally:
        _RefHandle.sparse_fit_grad_batch = orig
    assert f[1] == 1e10 and not np.any(g[1]) and f[0] == want[0][0] and f[2] == want[2][0]


def test_lockstep_applies_by_member_count_and_byte_budget(ref_handle, monkeypatch):
    X, Y = _data()
    m = _model(X, Y)
    assert m._lockstep_applies(1) and m._lockstep_applies(5) and m._lockstep_applies(64)
    assert not m._lockstep_applies(0) and not m._lockstep_applies(65)
    monkeypatch.setattr(SG, "BATCH_MAX_BYTES", 5000)
    assert m._lockstep_applies(5) and not m._lockstep_applies(6)     # 1000 bytes per member of the stand-in
    # past the budget the serial loop runs
    for k in ref_handle.calls:
        ref_handle.calls[k] = 0
    np.random.seed(1)
    runs = m.optimize_restarts(6, verbose=False, max_iters=3, parallel=True)
    assert len(runs) == 6 and ref_handle.calls["sparse_fit_grad_batch"] == 0 and ref_handle.calls["sparse_fit_grad"] >= 6


def test_gpmodel_forwards_the_flag(ref_handle):
    X, Y = _data()
    with pytest.raises(ValueError):
        gpo.GPModel(lockstep_restarts=True)
    with pytest.raises(ValueError):
        gpo.GPModel(sparse=True, parallel_restarts=True)              # the exact model's flag keeps raising
    seen = []
    for flag in (False, True):
        gm = gpo.GPModel(sparse=True, num_inducing=6, optimize_restarts=3, max_iters=4, verbose=False, lockstep_restarts=flag)
        assert gm.lockstep_restarts is flag
        np.random.seed(2)
        gm._create_model(X, Y)
        orig = gm.model.optimize_restarts

        def spy(*a, **k):
            seen.append(k.get("parallel", False))
            return orig(*a, **k)

        gm.model.optimize_restarts = spy
        for k in ref_handle.calls:
            ref_handle.calls[k] = 0
        gm.updateModel(X, Y, None, None)
        print("lockstep_restarts=%s: calls %s" % (flag, ref_handle.calls))
        assert (ref_handle.calls["sparse_fit_grad_batch"] >= 1) == flag
        assert (ref_handle.calls["sparse_fit_grad"] == 0) == flag
    assert seen == [False, True]
    # one restart: a single optimize, whatever the flag
    gm = gpo.GPModel(sparse=True, num_inducing=6, optimize_restarts=1, max_iters=2, verbose=False, lockstep_restarts=True)
    for k in ref_handle.calls:
        ref_handle.calls[k] = 0
    gm.updateModel(X, Y, None, None)
    assert ref_handle.calls["sparse_fit_grad_batch"] == 0
