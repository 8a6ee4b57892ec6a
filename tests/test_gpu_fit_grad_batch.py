"""GPU: gp_fit_grad_batch -- R members against gp_fit_grad one at a time, against the oracle, per-member jitter, the Gower
set-up, the untouched resident fit, the size limits, and optimize_restarts(parallel=True) against the serial restarts."""
import ctypes
import json
import os

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd.kern import gower_config
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h():
    hh = _lib.Handle(0)
    yield hh
    hh.close()


def _data(N, D, P, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.stack([np.sin(2 * np.pi * (p + 1) * X).sum(1) / np.sqrt(D) + 0.1 * rng.standard_normal(N) for p in range(P)], 1)
    return X, Y


def _members(R, D, ard, seed):
    """Parameters spread over three decades."""
    rng = np.random.default_rng(seed)
    nls = D if ard else 1
    var = 10.0 ** rng.uniform(-1.5, 1.5, R)
    ls = np.sqrt(D) * 10.0 ** rng.uniform(-1.2, 0.3, (R, nls))
    noise = 10.0 ** rng.uniform(-4.0, -1.0, R)
    return var, ls, noise


def _single(h, kernel, ard, var, ls, noise, maxtries=5):
    h.set_params(kernel, ard, var, ls, noise)
    try:
        (lml, logdet, jit), (dv, dl, dn) = h.fit_grad(ls.size, maxtries)
    except np.linalg.LinAlgError:
        return None
    return np.r_[lml, logdet, jit, dv, dl, dn]


def _batch_rows(res, r):
    (lml, logdet, jit), (dv, dl, dn), _ = res
    return np.r_[lml[r], logdet[r], jit[r], dv[r], dl[r], dn[r]]


def _close(a, b, rtol=1e-12):
    """lml, log det and jitter within rtol relative; the gradient entries within rtol of the member's largest one."""
    head = np.all(np.abs(a[:3] - b[:3]) <= rtol * np.abs(b[:3]))
    return bool(head and np.max(np.abs(a[3:] - b[3:])) <= rtol * np.max(np.abs(b[3:])))


CASES = [  # (N, kernel, ard, D, P, R)
    (1, 0, False, 1, 1, 2), (2, 1, True, 3, 1, 5), (64, 0, True, 8, 3, 16), (64, 1, False, 3, 1, 64),
    (127, 1, True, 1, 1, 5), (128, 0, False, 1, 3, 2), (129, 1, True, 3, 1, 16), (300, 0, True, 8, 1, 5),
    (300, 1, True, 8, 3, 1), (1000, 1, True, 3, 1, 5), (1000, 0, False, 3, 3, 2), (2048, 1, True, 8, 1, 5),
    (2048, 0, False, 1, 1, 16), (300, 1, False, 1, 1, 64),
]


@pytest.mark.parametrize("N,kernel,ard,D,P,R", CASES)
def test_members_equal_the_single_call(h, N, kernel, ard, D, P, R):
    X, Y = _data(N, D, P, seed=N + D)
    h.set_data(X, Y)
    var, ls, noise = _members(R, D, ard, seed=R + N)
    h.set_params(kernel, ard, var[0], ls[0], noise[0])
    res = h.fit_grad_batch(var, ls, noise)
    status = res[2]
    exact = 0
    for r in range(R):
        ref = _single(h, kernel, ard, var[r], ls[r], noise[r])
        if ref is None:
            assert status[r] > 0
            continue
        assert status[r] == 0, r
        got = _batch_rows(res, r)
        assert got[2] == ref[2], (r, got[2], ref[2])       # the same rung of the jitter ladder
        assert _close(got, ref), (r, got, ref)
        exact += int(np.array_equal(got, ref))
    if -(-N // 128) * 128 <= 768:   # below one panel gp_fit_grad takes the single-stream route the batch mirrors: the same bits
        assert exact == int(np.sum(status == 0)), (exact, R)


@pytest.mark.parametrize("kernel,ard,D", [(0, False, 2), (1, True, 5)])
def test_members_against_the_oracle(h, kernel, ard, D):
    X, Y = _data(200, D, 1, seed=3)
    h.set_data(X, Y)
    var, ls, noise = _members(4, D, ard, seed=17)
    noise = np.maximum(noise, 1e-2)
    h.set_params(kernel, ard, var[0], ls[0], noise[0])
    (lml, logdet, _), (dv, dl, dn), st = h.fit_grad_batch(var, ls, noise)
    assert not st.any()
    for r in range(4):
        kern = O.make_kernel("rbf" if kernel == 0 else "Mat52", D, var[r], ls[r], ARD=ard)
        gp = O.OracleGP(X, Y, kern, noise[r])
        dv0, dl0, dn0 = gp.gradients()
        assert abs(lml[r] - gp.log_likelihood()) <= 1e-8 * abs(gp.log_likelihood())
        scale = max(abs(dv0), float(np.max(np.abs(dl0))), 1.0)
        assert abs(dv[r] - dv0) < 1e-6 * scale and np.max(np.abs(dl[r] - dl0)) < 1e-6 * scale
        assert abs(dn[r] - dn0) < 1e-6 * max(abs(dn0), 1.0)


def test_jitter_per_member(h):
    X, Y = _data(120, 2, 1, seed=5)
    X = np.vstack([X, X[:40]])                       # duplicated rows: with a large variance and no noise K + 1e-8 is not PD
    Y = np.vstack([Y, Y[:40]])
    h.set_data(X, Y)
    R = 6
    var = np.array([1.0, 1e8, 1.0, 1e7, 1.0, 1e8])
    ls = np.array([[0.3], [2.0], [0.3], [1.5], [0.25], [1.0]])
    noise = np.array([1e-2, 1e-12, 1e-3, 1e-12, 1e-2, 1e-12])
    h.set_params(0, False, var[0], ls[0], noise[0])
    res = h.fit_grad_batch(var, ls, noise)
    jit = res[0][2]
    for r in range(R):
        ref = _single(h, 0, False, var[r], ls[r], noise[r])
        assert ref is not None and res[2][r] == 0
        assert jit[r] == ref[2]
        assert _close(_batch_rows(res, r), ref)
        if noise[r] > 1e-6:
            assert jit[r] == 0.0 and np.array_equal(_batch_rows(res, r), ref)   # the well-conditioned members: untouched, bitwise
    assert np.any(jit > 0) and np.all(jit[noise > 1e-6] == 0)
    # with no retries allowed, exactly the members that needed jitter fail -- alone, with gp_fit_grad's code
    res0 = h.fit_grad_batch(var, ls, noise, maxtries=0)
    st = res0[2]
    assert np.array_equal(st != 0, jit > 0)
    for r in range(R):
        if st[r]:
            h.set_params(0, False, var[r], ls[r], noise[r])
            with pytest.raises(np.linalg.LinAlgError):
                h.fit_grad(1, 0)
            assert np.isnan(res0[0][0][r])
        else:
            assert np.array_equal(_batch_rows(res0, r), _batch_rows(res, r))


def test_jitter_per_member_later_tile(h):
    """The same over three tiles (tests/_jitter_cases.py: N = 300, rows 260 .. 299 repeat rows 0 .. 39): the members of
    test_jitter_per_member, whose hard ones give way in the first tile and carry what is left through two more, and two members
    whose first non-positive pivot lies among the repeated rows -- in the third tile of potrf_tile_batch_kernel, with a
    per-member info.  tests/test_jitter_cases_host.py checks on the CPU that the hard members fail un-jittered, and where."""
    import _jitter_cases as J
    X, Y = J.batch_problem()
    h.set_data(X, Y)
    var, ls, noise = J.BATCH_VAR, J.BATCH_LS, J.BATCH_NOISE
    R = var.size
    h.set_params(0, False, var[0], ls[0], noise[0])
    res = h.fit_grad_batch(var, ls, noise)
    jit = res[0][2]
    for r in range(R):
        ref = _single(h, 0, False, var[r], ls[r], noise[r])
        assert ref is not None and res[2][r] == 0
        assert jit[r] == ref[2]
        assert np.array_equal(_batch_rows(res, r), ref), (r, _batch_rows(res, r), ref)   # Npad = 384 <= 768: the same bits
        if noise[r] > 1e-6:
            assert jit[r] == 0.0
    assert np.all(jit[noise < 1e-6] > 0) and np.all(jit[noise > 1e-6] == 0)
    for r in J.BATCH_THIRD_TILE:          # the first rung, nine orders above the rounding that decided the failure
        assert jit[r] == pytest.approx((var[r] + (noise[r] + 1e-8)) * 1e-6, rel=1e-12)
    # with no retries allowed, exactly the members that needed jitter fail -- alone, with gp_fit_grad's code
    res0 = h.fit_grad_batch(var, ls, noise, maxtries=0)
    st = res0[2]
    assert np.array_equal(st != 0, jit > 0)
    for r in range(R):
        if st[r]:
            h.set_params(0, False, var[r], ls[r], noise[r])
            lml, logdet, jt = _lib._fit_scalars()
            dv, dn, dl = ctypes.c_double(), ctypes.c_double(), np.empty(1)
            rc = h.lib.gp_fit_grad(h.h, 0, ctypes.byref(lml), ctypes.byref(logdet), ctypes.byref(jt), ctypes.byref(dv),
                                   _lib.dptr(dl), ctypes.byref(dn))
            assert rc == st[r] and 0 < rc <= J.BATCH_N, (r, rc, st[r])
            if r in J.BATCH_THIRD_TILE:
                assert rc > J.BATCH_N - J.BATCH_DUP > 2 * J.TILE
            assert np.isnan(res0[0][0][r])
        else:
            assert np.array_equal(_batch_rows(res0, r), _batch_rows(res, r))


G = np.load(os.path.join(os.path.dirname(__file__), "golden", "gp_gower.npz"))


@pytest.mark.parametrize("tag", ["G_N64_M48_s0_Mat52_n0.01", "G_N300_M120_s1_rbf_n1e-06"])
def test_gower_members_equal_the_single_call(h, tag):
    domain = json.loads(str(G["domain_json"]))
    for d in domain:
        d["domain"] = tuple(d["domain"])
    space = gpo.Design_space(domain)
    X, Y = G[tag + "/X"], G[tag + "/Y"]
    kernel, ard = int(G[tag + "/kernel"]), bool(int(G[tag + "/ard"]))
    ls0 = np.atleast_1d(G[tag + "/lengthscale"]).astype(float)
    h.set_data(X, Y)
    R = 5
    rng = np.random.default_rng(2)
    var = float(G[tag + "/variance"]) * 10.0 ** rng.uniform(-1, 1, R)
    ls = ls0[None, :] * 10.0 ** rng.uniform(-1, 1, (R, ls0.size))
    noise = float(G[tag + "/noise"]) * 10.0 ** rng.uniform(-0.5, 1, R)
    h.set_params(kernel, ard, var[0], ls[0], noise[0])
    h.set_gower(*gower_config(space, X.shape[1]))
    res = h.fit_grad_batch(var, ls, noise)
    for r in range(R):
        ref = _single(h, kernel, ard, var[r], ls[r], noise[r])
        assert res[2][r] == 0 and ref is not None
        assert np.array_equal(_batch_rows(res, r), ref), (r, _batch_rows(res, r), ref)


def test_resident_fit_is_untouched(h):
    X, Y = _data(300, 3, 1, seed=9)
    Xs = np.random.default_rng(1).uniform(0, 1, (50, 3))
    h.set_data(X, Y)
    h.set_params(1, True, 1.3, np.array([0.3, 0.5, 0.7]), 1e-3)
    state = h.fit()
    h.set_candidates(Xs)
    m0, v0 = h.predict()
    var, ls, noise = _members(5, 3, True, seed=1)
    h.fit_grad_batch(var, ls, noise)
    m1, v1 = h.predict()
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    assert h.fit_state() == state


def test_size_limits(h):
    X, Y = _data(2049, 2, 1, seed=1)
    h.set_data(X, Y)
    h.set_params(0, False, 1.0, np.array([0.3]), 1e-2)
    with pytest.raises(ValueError, match="2048"):
        h.fit_grad_batch(np.ones(2), np.full((2, 1), 0.3), np.full(2, 1e-2))
    X, Y = _data(100, 2, 1, seed=1)
    h.set_data(X, Y)
    h.set_params(0, True, 1.0, np.array([0.3, 0.3]), 1e-2)
    with pytest.raises(ValueError, match="64"):
        h.fit_grad_batch(np.ones(65), np.full((65, 2), 0.3), np.full(65, 1e-2))
    with pytest.raises(ValueError):                     # one lengthscale per member where the model has two
        h.fit_grad_batch(np.ones(2), np.full((2, 1), 0.3), np.full(2, 1e-2))
    with pytest.raises(ValueError):                     # non-positive parameters
        h.fit_grad_batch(np.array([1.0, -1.0]), np.full((2, 2), 0.3), np.full(2, 1e-2))
    lib = h.lib
    n = np.zeros(1)
    st = np.zeros(1, dtype=np.int32)
    p = _lib.dptr(n)
    assert lib.gp_fit_grad_batch(h.h, 0, p, p, p, 5, p, p, p, p, p, p, st.ctypes.data_as(_lib.c_int_p)) == _lib.GP_ERR_ARG


def test_parallel_restarts_above_the_limit_take_the_serial_route():
    X, Y = _data(3000, 2, 1, seed=4)
    m = gpo.models.GPRegression(X, Y, gpo.kern.RBF(2, ARD=False), noise_var=1e-2)
    calls = {"batch": 0}
    orig = m._h.fit_grad_batch

    def counted(*a, **k):
        calls["batch"] += 1
        return orig(*a, **k)

    m._h.fit_grad_batch = counted
    np.random.seed(0)
    runs = m.optimize_restarts(2, verbose=False, max_iters=5, parallel=True)
    assert len(runs) == 2 and calls["batch"] == 0
    m.close()


class _Counting(object):
    def __init__(self, h):
        self.h, self.calls = h, {"fit_grad": 0, "fit_grad_batch": 0}

    def __getattr__(self, name):
        return getattr(self.h, name)

    def fit_grad(self, *a, **k):
        self.calls["fit_grad"] += 1
        return self.h.fit_grad(*a, **k)

    def fit_grad_batch(self, *a, **k):
        self.calls["fit_grad_batch"] += 1
        return self.h.fit_grad_batch(*a, **k)


def _compare_runs(rs, rp):
    assert len(rs) == len(rp)
    for (fs, _), (fp, _) in zip(rs, rp):
        assert abs(fs - fp) <= 1e-8 * abs(fs), (fs, fp)
    assert int(np.argmin([f for f, _ in rs])) == int(np.argmin([f for f, _ in rp]))


def test_model_parallel_restarts_against_serial():
    X, Y = _data(200, 3, 1, seed=12)

    def model():
        m = gpo.models.GPRegression(X, Y, gpo.kern.Matern52(3, ARD=True), noise_var=1e-2)
        m.Gaussian_noise.constrain_bounded(1e-9, 1e6, warning=False)
        return m

    ms, mp = model(), model()
    np.random.seed(77)
    rs = ms.optimize_restarts(5, verbose=False, max_iters=200)
    np.random.seed(77)
    mp._h = _Counting(mp._h)
    rp = mp.optimize_restarts(5, verbose=False, max_iters=200, parallel=True)
    _compare_runs(rs, rp)
    assert mp._h.calls["fit_grad"] == 0 and mp._h.calls["fit_grad_batch"] >= 1
    assert abs(ms.log_likelihood() - mp.log_likelihood()) <= 1e-8 * abs(ms.log_likelihood())
    ms.close()
    mp.close()

    # exact_feval (noise fixed at 1e-6) through GPModel(parallel_restarts=True).updateModel
    out = []
    for flag in (False, True):
        gm = gpo.GPModel(exact_feval=True, optimize_restarts=5, max_iters=200, verbose=False, ARD=True, parallel_restarts=flag)
        gm._create_model(X, Y)
        if flag:
            gm.model._h = _Counting(gm.model._h)
        np.random.seed(78)
        runs = []
        orig = gm.model.optimize_restarts
        gm.model.optimize_restarts = lambda *a, **k: runs.extend(orig(*a, **k)) or runs
        gm.updateModel(X, Y, None, None)
        out.append((runs, gm.model.log_likelihood()))
        if flag:
            assert gm.model._h.calls["fit_grad"] == 0 and gm.model._h.calls["fit_grad_batch"] >= 1
        gm.model.close()
    _compare_runs(out[0][0], out[1][0])
    assert abs(out[0][1] - out[1][1]) <= 1e-8 * abs(out[0][1])
