"""GPU: the wide pass of the fused one-location path (csrc/onerow.hip, rows_forward_wide_kernel and the MV = 8 instances of the
backward, finish and mean-gradient kernels): 5 .. 8 locations in ONE pass over the inverse factor (option "rows_wide").

Per location the wide pass does the arithmetic of the passes of four in their order, so the two routes are compared with
``np.array_equal`` -- no tolerance -- and so is a location in company against the same location alone.  The oracle cases use the
tolerances of tests/test_gpu_rows.py::test_rows_calls_against_the_oracle.

Shapes (the smallest that meet each instance and edge):
  N = 200    2 tiles, the 32-row instance, one chunk, a ragged last tile
  N = 1100   9 tiles, the 32-row instance, two 1024-column chunks (the second cut at the diagonal)
  N = 2200   18 tiles, the 128-row instance, three chunks, N no multiple of 64
  N = 2200 with rows_nt = 1: the non-temporal instance
"""
import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

import _kernel_families as KF

pytestmark = pytest.mark.gpu

ACQS = ((_lib.GP_ACQ_EI, 0.01), (_lib.GP_ACQ_LCB, 2.0), (_lib.GP_ACQ_MPI, 0.01))
SHAPES = [(200, -1), (1100, -1), (2200, -1), (2200, 1)]          # (N, rows_nt)
R0, S0 = np.array([0.05, 0.2, 0.01]), np.array([0.03, 0.1, 0.02])


def _fitted(N, D, nt=-1, P=1, seed=None):
    X, Y, Xs = O.synthetic_problem(N, D, 40, seed=N + D if seed is None else seed)
    ard = D > 1
    ls = O.default_lengthscale(D, ard)
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    h.set_data(X, Y if P == 1 else np.hstack([Y, 0.5 * Y + 0.1]))
    h.set_params(_lib.GP_KERNEL_MATERN52 if D == 8 else _lib.GP_KERNEL_RBF, int(ard), 1.1, ls, 1e-2)
    h.fit()
    h.set_option("rows_build", 1)
    h.set_option("rows_nt", nt)
    return h, X, Xs


def _every_call(h, x, fmin, Xb):
    """Everything the *_rows entry points answer for the rows x, as a flat list of arrays, and the number of calls made."""
    out = []
    for t, par in ACQS:
        out.append(h.acq_rows(x, t, par, fmin, 0.3, 1.7))
        out.extend(h.acq_rows(x, t, par, fmin, 0.3, 1.7, grad=True))
    for noise in (True, False):
        out.extend(h.predict_rows(x, noise))
        out.extend(h.predict_rows(x, noise, grad=True))
    out.append(h.mean_grad_rows(x))
    calls = 6 + 4 + 1
    for (t, par), tr in ((ACQS[0], 0), (ACQS[1], 1)):
        for nb in (0, 1, 3):
            lp = (tr, None, None, None) if nb == 0 else (tr, Xb[:nb], R0[:nb], S0[:nb])
            out.append(h.acq_rows(x, t, par, fmin, lp=lp))
            out.extend(h.acq_rows(x, t, par, fmin, grad=True, lp=lp))
            calls += 2
    return out, calls


@pytest.mark.parametrize("D", [1, 8, 16])
@pytest.mark.parametrize("N,nt", SHAPES)
def test_wide_pass_equals_the_passes_of_four(N, nt, D):
    """rows_wide = 1 (one wide pass per call) against rows_wide = 0 (two passes of at most four) for M = 5 .. 8: EI / LCB / MPI with
    and without gradient, predict_rows with and without gradients and noise, the mean's gradient alone, the penalised
    acquisition under both transforms with 0, 1 and 3 batch points -- the same bits; and the route counters say which ran."""
    h, X, Xs = _fitted(N, D, nt)
    fmin = h.fmin()
    Xb = Xs[20:23]
    for M in (5, 6, 7, 8):
        x = Xs[:M]
        got = {}
        for wide in (1, 0):
            h.set_option("rows_wide", wide)
            p0, s0 = h.rows_pass_stats(), h.rows_stats()
            got[wide], calls = _every_call(h, x, fmin, Xb)
            p1, s1 = h.rows_pass_stats(), h.rows_stats()
            assert s1["fused"] - s0["fused"] == calls and s1["fallback"] == s0["fallback"]
            assert (p1["wide"] - p0["wide"], p1["narrow"] - p0["narrow"]) == ((calls, 0) if wide else (0, 2 * calls))
        for q, (a, b) in enumerate(zip(got[1], got[0])):
            assert np.all(np.isfinite(a[np.isfinite(b)])) and np.array_equal(a, b, equal_nan=True), (M, q, a, b)
    h.set_option("rows_wide", 1)
    h.close()


def _three(h, x, fmin, Xb):
    """EI with gradient, EI value alone, penalised EI with gradient, the posterior with gradients: a flat list of [M, ...] arrays."""
    out = list(h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True))
    out.append(h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin))
    out.extend(h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=(0, Xb, R0, S0)))
    out.extend(h.predict_rows(x, True, grad=True))
    return out


@pytest.mark.parametrize("N", [200, 2200])
def test_a_location_does_not_notice_its_company(N):
    """Location j's results in a call of M rows, M = 1 .. 8 and every slot (the rotations of the first M rows), are those of its
    one-location call, bit for bit: what the lockstep anchor optimiser rests on."""
    h, X, Xs = _fitted(N, 8)
    fmin = h.fmin()
    Xb = Xs[20:23]
    alone = [_three(h, Xs[i:i + 1], fmin, Xb) for i in range(8)]
    for M in range(1, 9):
        for shift in range(M):
            order = np.roll(np.arange(M), shift)
            got = _three(h, Xs[order], fmin, Xb)
            for slot, i in enumerate(order):
                for q, (a, b) in enumerate(zip(got, alone[i])):
                    assert np.array_equal(a[slot], b[0]), (M, shift, slot, q, a[slot], b[0])
    h.close()


ORACLE_CASES = [(fam, ard) for fam in ("rbf", "Mat52", "Mat32", "Exponential") for ard in (False, True)]
KERN = {"rbf": "RBF", "Mat52": "Matern52", "Mat32": "Matern32", "Exponential": "Exponential"}


def _hold_to_the_oracle(gm, gm0, x):
    f0 = gm0.get_fmin()
    assert abs(gm.get_fmin() - f0) <= 1e-6 * max(1.0, abs(f0))
    pairs = ((gpo.AcquisitionEI(gm), lambda z: O.acq_EI_withGradients(gm0, z, 0.01, f0)),
             (gpo.AcquisitionLCB(gm), lambda z: O.acq_LCB_withGradients(gm0, z, 2.0)),
             (gpo.AcquisitionMPI(gm), lambda z: O.acq_MPI_withGradients(gm0, z, 0.01, f0)))
    h = gm.model._h
    p0 = h.rows_pass_stats()
    for acq, ref in pairs:
        a, da = acq.acquisition_function_withGradients(x)
        a0, da0 = ref(x)
        for j in range(x.shape[0]):       # the tolerances of test_rows_calls_against_the_oracle, location by location
            assert abs(a[j].item() + a0[j].item()) <= 1e-5 * max(abs(a0[j].item()), 1e-12), (type(acq).__name__, j, a[j], a0[j])
            np.testing.assert_allclose(da[j], -da0[j], rtol=0, atol=1e-5 * max(np.max(np.abs(da0[j])), 1e-12))
        v = acq.acquisition_function(x)
        assert np.max(np.abs(v - a)) <= 1e-6 * np.max(np.abs(a))
    p1 = h.rows_pass_stats()
    assert p1["wide"] - p0["wide"] == 6 and p1["narrow"] == p0["narrow"]


@pytest.mark.parametrize("N", [200, 2200])
@pytest.mark.parametrize("fam,ard", ORACLE_CASES)
def test_wide_pass_against_the_oracle(N, fam, ard):
    """EI / LCB / MPI and their gradients at eight locations (D = 8: one wide pass each) against the oracle's restatement of
    acquisition_function_withGradients, for the four covariance families with one and with per-dimension lengthscales."""
    D = 8
    X, Y, Xs = O.synthetic_problem(N, D, 12, seed=5 + N)
    x = np.vstack([Xs[:7], X[[17]]])                    # seven locations off and one ON a training point
    ls = O.default_lengthscale(D, ard)
    gm = gpo.GPModel(kernel=getattr(gpo.kern, KERN[fam])(D, 1.2, ls, ARD=ard), noise_var=1e-2, max_iters=0, verbose=False, ARD=ard)
    gm.updateModel(X, Y, None, None)
    gm0 = O.OracleGPModel(O.OracleGP(X, Y, KF.make(fam, D, 1.2, ls, ard, direct=True), 1e-2))   # r = 0 exactly on the training point
    _hold_to_the_oracle(gm, gm0, x)
    gm.model.close()


@pytest.mark.parametrize("N", [200, 2200])
def test_wide_pass_against_the_oracle_under_the_gower_kernel(N):
    dom = [{'name': 'a', 'type': 'discrete', 'domain': (0, 1, 2, 3)}, {'name': 'x', 'type': 'continuous', 'domain': (-2.0, 5.0)},
           {'name': 'b', 'type': 'discrete', 'domain': (10, 20)}, {'name': 'y', 'type': 'continuous', 'domain': (0.0, 0.5)}]
    space0 = O.MixedSpace(dom)
    rng = np.random.default_rng(3)
    X, x = space0.draw(rng, N), space0.draw(rng, 8)
    x[0] = X[7]
    Y = O.normalize((np.sin(X[:, 1]) + 0.3 * X[:, 0] - 0.1 * (X[:, 2] == 20) + 2 * X[:, 3])[:, None])
    space = gpo.Design_space(dom)
    gm = gpo.GPModel(kernel=gpo.kern.RBF(4, 0.9, 1.7, Gower=True, space=space), noise_var=1e-3, max_iters=0, Gower=True,
                     space=space, verbose=False)
    gm.updateModel(X, Y, None, None)
    gm0 = O.OracleGPModel(O.OracleGP(X, Y, O.make_kernel("rbf", 4, 0.9, [1.7], Gower=True, space=space0), 1e-3))
    _hold_to_the_oracle(gm, gm0, x)
    gm.model.close()


def _close(a, b, rel):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= rel * max(np.max(np.abs(b)), 1e-300), float(np.max(np.abs(a - b)))


def test_routing_edges():
    """M D > 128 keeps the passes of four (same results as the batched calls); small_m = 4 and P = 2 take the batched calls."""
    h, X, Xs = _fitted(200, 17)
    fmin = h.fmin()
    x = Xs[:8]
    p0, s0 = h.rows_pass_stats(), h.rows_stats()
    a, da = h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
    mu, var, dm, dv = h.predict_rows(x, True, grad=True)
    p1, s1 = h.rows_pass_stats(), h.rows_stats()
    assert (p1["narrow"] - p0["narrow"], p1["wide"] - p0["wide"]) == (4, 0) and s1["fused"] - s0["fused"] == 2
    h.set_candidates(x)
    mu_b, var_b = h.predict(True)
    dm_b, dv_b = h.predict_grad()
    a_b, da_b = h.acq_grad(_lib.GP_ACQ_EI, 0.01, fmin)
    _close(mu, mu_b, 1e-9)                # the tolerances of test_rows_calls_equal_the_batched_calls at noise 1e-2
    assert np.max(np.abs(var - var_b) / np.abs(var_b)) <= 1e-9
    _close(dm, dm_b, 1e-9)
    _close(dv, dv_b, 1e-8)
    _close(a, a_b, 1e-8)
    _close(da, da_b, 1e-7)
    h.set_option("rows_wide", 0)          # ... and the option changes nothing there
    a2, da2 = h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
    assert np.array_equal(a, a2) and np.array_equal(da, da2)
    h.close()

    h, X, Xs = _fitted(200, 8)
    fmin = h.fmin()
    wide = h.acq_rows(Xs[:5], _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
    h.set_option("small_m", 4)
    p0, s0 = h.rows_pass_stats(), h.rows_stats()
    back = h.acq_rows(Xs[:5], _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
    assert h.rows_stats()["fallback"] == s0["fallback"] + 1 and h.rows_pass_stats() == p0
    _close(wide[0], back[0], 1e-8)
    _close(wide[1], back[1], 1e-7)
    h.close()

    h, X, Xs = _fitted(200, 8, P=2)
    p0, s0 = h.rows_pass_stats(), h.rows_stats()
    mu, var = h.predict_rows(Xs[:5], True)
    assert mu.shape == (5, 2) and np.all(np.isfinite(mu))
    assert h.rows_stats()["fallback"] == s0["fallback"] + 1 and h.rows_pass_stats() == p0
    h.close()


@pytest.mark.parametrize("N", [200, 2200])
def test_training_point_duplicates_and_a_nan_row(N):
    """A row ON a training point, the same row twice, and a row with a NaN coordinate in one wide call: every other row is finite
    and equal to its one-location call."""
    h, X, Xs = _fitted(N, 8)
    fmin = h.fmin()
    Xb = Xs[20:23]
    x = np.vstack([Xs[0], X[3], Xs[0], Xs[2], Xs[4], X[N - 1], Xs[5]])
    x[4, 2] = np.nan
    p0 = h.rows_pass_stats()
    got = _three(h, x, fmin, Xb)
    assert h.rows_pass_stats()["wide"] - p0["wide"] == 4
    for j in (0, 1, 2, 3, 5, 6):
        alone = _three(h, x[j:j + 1], fmin, Xb)
        for q, (a, b) in enumerate(zip(got, alone)):
            assert np.all(np.isfinite(a[j])) and np.array_equal(a[j], b[0]), (j, q, a[j], b[0])
    for a in got:
        assert np.array_equal(a[0], a[2])
    assert np.isnan(got[0][4]).all()
    h.close()


def test_wide_pass_repeats_its_bits_and_is_guarded_against_stale_results():
    """The same wide call twice gives the same bits.  With the arrival base skewed (the existing test hook) no workgroup finishes
    the wide pass: the call raises instead of returning the block's previous contents, and the next call is right again."""
    h, X, Xs = _fitted(1100, 8)
    fmin = h.fmin()
    x = Xs[:8]
    one = h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
    two = h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    h.acq_rows(Xs[8:16], _lib.GP_ACQ_EI, 0.01, fmin, grad=True)        # other numbers in the block
    for call in (lambda: h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True), lambda: h.predict_rows(x, True),
                 lambda: h.mean_grad_rows(x)):
        h.set_option("debug_rows_skew", 3)
        with pytest.raises(RuntimeError, match="did not complete"):
            call()
        again = h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
        assert np.array_equal(again[0], one[0]) and np.array_equal(again[1], one[1])
    h.close()
