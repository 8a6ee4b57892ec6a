"""GPU: the three fused rows paths -- exact model, sparse model, ensemble -- on ONE context.  Each path owns the arrival counter,
counter bases, ticket and pinned result block of its passes (PassOwner, csrc/api_internal.h); whatever the order of the calls, a
path returns the bits it returns on a context that runs it alone, and a pass of one path that nobody finishes leaves the other
two untouched.
"""
import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

N, D, MZ, S = 300, 3, 40, 3   # three tiles, five finishing workgroups of the exact pass and of each member, five of the sparse pass
EI = _lib.GP_ACQ_EI
SIZES = (1, 5)                # one narrow pass; a wide pass (exact), one pass (sparse), passes of four and of one (ensemble)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_three_paths_on_one_context_keep_their_bits_and_their_own_recovery():
    X, Y, Xs = O.synthetic_problem(N, D, 40, seed=31)
    Z = X[::7][:MZ].copy()
    var, ls, noise = np.array([0.9, 1.1, 1.3]), np.array([[0.4], [0.5], [0.6]]), np.array([1e-2, 2e-2, 1.5e-2])

    def handle(exact, sparse, ens):
        h = _lib.Handle(0)
        h.set_option("emulate_fp64", 0)
        h.set_data(X, Y)
        h.set_params(_lib.GP_KERNEL_RBF, 0, 1.1, [0.5], 1e-2)
        if exact:
            h.fit()
        if sparse:
            h.sparse_set_inducing(Z)
            h.sparse_fit()
        if ens:
            h.ens_fit(var, ls, noise)
        return h

    calls = {"exact": lambda h, M: h.acq_rows(Xs[:M], EI, 0.01, -1.0, grad=True),
             "sparse": lambda h, M: h.sparse_acq_rows(Xs[:M], EI, 0.01, -1.0, grad=True),
             "ens": lambda h, M: h.ens_acq_rows(Xs[:M], EI, 0.01, grad=True)}
    want = {}
    for path in calls:   # the reference bits: each path on a context that runs it alone
        alone = handle(path == "exact", path == "sparse", path == "ens")
        for M in SIZES:
            want[path, M] = calls[path](alone, M)
            assert np.all(np.isfinite(want[path, M][0])) and np.all(np.isfinite(want[path, M][1]))
        alone.close()
    assert not np.array_equal(want["exact", 1][0], want["sparse", 1][0]) and not np.array_equal(want["exact", 1][0], want["ens", 1][0])

    h = handle(True, True, True)
    try:
        fused0, sparse0 = h.rows_stats()["fused"], h.sparse_rows_stats()["fused"]
        for order in (("exact", "sparse", "ens"), ("ens", "exact", "sparse", "sparse", "ens", "exact")):
            for M in SIZES:
                for path in order:
                    assert _same(calls[path](h, M), want[path, M]), (order, M, path)
        assert h.rows_stats()["fused"] - fused0 == 6 and h.sparse_rows_stats()["fused"] - sparse0 == 6   # (all on the fused paths)
        # nobody finishes the exact model's next pass: that call fails, the other two owners were not touched
        h.set_option("debug_rows_skew", 3)
        with pytest.raises(RuntimeError, match="did not complete"):
            calls["exact"](h, 1)
        for M in SIZES:
            assert _same(calls["sparse"](h, M), want["sparse", M])
            assert _same(calls["ens"](h, M), want["ens", M])
        for M in SIZES:
            assert _same(calls["exact"](h, M), want["exact", M])
    finally:
        h.close()
