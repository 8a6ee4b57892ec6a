"""The strands of the look-ahead factorisation scheduler (csrc/api_factor.hip) in combination, at the smallest sizes at which
each still does something: chain-owned tile columns, pipelined candidate / L^-T stages, a ragged last panel."""
import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

N, D, M = 1280, 3, 300   # 10 tiles, P = 1
DEFAULTS = {"emulate_fp64": 0, "lookahead": 1, "lookahead_min_tiles": 40, "panel_tiles": 6, "own_keep_per_row": 36,
            "own_keep_base": 200, "pipe_stages": 0, "pipe_start_pct": -1, "pipe_stages_grad": 0, "pipe_start_pct_grad": 40}
OWNED = {"plain": {"own_keep_per_row": 0}, "owned": {"own_keep_per_row": 1, "own_keep_base": 0}}
# automatic stages and release point, or every stage behind the factorisation from the first panel on
# (pipe_start_pct_grad has no automatic value: its default stands in)
PIPE = {"auto": {"pipe_stages": 0, "pipe_start_pct": -1, "pipe_stages_grad": 0, "pipe_start_pct_grad": 40},
        "all": {"pipe_stages": 1 << 20, "pipe_start_pct": 0, "pipe_stages_grad": 1 << 20, "pipe_start_pct_grad": 0}}


@pytest.fixture(scope="module")
def problem():
    h = _lib.Handle(0)
    X, Y, Xs = O.synthetic_problem(N, D, M, seed=1280)
    try:
        h.set_option("emulate_fp64", 0)
        h.set_option("lookahead_min_tiles", 0)
        h.set_data(X, Y)
        h.set_params(0, 0, 1.2, [0.5], 1e-2)
        h.set_candidates(Xs)
        yield h
    finally:
        for k, v in DEFAULTS.items():
            h.set_option(k, v)
        h.close()


@pytest.fixture(scope="module", params=[1, 3])
def baseline(request, problem):
    """lookahead = 0: the single-stream factorisation through gp_fit + gp_predict + gp_lml_grad, once per panel width."""
    h = problem
    h.set_option("panel_tiles", request.param)
    h.set_option("lookahead", 0)
    try:
        lml, _, jit = h.fit()
        ref = dict(W=request.param, lml=lml, jit=jit, L=h.chol(), alpha=h.alpha(), pred=h.predict(True), grad=h.lml_grad(1))
    finally:
        h.set_option("lookahead", 1)
    return ref


@pytest.mark.parametrize("pipe", sorted(PIPE))
@pytest.mark.parametrize("owned", sorted(OWNED))
def test_lookahead_strands_combined_equal_the_single_stream_factorisation(problem, baseline, owned, pipe):
    """N = 1280 is 10 tiles.  panel_tiles = 1: at the first panel the rule (own_keep_per_row = 1, own_keep_base = 0) has n = 8 rows
    below the look-ahead target, keeps 1 tile and owns 7 tile columns; panel_tiles = 3: three panels and a last one of a single
    tile, 3 columns owned at panel 0 and 1 at panel 1.  Whatever the owned range and however many candidate / L^-T stages ride
    behind the factorisation, every tile takes the same contractions in the same order: factor, alpha, LML, jitter, posterior
    and gradients are BITWISE those of lookahead = 0 through the separate calls."""
    h, ref = problem, baseline
    opts = dict(OWNED[owned], **PIPE[pipe])
    try:
        h.set_option("panel_tiles", ref["W"])
        for k, v in opts.items():
            h.set_option(k, v)
        lml, _, jit = h.fit()
        assert lml == ref["lml"] and jit == ref["jit"]
        assert np.array_equal(h.chol(), ref["L"]) and np.array_equal(h.alpha(), ref["alpha"])
        (lml, _, _), mu, var = h.fit_predict(True)
        assert lml == ref["lml"] and np.array_equal(mu, ref["pred"][0]) and np.array_equal(var, ref["pred"][1])
        (lml, _, _), (dv, dl, dn) = h.fit_grad(1)
        assert lml == ref["lml"]
        assert dv == ref["grad"][0] and np.array_equal(dl, ref["grad"][1]) and dn == ref["grad"][2]
    finally:
        for k in opts:
            h.set_option(k, DEFAULTS[k])
