"""One case of the stream-operation comparison between two builds (profiles/r09_scheduler_strands.txt): every strand of the
factorisation scheduler, each call made twice (the first allocates, the second is the steady state).  Run it under
rocprofv3 --kernel-trace / --hip-trace on a GPU, or against a library linked with tools/hip_recorder.cpp anywhere.
usage: stream_ops.py <case: 1 2 3 4a 4b 5 6a 6b 7 8 9>"""
import sys
import numpy as np
from gaussian_process_optimization_amd import _lib

case = sys.argv[1]
D = 5
def problem(N, M=0, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D)); Y = np.sin(3 * X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
    Xs = rng.uniform(0, 1, (M, D)) if M else None
    return X, Y, Xs
h = _lib.Handle(0)
def setup(N, M=0, opts=()):
    X, Y, Xs = problem(N, M)
    h.set_option("emulate_fp64", 0)
    for k, v in opts: h.set_option(k, v)
    h.set_data(X, Y); h.set_params(0, 0, 1.2, [0.5], 1e-2)
    if M: h.set_candidates(Xs)
def twice(fn):
    a = fn(); h.synchronize(); b = fn(); h.synchronize()
    return b
if case == "1":
    setup(6144, 1000); r = twice(lambda: h.fit_predict(True)); print(case, r[0], float(r[1].sum()), float(r[2].sum()))
elif case == "2":
    setup(6144); r = twice(lambda: h.fit_grad(1)); print(case, r)
elif case == "3":
    setup(3000, 0, [("lookahead_min_tiles", 0), ("own_keep_per_row", 4), ("own_keep_base", 0)]); print(case, twice(h.fit))
elif case == "4a":
    setup(2048); print(case, twice(h.fit))
elif case == "4b":
    setup(300); print(case, twice(h.fit))
elif case == "5":
    setup(2048, 0, [("inner_tiles", 2)]); print(case, twice(h.fit))
elif case in ("6a", "6b"):
    setup(6144, 0, [("panel_tiles", 4), ("rns_group_fit", 8 if case == "6a" else 1)])
    h.set_option("emulate_fp64", 1); print(case, twice(h.fit))
elif case == "7":
    setup(300, 200); h.fit()
    Z = np.random.default_rng(3).standard_normal((4, 200))
    r = twice(lambda: h.posterior_samples(Z, False)); print(case, [float(np.sum(x)) for x in r if hasattr(x, "sum")])
elif case == "8":   # the combinations of tests/test_gpu_lookahead.py
    setup(1280, 300, [("lookahead_min_tiles", 0)])
    for W in (1, 3):
        for own in ((0, 200), (1, 0)):
            for pipe in ((0, -1, 0, 40), (1 << 20, 0, 1 << 20, 0)):
                for k, v in zip(("panel_tiles", "own_keep_per_row", "own_keep_base", "pipe_stages", "pipe_start_pct", "pipe_stages_grad", "pipe_start_pct_grad"), (W,) + own + pipe):
                    h.set_option(k, v)
                h.fit(); h.fit_predict(True); h.fit_grad(1)
elif case == "9":   # the default owned-column rule where it owns columns, with the pipe sharing the bulk stream's CUs
    setup(12416, 700)
    for pct in (0, 50):
        h.set_option("own_keep_pipe_pct", pct)
        h.fit(); h.fit_predict(True); h.fit_grad(1)
else:
    raise SystemExit("unknown case")
h.close()
