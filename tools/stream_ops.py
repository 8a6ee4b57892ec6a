"""One case of the stream-operation comparison between two builds (profiles/r09_scheduler_strands.txt, r10_scoring_layer.txt):
every strand of the factorisation scheduler (1 ... 9) and the scoring entry points (s1 ... s8), each call made twice (the first
allocates, the second is the steady state).  Run it under rocprofv3 --kernel-trace / --hip-trace on a GPU, or against a library
linked with tools/hip_recorder.cpp anywhere.  The scoring cases save every array and scalar they got back when given a path.
s9 ... s12 are the table entries of the sparse model, the ensemble and entropy search, and all four tables interleaved.
usage: stream_ops.py <case: 1 2 3 4a 4b 5 6a 6b 7 8 9 s1 s2 s3 s4a s4b s5 s6 s7 s8 s9 s10 s11 s12> [results.npz]"""
import sys
import numpy as np
from gaussian_process_optimization_amd import _lib

case = sys.argv[1]
D = 3 if case.startswith("s") else 5
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
elif case.startswith("s"):
    EI, LCB = _lib.GP_ACQ_EI, _lib.GP_ACQ_LCB
    got = {}
    def keep(name, fn):   # fn twice; what the second call returned, flattened into got[name.i]
        r = twice(fn)
        for i, x in enumerate(r if isinstance(r, tuple) else (r,)): got["%s.%d" % (name, i)] = np.asarray(x)
        return r
    rng = np.random.default_rng(11)
    Xb, r0, s0 = rng.uniform(0, 1, (3, D)), np.array([0.05, 0.2, 0.01]), np.array([0.03, 0.1, 0.02])
    def table_calls(o, fmin, M):   # what Handle and Group share
        keep("acq_argbest", lambda: o.acq_argbest(EI, 0.01, fmin, -1))
        keep("acq_topk", lambda: o.acq_topk(LCB, 2.0, fmin, +1, 5))
        keep("acq_lp_argbest", lambda: o.acq_lp_argbest(EI, 0.01, fmin, 1, -1, Xb, r0, s0, exclude=range(0, 2 * min(256, M // 2), 2)))
    if case == "s1":
        setup(300, 1001); h.fit(); fmin = keep("fmin", h.fmin)
        keep("acq", lambda: h.acq(EI, 0.01, fmin)); keep("acq_grad", lambda: h.acq_grad(LCB, 2.0, fmin))
        table_calls(h, fmin, 1001)
        keep("acq_lp", lambda: h.acq_lp(EI, 0.01, fmin, 1, Xb, r0, s0)); keep("acq_lp0", lambda: h.acq_lp(EI, 0.01, fmin, 0))
        keep("acq_lp_grad", lambda: h.acq_lp_grad(EI, 0.01, fmin, 1, Xb, r0, s0))
    elif case in ("s2", "s3"):   # s3: N = 4500, where the first *_rows calls after a fit take the batched entry points
        setup(300 if case == "s2" else 4500, 9); h.fit(); fmin = h.fmin(); Xs = problem(300, 9)[2]
        for n, M in enumerate((1, 4, 5, 9) if case == "s2" else (1, 1, 1, 5, 1, 1, 1, 1)):
            for grad in (False, True):
                keep("%d.predict_rows%d%d" % (n, M, grad), lambda: h.predict_rows(Xs[:M], True, grad))
                for lp in (None, (1, Xb, r0, s0), (0, None, None, None)):
                    keep("%d.acq_rows%d%d%s" % (n, M, grad, lp and lp[0]), lambda: h.acq_rows(Xs[:M], EI, 0.01, fmin, grad=grad, lp=lp))
            keep("%d.mean_grad_rows%d" % (n, M), lambda: h.mean_grad_rows(Xs[:M]))
        got["rows_stats"] = np.array(sorted(h.rows_stats().items()), dtype=object)[:, 1].astype(np.int64)
    elif case in ("s4a", "s4b"):
        X, Y, Xs = problem(300, 1001)
        grp = _lib.Group((0, 0) if case == "s4a" else (0,))
        grp.set_option("emulate_fp64", 0); grp.set_data(X, Y); grp.set_params(0, 0, 1.2, [0.5], 1e-2)
        got["fit"] = np.array(grp.fit()); fmin = grp.fmin()
        for M in (1001, 3):
            twice(lambda: grp.set_candidates(Xs[:M])); table_calls(grp, fmin, M)
            got.update({k + "/%d" % M: got.pop(k) for k in list(got) if k.startswith("acq")})
        grp.close()
    elif case == "s5":
        setup(300); h.comm_init(h.comm_unique_id(), 0, 1)
        keep("allgather_best", lambda: h.comm_allgather_best(-0.25, 123456789012, 1))
        keep("allgather_topk", lambda: h.comm_allgather_topk(np.arange(5) * 0.5, np.arange(5) + (1 << 40), 1))
    elif case in ("s6", "s7", "s8"):   # the fused rows passes of the sparse model (s6), the ensemble (s7), and all three interleaved (s8)
        setup(300, 9); Xs = problem(300, 9)[2]
        def sparse_fit():
            h.sparse_set_inducing(problem(40, seed=3)[0]); h.sparse_fit(); return h.sparse_fmin()
        def ens_fit(S):
            h.ens_fit(np.linspace(1.0, 1.4, S), np.linspace(0.4, 0.6, S)[:, None], np.linspace(1e-2, 2e-2, S))
        if case == "s6":   # M = 9 takes the fallback
            fmin = sparse_fit()
            for M in (1, 4, 5, 8, 9):
                for grad in (False, True):
                    keep("sparse_predict_rows%d%d" % (M, grad), lambda: h.sparse_predict_rows(Xs[:M], True, grad))
                    for lp in (None, (1, Xb, r0, s0)):
                        keep("sparse_acq_rows%d%d%s" % (M, grad, lp and lp[0]), lambda: h.sparse_acq_rows(Xs[:M], EI, 0.01, fmin, grad=grad, lp=lp))
            got["sparse_rows_stats"] = np.array(sorted(h.sparse_rows_stats().items()), dtype=object)[:, 1].astype(np.int64)
        elif case == "s7":   # the second fit, with another S, restarts the counters
            ens_fit(3)
            for M in (1, 4, 5, 8):
                if M == 5: ens_fit(2)
                for grad in (False, True):
                    keep("ens_predict_rows%d%d" % (M, grad), lambda: h.ens_predict_rows(Xs[:M], True, grad))
                    keep("ens_acq_rows%d%d" % (M, grad), lambda: h.ens_acq_rows(Xs[:M], EI, 0.01, grad=grad))
        else:
            h.fit(); fmin = h.fmin(); smin = sparse_fit(); ens_fit(3)
            for M in (1, 5):
                for grad in (False, True):
                    keep("acq_rows%d%d" % (M, grad), lambda: h.acq_rows(Xs[:M], EI, 0.01, fmin, grad=grad))
                    keep("sparse_acq_rows%d%d" % (M, grad), lambda: h.sparse_acq_rows(Xs[:M], EI, 0.01, smin, grad=grad))
                    keep("ens_acq_rows%d%d" % (M, grad), lambda: h.ens_acq_rows(Xs[:M], EI, 0.01, grad=grad))
                    keep("predict_rows%d%d" % (M, grad), lambda: h.predict_rows(Xs[:M], True, grad))
                    keep("ens_predict_rows%d%d" % (M, grad), lambda: h.ens_predict_rows(Xs[:M], True, grad))
                    keep("sparse_predict_rows%d%d" % (M, grad), lambda: h.sparse_predict_rows(Xs[:M], True, grad))
    elif case in ("s9", "s10", "s11", "s12"):   # the candidate tables of the sparse model (s9), the ensemble (s10), ES (s11), all four (s12)
        setup(300, 1001); Xs = problem(300, 1001)[2]; ex = range(0, 512, 2)
        def sparse_fit():
            h.sparse_set_inducing(problem(40, seed=3)[0]); h.sparse_fit(); return h.sparse_fmin()
        def ens_fit(S=3):
            h.ens_fit(np.linspace(1.0, 1.4, S), np.linspace(0.4, 0.6, S)[:, None], np.linspace(1e-2, 2e-2, S))
        def es_belief(R=6, S=4):   # from host arrays: the EP sites come from a kernel, which a recorder does not run
            h.es_set_representers(rng.uniform(0, 1, (R, D)))
            h.es_set_belief(np.log(np.full(R, 1.0 / R)), np.zeros(R), rng.standard_normal((R, R)), rng.standard_normal((R, R, R)), np.linspace(-1, 1, S))
        def sparse_table(fmin, M, tag=""):
            twice(lambda: h.sparse_set_candidates(Xs[:M]))
            for grad in (False, True):
                for lp in (None, (1, Xb, r0, s0)):
                    keep("sparse_acq%d%s%s" % (grad, lp and lp[0], tag), lambda: h.sparse_acq(EI, 0.01, fmin, grad=grad, lp=lp))
            keep("sparse_acq_argbest" + tag, lambda: h.sparse_acq_argbest(EI, 0.01, fmin, -1, lp=(1, Xb, r0, s0), exclude=[e for e in ex if e < M]))
            keep("sparse_acq_topk" + tag, lambda: h.sparse_acq_topk(LCB, 2.0, fmin, +1, 5))
        def ens_table(tag=""):
            keep("ens_acq" + tag, lambda: h.ens_acq(EI, 0.01))
            for sense in (-1, +1): keep("ens_acq_argbest%d%s" % (sense, tag), lambda: h.ens_acq_argbest(LCB, 2.0, sense))
        def es_table(tag=""):
            keep("es_acq" + tag, lambda: h.es_acq(1.0))
            for sense in (-1, +1): keep("es_acq_argbest%d%s" % (sense, tag), lambda: h.es_acq_argbest(sense, 1.0))
        if case == "s9":
            fmin = sparse_fit()
            for M in (1001, 3): sparse_table(fmin, M, "/%d" % M)
            for grad in (False, True):   # M = 9: the fallback of the rows entry, over scratch
                for lp in (None, (1, Xb, r0, s0)):
                    keep("sparse_acq_rows9%d%s" % (grad, lp and lp[0]), lambda: h.sparse_acq_rows(Xs[:9], EI, 0.01, fmin, grad=grad, lp=lp))
        elif case == "s10":
            ens_fit()
            for M in (1001, 3): twice(lambda: h.set_candidates(Xs[:M])); ens_table("/%d" % M)
        elif case == "s11":
            h.fit(); es_belief()
            for M in (1001, 3): twice(lambda: h.set_candidates(Xs[:M])); es_table("/%d" % M)
        else:   # gp_es_* refuses a context that holds a sparse fit or an ensemble: ES beside the exact table, then the other two, then ES again
            def exact(tag, M):
                keep("acq_lp_argbest" + tag, lambda: h.acq_lp_argbest(EI, 0.01, fmin, 1, -1, Xb, r0, s0, exclude=[e for e in ex if e < M]))
                yield
                keep("acq_rows" + tag, lambda: h.acq_rows(Xs[:3], EI, 0.01, fmin, grad=True, lp=(1, Xb, r0, s0)))
                keep("acq_topk" + tag, lambda: h.acq_topk(LCB, 2.0, fmin, +1, 5))
                yield
                keep("acq_lp_grad" + tag, lambda: h.acq_lp_grad(EI, 0.01, fmin, 1, Xb, r0, s0))
                yield
            for M in (1001, 3):
                X, Y, _ = problem(300); h.set_data(X, Y); h.set_params(0, 0, 1.2, [0.5], 1e-2); h.set_candidates(Xs[:M])
                h.fit(); fmin = h.fmin(); es_belief()
                for n, _ in enumerate(exact("/%d.es" % M, M)): es_table("/%d.%d" % (M, n))
                smin = sparse_fit(); ens_fit()
                for n, _ in enumerate(exact("/%d" % M, M)):
                    if n == 0: sparse_table(smin, M, "/%d" % M)
                    if n == 1: keep("sparse_acq_rows/%d" % M, lambda: h.sparse_acq_rows(Xs[:9], EI, 0.01, smin, grad=True, lp=(0, Xb, r0, s0)))
                    if n == 2: keep("sparse_acq_topk2/%d" % M, lambda: h.sparse_acq_topk(EI, 0.01, smin, -1, 5))
                    ens_table("/%d.%d" % (M, n))
    else:
        raise SystemExit("unknown case")
    print(case, {k: float(np.sum(v)) for k, v in got.items()})
    if len(sys.argv) > 2: np.savez(sys.argv[2], **got)
else:
    raise SystemExit("unknown case")
h.close()
