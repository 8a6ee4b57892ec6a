"""GPU: the scoring entry points as a layer (csrc/api_predict.hip, api_grad.hip, api_rows.hip, api_group.hip, api_comm.hip).

Three things no numerical test of a single entry point sees: that the small scratch buffers the entry points share (the scratch
map of csrc/api_internal.h) serve any interleaving of them, which code every refused call returns -- and that it leaves the
context as it was -- and how a group treats blocks whose rows are all excluded.  Everything here is index and bit equality:
the references are NumPy's lowest-index arg-best and stable sort over vectors the device itself returned.

The table of return codes was checked against the parent of the refactor with tools/hip_recorder.cpp standing in for the
device; profiles/r10_scoring_layer.txt says what else was and was not run on an MI355X when this file was written.
"""
import ctypes

import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

EI, LCB = _lib.GP_ACQ_EI, _lib.GP_ACQ_LCB
ARG, STATE = _lib.GP_ERR_ARG, _lib.GP_ERR_STATE
R0, S0 = np.array([0.05, 0.2, 0.01]), np.array([0.03, 0.1, 0.02])


def _context(N, M, P=1, fit=True, candidates=True, seed=5):
    X, Y, Xs = O.synthetic_problem(N, 3, M, seed=seed)
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    h.set_data(X, np.repeat(Y, P, axis=1))
    h.set_params(_lib.GP_KERNEL_RBF, 0, 1.1, [0.4], 1e-2)
    if fit:
        h.fit()
    if candidates:
        h.set_candidates(Xs)
    return h, Xs


def _same(a, b):
    a, b = [np.asarray(x) for x in a], [np.asarray(x) for x in b]
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_scratch_slots_serve_any_order_of_the_scoring_calls():
    """N = 300 (three tiles, the last partial), M = 600 (three first-level arg-best blocks: the two-level reduction and its
    partial slots), one context.  The calls that share dScal / dRedV / dRedI / dComm -- the penalised arg-best with a batch of 3
    and all 256 excluded-row slots taken, top-5, the training minimum, both gathers of a one-rank communicator, the plain
    arg-best and posterior samples (S = 2, M = 200) -- in two orders, each after a fresh fit so that gp_fmin reduces again.
    Winners and values are NumPy's over the device's own gp_acq / gp_acq_lp vectors, and the two orders agree in every bit."""
    h, Xs = _context(300, 600)
    fmin0 = h.fmin()
    Xb = Xs[7:10]
    acq = h.acq(EI, 0.01, fmin0).ravel()
    lp = h.acq_lp(EI, 0.01, fmin0, 1, Xb, R0, S0).ravel()
    order_lp = np.argsort(lp, kind="stable")
    taken = order_lp[:256]
    Z = np.random.default_rng(3).standard_normal((2, 200))
    h.comm_init(h.comm_unique_id(), 0, 1)

    def samples():
        h.set_candidates(Xs[:200])
        r = h.posterior_samples(Z, False)
        h.set_candidates(Xs)
        return r

    ops = {
        "lp_argbest": lambda: h.acq_lp_argbest(EI, 0.01, fmin0, 1, -1, Xb, R0, S0, exclude=taken),
        "topk": lambda: h.acq_topk(EI, 0.01, fmin0, -1, 5),
        "topk_max": lambda: h.acq_topk(EI, 0.01, fmin0, +1, 5),
        "fmin": lambda: (h.fmin(),),
        "gather_best": lambda: h.comm_allgather_best(-0.25, 123456789012, 1),
        "gather_topk": lambda: h.comm_allgather_topk(np.arange(5) * 0.5, np.arange(5) + (1 << 40), 1),
        "argbest": lambda: h.acq_argbest(EI, 0.01, fmin0, -1),
        "argbest_max": lambda: h.acq_argbest(EI, 0.01, fmin0, +1),
        "samples": samples,
    }
    names = list(ops)
    runs = []
    for order in (names, [names[i] for i in (8, 3, 6, 0, 4, 1, 7, 5, 2)]):
        h.fit()
        runs.append({name: ops[name]() for name in order})
    first, second = runs
    for name in names:
        assert _same(first[name], second[name]), name
    up = np.argsort(acq, kind="stable")
    down = np.argsort(-acq, kind="stable")
    for r in runs:
        assert r["lp_argbest"] == (int(order_lp[256]), lp[order_lp[256]])
        assert np.array_equal(r["topk"][0], up[:5]) and np.array_equal(r["topk"][1], acq[up[:5]])
        assert np.array_equal(r["topk_max"][0], down[:5]) and np.array_equal(r["topk_max"][1], acq[down[:5]])
        assert r["argbest"] == (int(np.argmin(acq)), acq.min()) and r["argbest_max"] == (int(np.argmax(acq)), acq.max())
        assert r["fmin"] == (fmin0,)
        assert _same(r["gather_best"], (np.array([-0.25]), np.array([123456789012])))
        assert _same(r["gather_topk"], (np.arange(5) * 0.5, np.arange(5) + (1 << 40)))
    h.close()


# ---- return codes of refused calls ------------------------------------------------------------------------------------------
# Arguments of the raw symbols, in the order of include/gphip.h; "g" is the context (or group) of the row's fault.
_ACQ = ["type", "par", "fmin", "y_mean", "y_std"]
_LP = ["transform", "Xb", "nb", "r0", "s0"]
ENTRIES = {
    "gp_predict": ["g", "noise", "mean", "var"],
    "gp_fmin": ["g", "scalar"],
    "gp_acq": ["g"] + _ACQ + ["out"],
    "gp_acq_argbest": ["g"] + _ACQ + ["sense", "idx", "val"],
    "gp_acq_lp": ["g"] + _ACQ + _LP + ["out"],
    "gp_acq_lp_argbest": ["g"] + _ACQ + _LP + ["sense", "exclude", "nex", "idx", "val"],
    "gp_predict_full_cov": ["g", "noise", "mean", "cov"],
    "gp_acq_topk": ["g"] + _ACQ + ["sense", "k", "idx", "val"],
    "gp_posterior_samples": ["g", "noise", "Z", "S", "maxtries", "mean", "dev", "scalar"],
    "gp_lml_grad": ["g", "scalar", "dl", "scalar2"],
    "gp_predict_grad": ["g", "dmdx", "dvdx"],
    "gp_acq_grad": ["g"] + _ACQ + ["out", "dout"],
    "gp_acq_lp_grad": ["g"] + _ACQ + _LP + ["out", "dout"],
    "gp_get_dl_dk": ["g", "cov"],
    "gp_predict_rows": ["g", "Xs", "M", "noise", "mean", "var", "dmdx", "dvdx"],
    "gp_acq_rows": ["g", "Xs", "M"] + _ACQ + ["lp"] + _LP + ["out", "dout"],
    "gp_comm_allgather_best": ["g", "par", "row", "out", "idx"],
    "gp_comm_allgather_topk": ["g", "k", "out", "idx", "val", "idx2"],
    "gp_group_acq_argbest": ["g"] + _ACQ + ["sense", "idx", "val"],
    "gp_group_acq_lp_argbest": ["g"] + _ACQ + _LP + ["sense", "exclude", "nex", "idx", "val"],
    "gp_group_acq_topk": ["g"] + _ACQ + ["sense", "k", "idx", "val"],
}
# fault -> what it overrides ("g": which context)
FAULTS = {
    "null output": None,            # the entry point's last required output, see _null_output
    "not fitted": {"g": "unfitted"},
    "no candidates": {"g": "bare"},
    "no communicator": {"g": "bare"},
    "P = 2": {"g": "two"},
    "type = 3": {"type": 3},
    "sense = 0": {"sense": 0},
    "k = 0": {"k": 0},
    "k = 65": {"k": 65},
    "nb = 257": {"nb": 257},
    "nb > 0, null batch": {"Xb": None},
    "nex = 257": {"nex": 257},
    "excluded row = M": {"exclude": "M"},
    "transform = 2": {"transform": 2},
    "M = 0": {"M": 0},
    "dvdx without dmdx": {"dmdx": None},
}
_NULL_OUTPUT = {"gp_predict_full_cov": "cov", "gp_posterior_samples": "dev", "gp_lml_grad": "dl", "gp_predict_grad": "dmdx",
                "gp_get_dl_dk": "cov", "gp_fmin": "scalar", "gp_comm_allgather_best": "out", "gp_comm_allgather_topk": "val",
                "gp_acq_grad": "dout", "gp_acq_lp_grad": "dout"}
# (entry point, single fault) -> code, as the parent of the scoring-layer refactor returned them.  "parent: accepted" marks the one
# deliberate change: transform outside {0, 1} used to be taken as 0 by these three and is refused as include/gphip.h documents.
CODES = [
    ("gp_predict", "not fitted", STATE), ("gp_predict", "no candidates", STATE),
    ("gp_fmin", "null output", ARG), ("gp_fmin", "not fitted", STATE), ("gp_fmin", "P = 2", ARG),
    ("gp_acq", "null output", ARG), ("gp_acq", "not fitted", STATE), ("gp_acq", "no candidates", STATE), ("gp_acq", "P = 2", ARG),
    ("gp_acq", "type = 3", ARG),
    ("gp_acq_argbest", "null output", ARG), ("gp_acq_argbest", "not fitted", STATE), ("gp_acq_argbest", "no candidates", STATE),
    ("gp_acq_argbest", "P = 2", ARG), ("gp_acq_argbest", "type = 3", ARG), ("gp_acq_argbest", "sense = 0", ARG),
    ("gp_acq_lp", "null output", ARG), ("gp_acq_lp", "not fitted", STATE), ("gp_acq_lp", "no candidates", STATE),
    ("gp_acq_lp", "P = 2", ARG), ("gp_acq_lp", "type = 3", ARG), ("gp_acq_lp", "nb = 257", ARG),
    ("gp_acq_lp", "nb > 0, null batch", ARG), ("gp_acq_lp", "transform = 2", ARG),   # parent: accepted
    ("gp_acq_lp_argbest", "null output", ARG), ("gp_acq_lp_argbest", "not fitted", STATE),
    ("gp_acq_lp_argbest", "no candidates", STATE), ("gp_acq_lp_argbest", "P = 2", ARG), ("gp_acq_lp_argbest", "type = 3", ARG),
    ("gp_acq_lp_argbest", "sense = 0", ARG), ("gp_acq_lp_argbest", "nb = 257", ARG),
    ("gp_acq_lp_argbest", "nb > 0, null batch", ARG), ("gp_acq_lp_argbest", "nex = 257", ARG),
    ("gp_acq_lp_argbest", "excluded row = M", ARG), ("gp_acq_lp_argbest", "transform = 2", ARG),   # parent: accepted
    ("gp_predict_full_cov", "null output", ARG), ("gp_predict_full_cov", "not fitted", STATE),
    ("gp_predict_full_cov", "no candidates", STATE),
    ("gp_acq_topk", "null output", ARG), ("gp_acq_topk", "not fitted", STATE), ("gp_acq_topk", "no candidates", STATE),
    ("gp_acq_topk", "P = 2", ARG), ("gp_acq_topk", "type = 3", ARG), ("gp_acq_topk", "sense = 0", ARG), ("gp_acq_topk", "k = 0", ARG),
    ("gp_acq_topk", "k = 65", ARG),
    ("gp_posterior_samples", "null output", ARG), ("gp_posterior_samples", "not fitted", STATE),
    ("gp_posterior_samples", "no candidates", STATE),
    ("gp_lml_grad", "null output", ARG), ("gp_lml_grad", "not fitted", STATE),
    ("gp_predict_grad", "null output", ARG), ("gp_predict_grad", "not fitted", STATE), ("gp_predict_grad", "no candidates", STATE),
    ("gp_acq_grad", "null output", ARG), ("gp_acq_grad", "not fitted", STATE), ("gp_acq_grad", "no candidates", STATE),
    ("gp_acq_grad", "P = 2", ARG), ("gp_acq_grad", "type = 3", ARG),
    ("gp_acq_lp_grad", "null output", ARG), ("gp_acq_lp_grad", "not fitted", STATE), ("gp_acq_lp_grad", "no candidates", STATE),
    ("gp_acq_lp_grad", "P = 2", ARG), ("gp_acq_lp_grad", "type = 3", ARG), ("gp_acq_lp_grad", "nb = 257", ARG),
    ("gp_acq_lp_grad", "nb > 0, null batch", ARG), ("gp_acq_lp_grad", "transform = 2", ARG),
    ("gp_get_dl_dk", "null output", ARG), ("gp_get_dl_dk", "not fitted", STATE),
    ("gp_predict_rows", "not fitted", STATE), ("gp_predict_rows", "M = 0", ARG), ("gp_predict_rows", "dvdx without dmdx", ARG),
    ("gp_acq_rows", "null output", ARG), ("gp_acq_rows", "not fitted", STATE), ("gp_acq_rows", "P = 2", ARG),
    ("gp_acq_rows", "type = 3", ARG), ("gp_acq_rows", "nb = 257", ARG), ("gp_acq_rows", "nb > 0, null batch", ARG),
    ("gp_acq_rows", "transform = 2", ARG), ("gp_acq_rows", "M = 0", ARG),
    ("gp_comm_allgather_best", "null output", ARG), ("gp_comm_allgather_best", "no communicator", STATE),
    ("gp_comm_allgather_topk", "null output", ARG), ("gp_comm_allgather_topk", "no communicator", STATE),
    ("gp_comm_allgather_topk", "k = 0", ARG), ("gp_comm_allgather_topk", "k = 65", ARG),
    ("gp_group_acq_argbest", "null output", ARG), ("gp_group_acq_argbest", "not fitted", STATE),
    ("gp_group_acq_argbest", "no candidates", STATE), ("gp_group_acq_argbest", "P = 2", ARG),
    ("gp_group_acq_argbest", "type = 3", ARG), ("gp_group_acq_argbest", "sense = 0", ARG),
    ("gp_group_acq_lp_argbest", "null output", ARG), ("gp_group_acq_lp_argbest", "not fitted", STATE),
    ("gp_group_acq_lp_argbest", "no candidates", STATE), ("gp_group_acq_lp_argbest", "P = 2", ARG),
    ("gp_group_acq_lp_argbest", "type = 3", ARG), ("gp_group_acq_lp_argbest", "sense = 0", ARG),
    ("gp_group_acq_lp_argbest", "nb = 257", ARG), ("gp_group_acq_lp_argbest", "nb > 0, null batch", ARG),
    ("gp_group_acq_lp_argbest", "nex = 257", ARG), ("gp_group_acq_lp_argbest", "excluded row = M", ARG),
    ("gp_group_acq_lp_argbest", "transform = 2", ARG),   # parent: accepted
    ("gp_group_acq_topk", "null output", ARG), ("gp_group_acq_topk", "not fitted", STATE),
    ("gp_group_acq_topk", "no candidates", STATE), ("gp_group_acq_topk", "P = 2", ARG), ("gp_group_acq_topk", "type = 3", ARG),
    ("gp_group_acq_topk", "sense = 0", ARG), ("gp_group_acq_topk", "k = 0", ARG), ("gp_group_acq_topk", "k = 65", ARG),
]
PARENT_ACCEPTED = {("gp_acq_lp", "transform = 2"), ("gp_acq_lp_argbest", "transform = 2"),
                   ("gp_group_acq_lp_argbest", "transform = 2")}


def _group(N, M, P=1, fit=True, candidates=True):
    X, Y, Xs = O.synthetic_problem(N, 3, M, seed=5)
    grp = _lib.Group((0, 0))
    grp.set_option("emulate_fp64", 0)
    grp.set_data(X, np.repeat(Y, P, axis=1))
    grp.set_params(_lib.GP_KERNEL_RBF, 0, 1.1, [0.4], 1e-2)
    if fit:
        grp.fit()
    if candidates:
        grp.set_candidates(Xs)
    return grp


def observed_codes(lib):
    """[(entry point, fault, code returned, valid arg-best afterwards == before)] for every row of CODES."""
    N, M = 100, 300   # (M > 257: the excluded-row faults are single faults)
    kinds = dict(ready={}, unfitted=dict(fit=False), bare=dict(candidates=False), two=dict(P=2))
    ctx = {k: _context(N, M, **kw)[0] for k, kw in kinds.items()}
    grp = {k: _group(N, M, **kw) for k, kw in kinds.items()}
    ctx["ready"].comm_init(ctx["ready"].comm_unique_id(), 0, 1)
    Xs = O.synthetic_problem(N, 3, M, seed=5)[2]
    dbuf = lambda n: np.zeros(n)
    vals = dict(noise=1, type=EI, par=0.01, fmin=0.0, y_mean=0.0, y_std=1.0, sense=-1, k=5, transform=1, nb=3, nex=2, lp=1,
                S=2, maxtries=5, row=7, M=4,
                Xb=dbuf(257 * 3), r0=dbuf(257) + 0.1, s0=dbuf(257) + 0.1, Xs=np.ascontiguousarray(Xs[:4]), Z=dbuf(2 * M),
                exclude=np.arange(257, dtype=np.int64), idx=np.zeros(64, dtype=np.int64), idx2=np.zeros(64, dtype=np.int64),
                out=dbuf(M), val=dbuf(64), dout=dbuf(M * 3), mean=dbuf(2 * M), var=dbuf(M), cov=dbuf(M * M), dev=dbuf(2 * M),
                dmdx=dbuf(2 * M * 3), dvdx=dbuf(M * 3), dl=dbuf(3), scalar=dbuf(1), scalar2=dbuf(1))

    def call(entry, over):
        fn = getattr(lib, entry)
        group = entry.startswith("gp_group")
        args = []
        for name, ctype in zip(ENTRIES[entry], fn.argtypes):
            v = over.get(name, vals.get(name))
            if name == "g":
                v = (grp if group else ctx)[over.get("g", "ready")].h
            elif name == "exclude" and isinstance(v, str):
                v = np.array([0, M], dtype=np.int64)
            if isinstance(v, np.ndarray):
                v = v.ctypes.data if ctype is ctypes.c_void_p else v.ctypes.data_as(ctype)
            args.append(v)
        return fn(*args)

    def valid(entry, over):
        where = over.get("g", "ready")
        if where != "ready":
            return None   # no arg-best is valid on a context that is not fitted / has no candidates / has two outputs
        return (grp if entry.startswith("gp_group") else ctx)[where].acq_argbest(EI, 0.01, 0.0, -1)

    got = []
    for entry, fault, _ in CODES:
        over = FAULTS[fault] or {_NULL_OUTPUT.get(entry, "out" if "out" in ENTRIES[entry] else "val"): None}
        before = valid(entry, over)
        code = call(entry, dict(over))
        got.append((entry, fault, code, valid(entry, over) == before))
    for o in list(ctx.values()) + list(grp.values()):
        o.close()
    return got


def test_refused_calls_return_the_parents_codes_and_leave_the_context_alone():
    """Every (entry point, single fault) of CODES through the raw symbols: the code is the one the table holds, and a valid
    gp_acq_argbest / gp_group_acq_argbest on the same context returns afterwards the bits it returned before."""
    got = observed_codes(_lib.load())
    wrong = [(e, f, code, want) for (e, f, code, _), (_, _, want) in zip(got, CODES) if code != want]
    assert not wrong, wrong
    disturbed = [(e, f) for e, f, _, same in got if not same]
    assert not disturbed, disturbed


def test_group_blocks_whose_rows_are_all_excluded():
    """Group((0, 0)), M = 4: block 0 = rows {0, 1}, block 1 = rows {2, 3}.  With both rows of block 0 excluded member 0 sits the
    call out and the winner is the single context's, from block 1.  With all four excluded no member scores anything: the group
    fails with GP_ERR_STATE, while the single context reduces over four masked values and returns row 0 with the empty value
    (both as recorded before the scoring-layer refactor; the two need not agree here)."""
    h, Xs = _context(100, 4)
    grp = _group(100, 4)
    fmin = h.fmin()
    Xb = Xs[1:2] + 0.01
    for sense, empty in ((-1, np.inf), (+1, -np.inf)):
        args = (EI, 0.01, fmin, 1, sense, Xb, R0[:1], S0[:1])
        i, v = grp.acq_lp_argbest(*args, exclude=(0, 1))
        assert i in (2, 3) and (i, v) == h.acq_lp_argbest(*args, exclude=(0, 1))
        assert grp.acq_lp_argbest(*args) == h.acq_lp_argbest(*args)
        assert h.acq_lp_argbest(*args, exclude=(0, 1, 2, 3)) == (0, empty)
        with pytest.raises(RuntimeError, match="no member produced a candidate"):
            grp.acq_lp_argbest(*args, exclude=(0, 1, 2, 3))
    grp.close()
    h.close()


def test_mean_gradient_rows_of_two_passes_equal_the_batched_mean_gradient():
    """gp_predict_rows with dmdx alone at M = 5 (a second pass of ONE location: the result block of a single location) and M = 8
    (two full passes) against gp_predict_grad(mean_only) of the same rows: 1e-9 relative, the bound tests/test_gpu_rows.py holds
    the fused route to against the batched one at noise 1e-2."""
    h, Xs = _context(300, 8)
    for M in (5, 8):
        jm = h.mean_grad_rows(Xs[:M])
        h.set_candidates(Xs[:M])
        ref = h.predict_grad(mean_only=True)
        assert jm.shape == ref.shape
        assert np.max(np.abs(jm - ref)) <= 1e-9 * np.max(np.abs(ref)), float(np.max(np.abs(jm - ref)))
    assert h.rows_stats() == dict(fused=2, fallback=0)
    h.close()
